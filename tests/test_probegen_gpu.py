"""The probe generators (include/mrt.h "probe generators", mrt_camera_pixel_rays_device) on the MI355X:
each device form against its host form (which test_probegen_host.py pins to the per-record functions and
the header's formulas), byte for byte; the argument rules; the device pipelines against the CPU
backend's host pipelines; one graph capture of generate -> trace -> fold; stream order beside renders;
mrt_radiance_rays_device; bin/mrt -pano on the GPU.  Batches of a few thousand records."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_probe_gpu import PAD, SENTINEL, same_records
from test_probe_host import bits, stream_case
from test_probegen_host import (H, NPATH, PIPE_DEPTH, PIPE_SQ, PROBE_RANGES, RAY_RANGES, SPP, W, desc, hit_records, pano_pipeline, surface_pipeline,
                                unit_normals)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def device_records(enqueue, n, dtype):
    """n 48-byte records written by enqueue(d_out_ptr, stream_ptr) on a new side stream, and whether the
    PAD bytes behind them kept their sentinel."""
    import torch
    d_out = torch.full((n * 48 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    enqueue(d_out.data_ptr(), st.cuda_stream)
    st.synchronize()
    out = d_out.cpu().numpy()
    return out[:n * 48].view(dtype), bool((out[n * 48:] == SENTINEL).all())


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


# ---------------------------------------------------------------- 1. device form equals host form
@pytest.mark.parametrize("sid", range(10))
def test_range_generators_equal_their_host_forms(gpu, sid):
    sc = stream_case(gpu, sid)[0]
    cam, cp, d = sc.view.camera, sc.camera_params(), desc(gpu)
    for first, n in PROBE_RANGES:
        got, kept = device_records(lambda o, s: gpu.camera_path_probes_device(cam, d, first, n, o, s), n, gpu.PROBE_DTYPE)
        assert got.tobytes() == gpu.camera_path_probe_range(cam, d, first, n).tobytes() and kept, ("camera", first, n)
        got, kept = device_records(lambda o, s: gpu.pano_probes_device(cp, d, first, n, o, s), n, gpu.PROBE_DTYPE)
        assert got.tobytes() == gpu.pano_probe_range(cp, d, first, n).tobytes() and kept, ("pano", first, n)
    for first, n in RAY_RANGES:
        got, kept = device_records(lambda o, s: gpu.camera_pixel_rays_device(cam, W, H, first, n, o, s), n, gpu.RAY_DTYPE)
        assert got.tobytes() == gpu.camera_pixel_ray_range(cam, W, H, first, n).tobytes() and kept, ("rays", first, n)


def test_range_generators_past_32_bits_of_path_index(gpu):
    """A render whose path indices need 64 bits: the kernels' 64-bit split, at ranges on both sides of 2^32."""
    sc = stream_case(gpu, 0)[0]
    cam, cp = sc.view.camera, sc.camera_params()
    d = gpu.render_desc(4096, 2048, 1024)  # 2^33 paths
    for first in (2 ** 32 - 100, 2 ** 32 + 12345, 2 ** 33 - 300):
        got, kept = device_records(lambda o, s: gpu.camera_path_probes_device(cam, d, first, 300, o, s), 300, gpu.PROBE_DTYPE)
        assert got.tobytes() == gpu.camera_path_probe_range(cam, d, first, 300).tobytes() and kept, first
        got, kept = device_records(lambda o, s: gpu.pano_probes_device(cp, d, first, 300, o, s), 300, gpu.PROBE_DTYPE)
        assert got.tobytes() == gpu.pano_probe_range(cp, d, first, 300).tobytes() and kept, first
    Wb, Hb = 2 ** 17, 2 ** 16  # 2^33 pixels
    for first in (2 ** 32 - 100, 2 ** 33 - 300):
        got, kept = device_records(lambda o, s: gpu.camera_pixel_rays_device(cam, Wb, Hb, first, 300, o, s), 300, gpu.RAY_DTYPE)
        assert got.tobytes() == gpu.camera_pixel_ray_range(cam, Wb, Hb, first, 300).tobytes() and kept, first


@pytest.mark.parametrize("n,sq", [(1, 1), (63, 1), (65, 2), (1000, 2), (257, 3), (300, 4)])
def test_surface_probes_device_equals_host_form(gpu, n, sq):
    rng = np.random.default_rng(600 + n)
    hits = hit_records(gpu, rng, n, misses=tuple(range(0, n, 7)))
    rays = np.zeros(n, dtype=gpu.RAY_DTYPE)
    rays["d"], rays["time"] = unit_normals(rng, n), rng.uniform(0, 1, n).astype(np.float32)
    d_hits, d_rays = upload(hits), upload(rays)
    total = n * sq * sq
    for with_rays in (False, True):
        want = gpu.surface_probes(hits, rays if with_rays else None, sqrt_per_hit=sq, seed=77, first_id=2 ** 64 - 500)
        got, kept = device_records(lambda o, s: gpu.surface_probes_device(d_hits.data_ptr(), d_rays.data_ptr() if with_rays else 0, n, o, sq, 77,
                                                                          2 ** 64 - 500, s), total, gpu.PROBE_DTYPE)
        assert got.tobytes() == want.tobytes() and kept, with_rays
    assert d_hits.cpu().numpy().tobytes() == hits.tobytes() and d_rays.cpu().numpy().tobytes() == rays.tobytes()  # inputs unchanged


# ---------------------------------------------------------------- 2. arguments
def test_device_arguments(gpu):
    import torch
    sc = stream_case(gpu, 5)[0]
    cam, cp, d = sc.view.camera, sc.camera_params(), desc(gpu)
    buf = torch.zeros(3 * 4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    out, hits, rays = p, p + 4096, p + 8192
    calls = []
    for o in (0, out + 4, out + 8):
        calls += [lambda o=o: gpu.camera_path_probes_device(cam, d, 0, 4, o), lambda o=o: gpu.pano_probes_device(cp, d, 0, 4, o),
                  lambda o=o: gpu.camera_pixel_rays_device(cam, W, H, 0, 4, o), lambda o=o: gpu.surface_probes_device(hits, rays, 4, o, 2),
                  lambda o=o: gpu.surface_probes_device(hits, 0, 4, o, 2)]
    calls += [lambda: gpu.surface_probes_device(0, rays, 4, out, 2), lambda: gpu.surface_probes_device(hits + 4, rays, 4, out, 2),
              lambda: gpu.surface_probes_device(hits, rays + 8, 4, out, 2), lambda: gpu.surface_probes_device(hits, rays, 4, out, 0),
              lambda: gpu.surface_probes_device(hits, rays, 2 ** 28, out, 4),
              lambda: gpu.camera_path_probes_device(cam, d, NPATH - 3, 4, out), lambda: gpu.pano_probes_device(cp, d, NPATH - 3, 4, out),
              lambda: gpu.camera_pixel_rays_device(cam, W, H, W * H - 3, 4, out), lambda: gpu.camera_pixel_rays_device(cam, 0, H, 0, 4, out),
              lambda: gpu.radiance_rays_device(0, 4, out), lambda: gpu.radiance_rays_device(hits + 4, 4, out),
              lambda: gpu.radiance_rays_device(hits, 4, 0), lambda: gpu.radiance_rays_device(hits, 4, out + 4)]
    for c in calls:
        with pytest.raises(gpu.MrtError):
            c()
    # n == 0: nothing enqueued, null pointers are fine
    gpu.camera_path_probes_device(cam, d, 0, 0, 0)
    gpu.pano_probes_device(cp, d, 0, 0, 0)
    gpu.camera_pixel_rays_device(cam, W, H, 0, 0, 0)
    gpu.surface_probes_device(0, 0, 0, 0, 2)
    gpu.radiance_rays_device(0, 0, 0)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was enqueued


# ---------------------------------------------------------------- 3. device pipelines equal the CPU backend's
_gpu = {}


def gpu_renderer(mrt, sid):
    if sid not in _gpu:
        _gpu[sid] = mrt.Renderer(stream_case(mrt, sid)[0], 0)
    return _gpu[sid]


@pytest.mark.parametrize("sid", [5, 7])
def test_surface_pipeline_on_one_stream_equals_the_cpu_backend(gpu, sid):
    import torch
    rays, hits, probes, rad, rgb = surface_pipeline(gpu, sid)
    sc = stream_case(gpu, sid)[0]
    cam = gpu.make_camera(sc.camera_params(), aspect=W / H)
    r = gpu_renderer(gpu, sid)
    npx, P = W * H, PIPE_SQ * PIPE_SQ
    work_bytes = r.trace_rays_workspace(PIPE_DEPTH)[0]
    d_rays = torch.full((npx * 48 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((npx * 32 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_probes = torch.full((npx * P * 48 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_rad = torch.full((npx * P * 16 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_rgb = torch.full((npx * 16 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_work = torch.zeros(work_bytes, dtype=torch.uint8, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    s = st.cuda_stream
    torch.cuda.synchronize()
    gpu.camera_pixel_rays_device(cam, W, H, 0, npx, d_rays.data_ptr(), s)
    r.cast_rays_device(d_rays.data_ptr(), npx, d_hits.data_ptr(), seed=3, stream_ptr=s)
    gpu.surface_probes_device(d_hits.data_ptr(), d_rays.data_ptr(), npx, d_probes.data_ptr(), PIPE_SQ, 11, 0, s)
    r.trace_rays_device(d_probes.data_ptr(), npx * P, d_rad.data_ptr(), d_work.data_ptr(), work_bytes, PIPE_DEPTH, stream_ptr=s)
    gpu.radiance_rays_device(d_rad.data_ptr(), npx * P, d_total.data_ptr(), s)
    gpu.radiance_fold_device(d_rad.data_ptr(), npx, P, d_rgb.data_ptr(), 1000.0, stream_ptr=s)
    st.synchronize()
    for buf, n in ((d_rays, npx * 48), (d_hits, npx * 32), (d_probes, npx * P * 48), (d_rad, npx * P * 16), (d_rgb, npx * 16)):
        assert bool((buf[n:] == SENTINEL).all().item())
    assert d_rays.cpu().numpy()[:npx * 48].tobytes() == rays.tobytes()
    assert d_hits.cpu().numpy()[:npx * 32].tobytes() == hits.tobytes()
    assert d_probes.cpu().numpy()[:npx * P * 48].tobytes() == probes.tobytes()
    got = d_rad.cpu().numpy()[:npx * P * 16].view(gpu.RADIANCE_DTYPE)
    assert same_records(got, rad)
    f, g = d_rgb.cpu().numpy()[:npx * 16].view(np.float32).reshape(-1, 4), rgb
    assert bool(((bits(f) == bits(g)) | (np.isnan(f) & np.isnan(g))).all())
    assert int(d_total.item()) == int(rad["rays"].sum())


@pytest.mark.parametrize("sid", [5, 7])
def test_pano_pipeline_on_one_stream_equals_the_cpu_backend(gpu, sid):
    import torch
    probes, rad, rgb = pano_pipeline(gpu, sid)
    sc = stream_case(gpu, sid)[0]
    d = desc(gpu, depth=PIPE_DEPTH)
    r = gpu_renderer(gpu, sid)
    work_bytes = r.trace_rays_workspace(PIPE_DEPTH)[0]
    d_probes = torch.zeros(NPATH * 48, dtype=torch.uint8, device="cuda")
    d_rad = torch.zeros(NPATH * 16, dtype=torch.uint8, device="cuda")
    d_rgb = torch.full((W * H, 4), -1.0, dtype=torch.float32, device="cuda")
    d_work = torch.zeros(work_bytes, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.pano_probes_device(sc.camera_params(), d, 0, NPATH, d_probes.data_ptr(), st.cuda_stream)
    r.trace_rays_device(d_probes.data_ptr(), NPATH, d_rad.data_ptr(), d_work.data_ptr(), work_bytes, PIPE_DEPTH, stream_ptr=st.cuda_stream)
    gpu.radiance_fold_device(d_rad.data_ptr(), W * H, SPP, d_rgb.data_ptr(), d.max_luminance, stream_ptr=st.cuda_stream)
    st.synchronize()
    assert d_probes.cpu().numpy().tobytes() == probes.tobytes()
    assert same_records(d_rad.cpu().numpy().view(gpu.RADIANCE_DTYPE), rad)
    f = d_rgb.cpu().numpy()
    assert bool(((bits(f) == bits(rgb)) | (np.isnan(f) & np.isnan(rgb))).all()) and f[:, :3].any()


# ---------------------------------------------------------------- 4. one capture
def test_captured_chain_replays_on_the_hit_buffer_s_contents(gpu):
    """surface probes -> trace -> fold captured once on a side stream, replayed on two hit buffers: each
    replay's pixels are the host chain's on that buffer's contents."""
    import torch
    sid = 5
    rays, hits, _, _, _ = surface_pipeline(gpu, sid)
    n, P = 200, PIPE_SQ * PIPE_SQ
    first, second = hits[:n], hits[len(hits) - n:]
    cpu = gpu.Renderer(stream_case(gpu, sid)[0], "cpu")
    want = [gpu.radiance_fold(cpu.trace_rays(gpu.surface_probes(h, None, sqrt_per_hit=PIPE_SQ, seed=21), PIPE_DEPTH)[0], P, 1000.0) for h in (first, second)]
    cpu.close()
    assert not np.array_equal(bits(want[0]), bits(want[1]))
    r = gpu_renderer(gpu, sid)
    work_bytes = r.trace_rays_workspace(PIPE_DEPTH)[0]
    d_hits = upload(first)
    d_probes = torch.zeros(n * P * 48, dtype=torch.uint8, device="cuda")
    d_rad = torch.zeros(n * P * 16, dtype=torch.uint8, device="cuda")
    d_rgb = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    d_work = torch.zeros(work_bytes, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()

    def chain(s):
        gpu.surface_probes_device(d_hits.data_ptr(), 0, n, d_probes.data_ptr(), PIPE_SQ, 21, 0, s)
        r.trace_rays_device(d_probes.data_ptr(), n * P, d_rad.data_ptr(), d_work.data_ptr(), work_bytes, PIPE_DEPTH, stream_ptr=s)
        gpu.radiance_fold_device(d_rad.data_ptr(), n, P, d_rgb.data_ptr(), 1000.0, stream_ptr=s)

    torch.cuda.synchronize()
    chain(side.cuda_stream)  # once outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain(torch.cuda.current_stream().cuda_stream)
    outs = []
    for h, w in ((second, want[1]), (first, want[0])):
        d_hits.copy_(upload(h))
        d_rgb.fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        f = d_rgb.cpu().numpy()
        assert bool(((bits(f) == bits(w)) | (np.isnan(f) & np.isnan(w))).all())
        outs.append(f)
    assert not np.array_equal(bits(outs[0]), bits(outs[1]))
    del graph


# ---------------------------------------------------------------- 5. stream order
def test_generators_between_two_renders_on_one_stream(gpu):
    import torch
    from test_aux_host import ref_scene
    sc = stream_case(gpu, 5)[0]
    cam, cp = sc.view.camera, sc.camera_params()
    r = gpu.Renderer(ref_scene(gpu, 5), 0)
    d = gpu.render_desc(48, 48, 16)
    n_local = len(gpu.local_pixels(d))
    r.prepare(d)
    st = torch.cuda.Stream()

    def buffers():
        return torch.full((n_local, 4), -1.0, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

    (img0, rays0), (img1, rays1), (img2, rays2) = buffers(), buffers(), buffers()
    gd = desc(gpu)
    d_a = torch.zeros(NPATH * 48, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(NPATH * 48, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.render_device(d, img0.data_ptr(), rays0.data_ptr(), st.cuda_stream)
    r.join(st.cuda_stream)
    st.synchronize()
    r.render_device(d, img1.data_ptr(), rays1.data_ptr(), st.cuda_stream)
    gpu.camera_path_probes_device(cam, gd, 0, NPATH, d_a.data_ptr(), st.cuda_stream)
    gpu.pano_probes_device(cp, gd, 0, NPATH, d_b.data_ptr(), st.cuda_stream)
    r.render_device(d, img2.data_ptr(), rays2.data_ptr(), st.cuda_stream)
    r.join(st.cuda_stream)
    st.synchronize()
    base = bits(img0.cpu().numpy())
    assert int(rays0.item()) > 0
    for img, nr in ((img1, rays1), (img2, rays2)):
        assert np.array_equal(bits(img.cpu().numpy()), base) and int(nr.item()) == int(rays0.item())
    assert d_a.cpu().numpy().tobytes() == gpu.camera_path_probe_range(cam, gd, 0, NPATH).tobytes()
    assert d_b.cpu().numpy().tobytes() == gpu.pano_probe_range(cp, gd, 0, NPATH).tobytes()
    r.close()


# ---------------------------------------------------------------- 6. the ray total
@pytest.mark.parametrize("n", [1, 63, 65, 1000, 300001])
def test_radiance_rays_device_adds_the_ray_counts(gpu, n):
    import torch
    rng = np.random.default_rng(n)
    rad = np.zeros(n, dtype=gpu.RADIANCE_DTYPE)
    rad["L"] = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    rad["rays"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)  # sums past 2^32
    d_rad = upload(rad)
    d_total = torch.full((3,), 5, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.radiance_rays_device(d_rad.data_ptr(), n, d_total.data_ptr() + 8, st.cuda_stream)
    gpu.radiance_rays_device(d_rad.data_ptr(), n, d_total.data_ptr() + 8, st.cuda_stream)  # accumulates
    st.synchronize()
    assert d_total.cpu().tolist() == [5, 5 + 2 * int(rad["rays"].astype(np.uint64).sum()), 5]
    assert d_rad.cpu().numpy().tobytes() == rad.tobytes()


# ---------------------------------------------------------------- 7. the command line
def test_cli_pano_on_the_gpu_equals_the_host_chain(gpu, tmp_path):
    Wc, Hc, spp = 32, 16, 4
    a = tmp_path / "a.pfm"
    cmd = [os.path.join(ROOT, "bin", "mrt"), "-scene", 5, "-width", Wc, "-height", Hc, "-samples", spp, "-pano", "-o", a]
    out = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=120, check=True).stdout
    sc = gpu.select_scene(5, Wc / Hc)
    d = gpu.render_desc(Wc, Hc, spp)
    r = gpu.Renderer(sc, "cpu")
    rad, total = r.trace_rays(gpu.pano_probe_range(sc.camera_params(), d, 0, Wc * Hc * spp), 32)
    r.close()
    img = gpu.radiance_fold(rad, spp, 1000.0).reshape(Hc, Wc, 4)
    assert np.array_equal(bits(gpu.read_pfm(str(a))), bits(img[..., :3])) and img[..., :3].any()
    assert f"rays {total}\n" in out
