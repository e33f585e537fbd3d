"""Radiance queries (include/mrt.h "radiance queries") on the MI355X: mrt_trace_rays_device against the
CPU backend's records (which test_probe_host.py pins to the reference's own paths and the C
restatement), bit for bit; ragged batch sizes under every grid the workspace can select; stream order
beside renders; one graph capture; the fold on the device; the blocking form; edge-operand probes.
Batches of at most 4096 paths."""
import numpy as np
import pytest

from test_cast_host import BY_NAME, ENTRIES
from test_probe_host import (EDGE_DEPTH, EDGE_KEYS, bits, cpu_edge_records, cpu_renderer, cpu_stream_records, edge_case, entry_paths,
                             stream_case, words)
from test_synthetic_scenes import GEN, NOBVHW, NOSIG

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
PAD = 4096  # sentinel bytes behind the records and behind the workspace


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def device_trace(r, probes, depth, work_bytes=None, stream=None):
    """trace_rays_device of a PROBE_DTYPE array on `stream` (default: a new side stream) with
    `work_bytes` of workspace (default: the full grid's): the n records, whether the PAD bytes behind
    them and behind the workspace kept their sentinel, and the probe buffer read back."""
    import torch
    from miniraytracer_amd import RADIANCE_DTYPE
    n = len(probes)
    if work_bytes is None:
        work_bytes = r.trace_rays_workspace(depth)[0]
    d_probes = torch.from_numpy(np.ascontiguousarray(probes).view(np.uint8).copy()).cuda()
    d_out = torch.full((n * 16 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_work = torch.full((work_bytes + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = stream if stream is not None else torch.cuda.Stream()
    torch.cuda.synchronize()
    r.trace_rays_device(d_probes.data_ptr(), n, d_out.data_ptr(), d_work.data_ptr(), work_bytes, depth, stream_ptr=st.cuda_stream)
    st.synchronize()
    out = d_out.cpu().numpy()
    kept = bool((out[n * 16:] == SENTINEL).all()) and bool((d_work[work_bytes:] == SENTINEL).all().item())
    return out[:n * 16].view(RADIANCE_DTYPE), kept, d_probes.cpu().numpy().view(probes.dtype)


_gpu = {}


def gpu_renderer(mrt, sid):
    if sid not in _gpu:
        _gpu[sid] = mrt.Renderer(stream_case(mrt, sid)[0], 0)
    return _gpu[sid]


_many = {}


def many_probes(mrt, sid, n=1000):
    """(n probes spread over the fixture's paths, the CPU backend's records of them), computed once."""
    if sid not in _many:
        sc, d, g, _, _ = stream_case(mrt, sid)
        ns = d.sqrt_samples ** 2
        idx = (np.arange(n, dtype=np.int64) * 7919) % (g["w"] * g["h"] * ns)
        probes = mrt.camera_path_probes(sc.view.camera, d, idx // ns, idx % ns)
        _many[sid] = (probes, cpu_renderer(mrt, sid).trace_rays(probes, g["depth"])[0])
    return _many[sid]


def same_records(a, b):
    """Equal words; a NaN channel equals a NaN channel (x86 and gfx950 produce default NaNs of
    different sign, as in test_edge_rays_host.py); the ray counts equal."""
    wa, wb = words(a), words(b)
    fa, fb = wa[:, :3].view(np.float32), wb[:, :3].view(np.float32)
    return bool(((wa[:, :3] == wb[:, :3]) | (np.isnan(fa) & np.isnan(fb))).all()) and np.array_equal(wa[:, 3], wb[:, 3])


# ---------------------------------------------------------------- 7. both backends agree
@pytest.mark.parametrize("sid", range(10))
def test_device_records_equal_cpu_backend_and_reference_paths(gpu, sid):
    _, _, g, idx, probes = stream_case(gpu, sid)
    got, kept, back = device_trace(gpu_renderer(gpu, sid), probes, g["depth"])
    assert np.array_equal(words(got), words(cpu_stream_records(gpu, sid)[0]))
    assert np.array_equal(bits(got["L"]), bits(g["path_rgb"][idx])) and np.array_equal(got["rays"], g["path_rays"][idx].astype(np.uint32))
    assert kept and back.tobytes() == probes.tobytes()


def catalogue_case(mrt, e, depth=32):
    s, _, _, _, probes = entry_paths(mrt, e)
    r = mrt.Renderer(s, "cpu")
    want = r.trace_rays(probes, depth)[0]
    r.close()
    return s, probes, want


@pytest.mark.parametrize("e", [e for e in ENTRIES if e.gpu], ids=lambda e: e.name)
def test_catalogue_device_records_equal_cpu_backend(gpu, e):
    s, probes, want = catalogue_case(gpu, e)
    r = gpu.Renderer(s, 0)
    assert r.kernel_info()["kernel_features"] == e.kernel, (hex(r.kernel_info()["kernel_features"]), hex(e.kernel))
    got, kept, _ = device_trace(r, probes, 32)
    r.close()
    assert np.array_equal(words(got), words(want)) and kept


@pytest.mark.parametrize("name,hook", [("a_cornell_plus_sphere", GEN), ("b_cornell_lookalike", NOSIG), ("j_tree_list_leaves", NOBVHW)])
def test_catalogue_device_records_under_upload_hooks(gpu, monkeypatch, name, hook):
    """The same records from the kernel variant an upload hook selects instead."""
    e = BY_NAME[name]
    assert hook in e.hooks
    s, probes, want = catalogue_case(gpu, e)
    with monkeypatch.context() as mp:
        mp.setenv(hook, "1")
        r = gpu.Renderer(s, 0)
    assert r.kernel_info()["kernel_features"] != e.kernel or hook == NOBVHW, hook
    got, _, _ = device_trace(r, probes, 32)
    r.close()
    assert np.array_equal(words(got), words(want))


# ---------------------------------------------------------------- 8. ragged sizes and the grid
def test_workspace_sizes(gpu):
    r = gpu_renderer(gpu, 7)
    n_cu = r.kernel_info()["n_cu"]
    for depth in (0, 1, 8, 32):
        full, least = r.trace_rays_workspace(depth)
        assert least == 64 * max(depth, 1) * 16 and full % least == 0 and full // least >= n_cu
        assert (full, least) == gpu_renderer(gpu, 5).trace_rays_workspace(depth)  # the device and max_bounces only


@pytest.mark.parametrize("grid", ["min", "twice", "full"])
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_exactly_n_records_whatever_the_grid(gpu, n, grid):
    """work_bytes = bytes_min (one wave: each lane strides over up to 16 records), twice that, and
    bytes_full: the same records, exactly n of them, the probes and the bytes beyond work_bytes untouched."""
    probes, want = many_probes(gpu, 7)
    depth = stream_case(gpu, 7)[2]["depth"]
    r = gpu_renderer(gpu, 7)
    full, least = r.trace_rays_workspace(depth)
    got, kept, back = device_trace(r, probes[:n], depth, {"min": least, "twice": 2 * least, "full": full}[grid])
    assert np.array_equal(words(got), words(want)[:n])
    assert kept and back.tobytes() == probes[:n].tobytes()


def test_device_arguments(gpu):
    import torch
    r = gpu_renderer(gpu, 5)
    full, least = r.trace_rays_workspace(8)
    buf = torch.zeros(8192 + least, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    probes_ptr, out_ptr, work_ptr = p, p + 4096, p + 8192
    r.trace_rays_device(0, 0, 0, 0, 0, 8)  # n == 0: nothing enqueued, null pointers are fine
    cases = [(0, out_ptr, work_ptr, least), (probes_ptr, 0, work_ptr, least), (probes_ptr, out_ptr, 0, least),
             (probes_ptr + 4, out_ptr, work_ptr, least), (probes_ptr, out_ptr + 8, work_ptr, least), (probes_ptr, out_ptr, work_ptr + 4, least),
             (probes_ptr, out_ptr, work_ptr, least - 1), (probes_ptr, out_ptr, work_ptr, 0)]
    for a, b, c, nbytes in cases:
        with pytest.raises(gpu.MrtError):
            r.trace_rays_device(a, 4, b, c, nbytes, 8)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was enqueued
    with pytest.raises(gpu.MrtError):
        gpu.radiance_fold_device(p + 4, 1, 4, p + 4096)
    with pytest.raises(gpu.MrtError):
        gpu.radiance_fold_device(p, 1, 0, p + 4096)
    gpu.radiance_fold_device(0, 0, 4, 0)


# ---------------------------------------------------------------- 9. stream order and capture
def test_trace_between_two_renders_on_one_stream(gpu):
    """render, trace, render on one stream: both images and ray totals are a lone render's, the records
    a lone trace's."""
    import torch
    from test_aux_host import ref_scene
    probes, want = many_probes(gpu, 5)
    depth = stream_case(gpu, 5)[2]["depth"]
    r = gpu.Renderer(ref_scene(gpu, 5), 0)
    d = gpu.render_desc(48, 48, 16)
    n_local = len(gpu.local_pixels(d))
    r.prepare(d)
    st = torch.cuda.Stream()

    def buffers():
        return torch.full((n_local, 4), -1.0, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

    img0, rays0 = buffers()
    torch.cuda.synchronize()
    r.render_device(d, img0.data_ptr(), rays0.data_ptr(), st.cuda_stream)
    r.join(st.cuda_stream)
    st.synchronize()
    (img1, rays1), (img2, rays2) = buffers(), buffers()
    work_bytes = r.trace_rays_workspace(depth)[0]
    d_probes = torch.from_numpy(probes.view(np.uint8).copy()).cuda()
    d_out = torch.full((len(probes) * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_work = torch.zeros(work_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.render_device(d, img1.data_ptr(), rays1.data_ptr(), st.cuda_stream)
    r.trace_rays_device(d_probes.data_ptr(), len(probes), d_out.data_ptr(), d_work.data_ptr(), work_bytes, depth, stream_ptr=st.cuda_stream)
    r.render_device(d, img2.data_ptr(), rays2.data_ptr(), st.cuda_stream)
    r.join(st.cuda_stream)
    st.synchronize()
    base = bits(img0.cpu().numpy())
    assert int(rays0.item()) > 0 and (base != bits(np.full(1, -1.0, np.float32))[0]).any()
    for img, nr in ((img1, rays1), (img2, rays2)):
        assert np.array_equal(bits(img.cpu().numpy()), base) and int(nr.item()) == int(rays0.item())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32).reshape(-1, 4), words(want))
    r.close()


def test_captured_trace_replays_on_the_buffer_s_contents(gpu):
    """One trace_rays_device captured on a side stream; each replay traces what the probe buffer then holds."""
    import torch
    probes, want = many_probes(gpu, 7)
    depth = stream_case(gpu, 7)[2]["depth"]
    r = gpu_renderer(gpu, 7)
    n = 500
    first, second = probes[:n], probes[n:2 * n]
    work_bytes = r.trace_rays_workspace(depth)[0]
    d_probes = torch.from_numpy(first.view(np.uint8).copy()).cuda()
    d_out = torch.full((n * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_work = torch.zeros(work_bytes, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    args = (d_probes.data_ptr(), n, d_out.data_ptr(), d_work.data_ptr(), work_bytes, depth)
    r.trace_rays_device(*args, stream_ptr=side.cuda_stream)  # once outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        r.trace_rays_device(*args, stream_ptr=torch.cuda.current_stream().cuda_stream)
    for q, rec in ((second, want[n:2 * n]), (first, want[:n])):
        d_probes.copy_(torch.from_numpy(q.view(np.uint8).copy()))
        d_out.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32).reshape(-1, 4), words(rec))
    assert not np.array_equal(words(want[:n]), words(want[n:2 * n]))
    del graph


# ---------------------------------------------------------------- 10. the fold on the device
@pytest.mark.parametrize("sid", [5, 7])
def test_device_fold_equals_host_fold_and_the_render(gpu, sid):
    import torch
    sc = stream_case(gpu, sid)[0]
    W, H, spp, depth = 24, 16, 4, 16
    d = gpu.render_desc(W, H, spp, depth=depth, tile_size=max(W, H))  # one tile: local pixel order is row-major
    px = gpu.local_pixels(d)
    assert np.array_equal(px, np.arange(W * H))
    cam = gpu.make_camera(sc.camera_params(), aspect=W / H)
    r = gpu.Renderer(sc, 0)
    r.set_camera(cam)
    r.prepare(d)
    pix, sm = np.divmod(np.arange(W * H * spp), spp)
    probes = gpu.camera_path_probes(cam, d, pix, sm)
    work_bytes = r.trace_rays_workspace(depth)[0]
    st = torch.cuda.Stream()
    d_probes = torch.from_numpy(probes.view(np.uint8).copy()).cuda()
    d_rad = torch.zeros(len(probes) * 16, dtype=torch.uint8, device="cuda")
    d_work = torch.zeros(work_bytes, dtype=torch.uint8, device="cuda")
    d_rgb = torch.full((W * H, 4), -1.0, dtype=torch.float32, device="cuda")
    d_img = torch.full((W * H, 4), -1.0, dtype=torch.float32, device="cuda")
    d_rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    r.trace_rays_device(d_probes.data_ptr(), len(probes), d_rad.data_ptr(), d_work.data_ptr(), work_bytes, depth, stream_ptr=st.cuda_stream)
    gpu.radiance_fold_device(d_rad.data_ptr(), W * H, spp, d_rgb.data_ptr(), d.max_luminance, stream_ptr=st.cuda_stream)
    r.render_device(d, d_img.data_ptr(), d_rays.data_ptr(), st.cuda_stream)
    r.join(st.cuda_stream)
    st.synchronize()
    rad = d_rad.cpu().numpy().view(gpu.RADIANCE_DTYPE)
    folded = d_rgb.cpu().numpy()
    assert np.array_equal(bits(folded), bits(gpu.radiance_fold(rad, spp, d.max_luminance)))
    assert np.array_equal(bits(folded), bits(d_img.cpu().numpy())) and folded[:, :3].any()
    assert int(rad["rays"].sum()) == int(d_rays.item())
    # the NaN rule and the clamp, hand-made records
    hand = np.zeros(8, dtype=gpu.RADIANCE_DTYPE)
    hand["L"] = [(1, 2, 3), (np.nan, 0, 0), (0.5, 0.5, 0.5), (0, np.inf, 0), (4000, 4000, 4000), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    d_hand = torch.from_numpy(hand.view(np.uint8).copy()).cuda()
    d_two = torch.zeros((2, 4), dtype=torch.float32, device="cuda")
    gpu.radiance_fold_device(d_hand.data_ptr(), 2, 4, d_two.data_ptr(), 10.0, stream_ptr=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(bits(d_two.cpu().numpy()), bits(gpu.radiance_fold(hand, 4, 10.0)))
    r.close()


# ---------------------------------------------------------------- 11. the blocking form
@pytest.mark.parametrize("sid", [5, 7])
def test_blocking_trace_on_a_gpu_scene_equals_the_device_form(gpu, monkeypatch, sid):
    """Also with staging pieces of 300 records (the MRT_TRACE_PIECE_RECORDS hook: the piece is
    MRT_TRACE_PIECE = 2^20 records otherwise): 1000 probes are three whole pieces and a ragged one."""
    probes, want = many_probes(gpu, sid)
    depth = stream_case(gpu, sid)[2]["depth"]
    r = gpu_renderer(gpu, sid)
    got, _, _ = device_trace(r, probes, depth)
    assert np.array_equal(words(got), words(want))
    rad, total = r.trace_rays(probes, depth)
    assert np.array_equal(words(rad), words(got)) and total == int(got["rays"].sum())
    with monkeypatch.context() as mp:
        mp.setenv("MRT_TRACE_PIECE_RECORDS", "300")
        rad, total = r.trace_rays(probes, depth)
        assert np.array_equal(words(rad), words(got)) and total == int(got["rays"].sum())
    assert np.array_equal(words(r.trace_rays(probes[:65], depth)[0]), words(got)[:65])  # a smaller batch reuses the staging records


# ---------------------------------------------------------------- 12. edge-operand and non-finite probes
@pytest.mark.parametrize("key", EDGE_KEYS)
def test_edge_and_non_finite_probes_equal_cpu_backend(gpu, key):
    sc, probes = edge_case(gpu, key)
    want = cpu_edge_records(gpu, key)
    r = gpu.Renderer(sc, 0)
    least = r.trace_rays_workspace(EDGE_DEPTH)[1]
    got, kept, _ = device_trace(r, probes, EDGE_DEPTH)
    one_wave, kept1, _ = device_trace(r, probes, EDGE_DEPTH, 4 * least)
    r.close()
    assert kept and kept1
    assert (got["rays"] >= 1).all() and (got["rays"] <= EDGE_DEPTH + 1).all()
    assert same_records(got, want), int((words(got) != words(want)).any(axis=1).sum())
    assert same_records(one_wave, want)
