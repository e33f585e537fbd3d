"""Sample moments and the adaptive render on the MI355X: mrt_moments_kernel bit for bit the host
mrt_moments (enqueued on a stream, capturable), and the GPU's mrt_render_adaptive bit for bit the CPU
backend's (the same decisions from the same moments, the same passes, the merge kernel)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_adaptive_host import assert_purpose, purpose_figures, wild_radiance
from test_aux_gpu import _bvh, _interpreter, _vsub
from test_aux_host import bits, ref_scene

pytestmark = pytest.mark.gpu

W, H, BASE = 40, 24, 4


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


# ---------------------------------------------------------------- 6. the moments kernel against the host
def device_moments(gpu, rad, n_pixels, n_samples, prior, slots=None, halves=False):
    """mrt_moments_device on a non-default stream, onto a copy of `prior` (float32 (slots, 4))."""
    import torch
    t_rad = torch.from_numpy(np.ascontiguousarray(rad)).cuda()
    t_m = torch.from_numpy(prior.copy()).cuda()
    t_s = torch.from_numpy(slots.astype(np.int32)).cuda() if slots is not None else None
    sp = t_s.data_ptr() if t_s is not None else 0
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    if halves:
        h = n_samples // 2
        gpu.moments_device(t_rad.data_ptr(), n_pixels, h, t_m.data_ptr(), sp, st.cuda_stream)
        gpu.moments_device(t_rad.data_ptr() + h * n_pixels * 12, n_pixels, n_samples - h, t_m.data_ptr(), sp, st.cuda_stream)
    else:
        gpu.moments_device(t_rad.data_ptr(), n_pixels, n_samples, t_m.data_ptr(), sp, st.cuda_stream)
    st.synchronize()
    assert np.array_equal(bits(t_rad.cpu().numpy()), bits(rad))  # the radiance is not written
    return t_m.cpu().numpy()


@pytest.mark.parametrize("n_pixels", [1, 63, 64, 65, 257, 1000])
def test_device_moments_equal_host_moments(gpu, n_pixels):
    """One below, at and above the kernel's in-flight depth, 1 and 33 samples; 257 and 1000 pixels are
    more than one 256-thread group; the prior moments are the test's (a second chunk resumes them)."""
    depth = gpu._lib.MOMENTS_DEPTH
    for n_samples in (1, depth - 1, depth, depth + 1, 33):
        rng = np.random.default_rng(n_pixels * 100 + n_samples)
        rad = wild_radiance(rng, n_pixels, n_samples)
        n_slots = n_pixels + 5
        prior = (rng.random((n_slots, 4)) * 3).astype(np.float32)
        want = gpu.moments(rad, n_pixels, n_samples, out=prior.copy())
        assert np.array_equal(bits(device_moments(gpu, rad, n_pixels, n_samples, prior)), bits(want))
        assert np.array_equal(bits(want[n_pixels:]), bits(prior[n_pixels:]))  # slots beyond the pixels stay
        slots = rng.permutation(n_slots)[:n_pixels].astype(np.uint32)
        swant = gpu.moments(rad, n_pixels, n_samples, slots=slots, out=prior.copy())
        assert np.array_equal(bits(device_moments(gpu, rad, n_pixels, n_samples, prior, slots=slots)), bits(swant))
        if n_samples > 1:
            assert np.array_equal(bits(device_moments(gpu, rad, n_pixels, n_samples, prior, slots=slots, halves=True)), bits(swant))


def test_device_moments_in_a_graph_capture(gpu):
    import torch
    n_pixels, n_samples = 300, 21
    rng = np.random.default_rng(7)
    rad = wild_radiance(rng, n_pixels, n_samples)
    slots = rng.permutation(n_pixels).astype(np.uint32)
    want = gpu.moments(rad, n_pixels, n_samples, slots=slots)
    t_rad = torch.from_numpy(rad).cuda()
    t_s = torch.from_numpy(slots.astype(np.int32)).cuda()
    t_m = torch.zeros((n_pixels, 4), dtype=torch.float32, device="cuda")

    def enqueue(stream_ptr):
        t_m.zero_()
        gpu.moments_device(t_rad.data_ptr(), n_pixels, n_samples, t_m.data_ptr(), t_s.data_ptr(), stream_ptr)

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        enqueue(side.cuda_stream)  # once outside the capture
    side.synchronize()
    assert np.array_equal(bits(t_m.cpu().numpy()), bits(want))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        t_m.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(t_m.cpu().numpy()), bits(want))
    del graph


# ---------------------------------------------------------------- 7. the adaptive render against the CPU backend
def cpu_case(mrt, sc, **kw):
    """The CPU backend's adaptive render of sc at 40 x 24, base 4 spp, 2 passes, atol = the median se
    of the pass-0 moments: (params, image, moments, rays)."""
    rc = mrt.Renderer(sc, "cpu")
    d = mrt.render_desc(W, H, BASE, **kw)
    _, m0, _ = rc.render_adaptive(d, mrt.default_adaptive_params(0))
    se = mrt.moments_se(m0)
    atol = float(np.median(se[np.isfinite(se)]))
    p = mrt.default_adaptive_params(2, atol, 0.0)
    out = rc.render_adaptive(d, p)
    rc.close()
    return p, out


def assert_same(got, want):
    assert np.array_equal(bits(got[0]), bits(want[0])), "image"
    assert np.array_equal(bits(got[1]), bits(want[1])), "moments"
    assert got[2] == want[2], "rays"


@pytest.mark.parametrize("sid", [5, 8])
def test_reference_scenes_equal_cpu_backend(gpu, sid):
    sc = ref_scene(gpu, sid, W / H)
    p, want = cpu_case(gpu, sc, tile_size=16)
    spent = want[1][..., 3]
    assert (spent == 4).any() and (spent > 4).any()
    rg = gpu.Renderer(sc, 0)
    assert_same(rg.render_adaptive(gpu.render_desc(W, H, BASE, tile_size=16), p), want)
    # several launches per pass: the moments resume across the chunks
    assert_same(rg.render_adaptive(gpu.render_desc(W, H, BASE, tile_size=16, chunk_samples=3), p), want)
    rg.close()


@pytest.mark.parametrize("build", [_interpreter, _bvh, _vsub], ids=["interpreter", "bvh_variant", "vsub_volume"])
def test_synthetic_graphs_equal_cpu_backend(gpu, build):
    s, kernel = build(gpu)
    p, want = cpu_case(gpu, s, tile_size=16)
    assert (want[1][..., 3] > 4).any()
    rg = gpu.Renderer(s, 0)
    got = rg.render_adaptive(gpu.render_desc(W, H, BASE, tile_size=16), p)
    assert rg.kernel_info()["kernel_features"] & 0xFFFF == kernel, hex(rg.kernel_info()["kernel_features"])
    assert_same(got, want)
    rg.close()


@pytest.mark.parametrize("sid", [5, 8])
def test_zero_passes_is_the_render_plus_moments_of_its_paths(gpu, sid):
    sc = ref_scene(gpu, sid, W / H)
    rg = gpu.Renderer(sc, 0)
    d = gpu.render_desc(W, H, 16, tile_size=16)
    img, rays = rg.render(d)
    aimg, mom, arays = rg.render_adaptive(d, gpu.default_adaptive_params(0))
    assert np.array_equal(bits(aimg), bits(img)) and arays == rays
    rg.render(gpu.render_desc(W, H, 16, tile_size=16, flags=gpu._lib.RF_PATH_DEBUG))
    px = gpu.local_pixels(d)
    prgb, _ = rg.paths(len(px) * 16)
    rg.close()
    want = gpu.moments(prgb, len(px), 16)  # [s][local pixel]
    assert np.array_equal(bits(mom.reshape(-1, 4)[px]), bits(want))
    assert (mom[..., 3] == 16).all()


def test_ranks_and_pixel_lists_equal_the_whole_image(gpu):
    sc = ref_scene(gpu, 5, W / H)
    p, want = cpu_case(gpu, sc, tile_size=8)
    rg = gpu.Renderer(sc, 0)
    uimg, umom, urays = np.zeros_like(want[0]), np.zeros_like(want[1]), 0
    for rank in range(3):
        dr = gpu.render_desc(W, H, BASE, tile_size=8, rank=rank, world=3)
        ri, rm, rr = rg.render_adaptive(dr, p)
        px = gpu.local_pixels(dr)
        rest = np.setdiff1d(np.arange(W * H), px)
        assert not ri.reshape(-1, 4)[rest].any() and not rm.reshape(-1, 4)[rest].any()  # owned pixels only
        uimg.reshape(-1, 4)[px] = ri.reshape(-1, 4)[px]
        umom.reshape(-1, 4)[px] = rm.reshape(-1, 4)[px]
        urays += rr
    assert_same((uimg, umom, urays), want)
    lst = np.random.default_rng(3).permutation(W * H)[: W * H // 2].astype(np.uint32)
    li, lm, _ = rg.render_adaptive(gpu.render_desc(W, H, BASE, pixels=lst), p)
    rg.close()
    assert np.array_equal(bits(li.reshape(-1, 4)[lst]), bits(want[0].reshape(-1, 4)[lst]))
    assert np.array_equal(bits(lm.reshape(-1, 4)[lst]), bits(want[1].reshape(-1, 4)[lst]))
    assert (lm.reshape(-1, 4)[lst][:, 3] > 4).any()


# ---------------------------------------------------------------- 8. the tolerance contract
def test_fast_numerics_unrefined_pixels_equal_the_plain_fast_render(gpu):
    rg = gpu.Renderer(ref_scene(gpu, 5, W / H), 0)
    d = gpu.render_desc(W, H, BASE, numerics="fast")
    plain, _ = rg.render(d)
    _, m0, _ = rg.render_adaptive(d, gpu.default_adaptive_params(0))
    atol = float(np.median(gpu.moments_se(m0)))
    img, mom, rays = rg.render_adaptive(d, gpu.default_adaptive_params(2, atol, 0.0))
    rg.close()
    un = mom[..., 3] == 4
    assert un.any() and (~un).any() and set(np.unique(mom[..., 3])) <= {4.0, 20.0, 84.0}
    assert np.array_equal(bits(img[un]), bits(plain[un]))
    assert not np.array_equal(bits(img[~un]), bits(plain[~un]))


def test_adaptive_beats_uniform_49spp_under_fast_numerics(gpu):
    assert_purpose(purpose_figures(gpu, 0, numerics="fast"))


# ---------------------------------------------------------------- 9. regression guard
def test_plain_renders_around_an_adaptive_render_are_unchanged(gpu):
    rg = gpu.Renderer(ref_scene(gpu, 5), 0)
    d = gpu.render_desc(48, 48, 9, numerics="fast")
    a, ra = rg.render(d)
    rg.render_adaptive(gpu.render_desc(W, H, BASE, numerics="fast", tile_size=8), gpu.default_adaptive_params(2, 0.05, 0.0))
    b, rb = rg.render(d)
    assert np.array_equal(bits(a), bits(b)) and ra == rb
    assert rg.kernel_info()["handover_lost"] == 0
    rg.close()


# ---------------------------------------------------------------- 10. the command-line driver
def test_cli_adaptive_on_the_gpu(gpu, tmp_path):
    """bin/mrt -adaptive 2 on the GPU backend, four ranks sharing the device (the host assembly): the
    image and the sample map equal the Python API's arrays bit for bit."""
    out, smap = tmp_path / "x.pfm", tmp_path / "n.pfm"
    args = ["-scene", "5", "-width", "40", "-height", "24", "-samples", "4"]
    res = subprocess.run([os.path.join(ROOT, "bin", "mrt")] + args + ["-numerics", "exact", "-gpus", "4", "-tilesize", "8", "-adaptive", "2",
                         "-atol", "0.05", "-o", str(out), "-samplemap", str(smap)], capture_output=True, text=True, timeout=120, check=True)
    p = gpu.ParseArgv(["mrt"] + args)
    r = gpu.Renderer(ref_scene(gpu, 5, 40 / 24), 0)
    d = gpu.render_desc(40, 24, 4, depth=p.max_bounces, max_luminance=p.max_luminance, mode=0, seed=p.seed, tile_size=8)
    img, mom, rays = r.render_adaptive(d, gpu.default_adaptive_params(2, 0.05))
    r.close()
    assert np.array_equal(bits(gpu.read_pfm(str(out))), bits(img[..., :3]))
    assert np.array_equal(bits(gpu.read_pfm(str(smap))), bits(np.repeat(mom[..., 3][..., None], 3, axis=2)))
    assert (mom[..., 3] > 4).any() and f"rays {rays}" in res.stdout.splitlines()
    assert any(ln.startswith("adaptive: ") for ln in res.stdout.splitlines())
