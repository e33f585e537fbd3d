"""First-hit feature buffers and the a-trous filter on the MI355X: mrt_aux_kernel<F> bit for bit the
CPU backend's buffers (the same source compiled for the host), mrt_atrous_kernel bit for bit the host
mrt_denoise, both enqueued on a stream and capturable."""
import numpy as np
import pytest

from test_aux_host import (EDGE_SIGMA_NORMALS, bits, black_cornell, cornell_16spp, edge_weight_frames, params, random_guides, ref_scene, rmse,
                           seq_mean)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def both(mrt, sc, d):
    """(GPU renderer, its buffers, the CPU backend's buffers) for one desc."""
    rc = mrt.Renderer(sc, "cpu")
    want = rc.render_aux(d)
    rc.close()
    rg = mrt.Renderer(sc, 0)
    return rg, rg.render_aux(d), want


def assert_same(got, want):
    for k in range(2):
        assert np.array_equal(bits(got[k]), bits(want[k])), ("normal", "albedo")[k]


# ---------------------------------------------------------------- 7. bit-exactness against the CPU backend
@pytest.mark.parametrize("sid", range(10))
def test_reference_scenes_equal_cpu_backend(gpu, sid):
    w, h, spp = 40, 24, 4
    d = gpu.render_desc(w, h, spp, tile_size=16)
    rg, got, want = both(gpu, ref_scene(gpu, sid, w / h), d)
    assert (want[0][..., 3] > 0).any()
    assert_same(got, want)
    assert_same(rg.render_aux(gpu.render_desc(w, h, spp, tile_size=16, numerics="fast")), want)  # MRT_RF_FAST: the same bits
    rg.close()


def _interpreter(m):
    from test_synthetic_scenes import b_biased_sphere
    return b_biased_sphere(m)[0], 0x3FFF  # LIN | ALL: the interpreter


def _bvh(m):
    from test_synthetic_scenes import b_bvh_in_room
    return b_bvh_in_room(m, 2)[0], 0x3CFC  # the lit bvh_node variant (book2's)


def _vsub(m):
    from test_synthetic_scenes import smoke_plus
    return smoke_plus(m, False)[0], 0x684C  # volumes bounded by sub-programs (Cornell smoke's)


@pytest.mark.parametrize("build", [_interpreter, _bvh, _vsub], ids=["interpreter", "bvh_variant", "vsub_volume"])
def test_synthetic_graphs_equal_cpu_backend(gpu, build):
    s, kernel = build(gpu)
    d = gpu.render_desc(40, 24, 4, tile_size=16)
    rg, got, want = both(gpu, s, d)
    assert rg.kernel_info()["kernel_features"] & 0xFFFF == kernel, hex(rg.kernel_info()["kernel_features"])
    assert (want[0][..., 3] > 0).any()
    assert_same(got, want)
    rg.close()


@pytest.mark.parametrize("sid", [5, 8])
def test_device_entry_ranks_and_pixel_lists(gpu, sid):
    """render_aux_device into torch tensors on a non-default stream == render_aux; the union of the
    world=3 ranks and a shuffled pixel list == the whole image."""
    import torch
    w, h, spp, ts = 40, 24, 4, 16
    d = gpu.render_desc(w, h, spp, tile_size=ts)
    rg, whole, want = both(gpu, ref_scene(gpu, sid, w / h), d)
    assert_same(whole, want)
    st = torch.cuda.Stream()
    union = [np.zeros((w * h, 4), dtype=np.float32) for _ in range(2)]
    px_list = np.random.default_rng(sid).permutation(w * h)[:300].astype(np.uint32)
    descs = [gpu.render_desc(w, h, spp, tile_size=ts, rank=r, world=3) for r in range(3)] + [gpu.render_desc(w, h, spp, tile_size=ts, pixels=px_list)]
    for i, dr in enumerate(descs):
        px = gpu.local_pixels(dr)
        rg.prepare(dr)
        t = [torch.full((len(px), 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        rg.render_aux_device(dr, t[0].data_ptr(), t[1].data_ptr(), st.cuda_stream)
        st.synchronize()
        host = rg.render_aux(dr)
        for k in range(2):
            loc = t[k].cpu().numpy()
            assert np.array_equal(bits(loc), bits(host[k].reshape(-1, 4)[px]))  # device entry == host entry, local-pixel order
            if i < 3:
                union[k][px] = loc
            else:
                assert np.array_equal(px, px_list) and np.array_equal(bits(loc), bits(want[k].reshape(-1, 4)[px_list]))
    for k in range(2):
        assert np.array_equal(bits(union[k]), bits(want[k].reshape(-1, 4)))
    rg.close()


@pytest.mark.parametrize("which", ["5", "5-black"])
def test_depth0_paths_fold_to_albedo_on_the_gpu(gpu, which):
    """Item 1 with Renderer.paths (MRT_RF_PATH_DEBUG): the depth-0 per-path radiance, summed in float32
    in sample order and divided by 16, is the albedo buffer on all-light / all-miss pixels -- on
    every pixel of the blackened Cornell box (tests/test_aux_host.py black_cornell)."""
    w = h = 32
    sc = black_cornell(gpu) if which == "5-black" else ref_scene(gpu, 5)
    r = gpu.Renderer(sc, 0)
    d = gpu.render_desc(w, h, 16, depth=0, flags=gpu._lib.RF_PATH_DEBUG)
    r.render(d)
    px = gpu.local_pixels(d)
    prgb, _ = r.paths(len(px) * 16)
    full = np.zeros((w * h, 16, 3), dtype=np.float32)
    full[px] = prgb.reshape(16, len(px), 3).transpose(1, 0, 2)
    nrm, alb = r.render_aux(gpu.render_desc(w, h, 16, depth=0))
    r.close()
    allmiss = (nrm[..., 3] == 0).ravel()
    alllight = (full.max(axis=2) > 1.0).all(axis=1) & (nrm[..., 3] == 1).ravel()
    mask = np.ones(w * h, dtype=bool) if which == "5-black" else allmiss | alllight
    assert np.array_equal(bits(seq_mean(full)[mask]), bits(alb.reshape(-1, 4)[mask][:, :3]))


# ---------------------------------------------------------------- 8. the filter on the device
def device_denoise(gpu, img, nrm, alb, p):
    import torch
    h, w = img.shape[:2]
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in (img, nrm, alb)]
    out = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    tmp = torch.full((h, w, 4), -2.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.denoise_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), w, h, out.data_ptr(), tmp.data_ptr(), p, st.cuda_stream)
    st.synchronize()
    assert np.array_equal(bits(t[0].cpu().numpy()), bits(img))  # d_rgb is not written
    return out.cpu().numpy()


@pytest.mark.parametrize("w,h,it", [(37, 23, 5), (1, 1, 5), (5, 3, 5), (67, 45, 4), (67, 45, 1), (9, 11, 0)])
def test_device_filter_equals_host_filter(gpu, w, h, it):
    """Random guides and colours; 67 x 45 is no multiple of the 64 x 4 workgroup either way; an even
    and an odd pass count (the last pass lands in d_out both ways); 0 passes copy."""
    rng = np.random.default_rng(w * 1000 + h * 10 + it)
    nrm, alb = random_guides(rng, h, w)
    nrm[..., :3] += np.float32(2.0) * (nrm[..., :3] != 0)
    img = rng.random((h, w, 4)).astype(np.float32)
    p = params(gpu, it, sigma_color=1.0, sigma_normal=4.0, sigma_albedo=0.8, sigma_depth=1.5)
    assert np.array_equal(bits(device_denoise(gpu, img, nrm, alb, p)), bits(gpu.denoise(img, nrm, alb, p)))


@pytest.mark.parametrize("sn", EDGE_SIGMA_NORMALS)
def test_device_filter_equals_host_filter_at_the_edges_of_exp_and_pow(gpu, sn):
    """tests/test_aux_host.py edge_weight_frames: summed exponents 0 ... ~110, so float-subnormal and
    exactly-zero weights, under sigma_normal 0.25, 5 (mrt_powf's pow5 shortcut) and 128."""
    img, nrm, alb, (it, kw) = edge_weight_frames(sn)
    p = params(gpu, it, **kw)
    assert np.array_equal(bits(device_denoise(gpu, img, nrm, alb, p)), bits(gpu.denoise(img, nrm, alb, p)))


def test_device_filter_keeps_constant_colours_apart(gpu):
    """Item 4's half-images on the device, against the host's bits."""
    w, h = 32, 20
    nrm = np.zeros((h, w, 4), dtype=np.float32)
    nrm[:, :w // 2, 0] = 1
    nrm[:, w // 2:, 2] = 1
    alb = np.broadcast_to(np.array([0.5, 0.5, 0.5, 7.0], dtype=np.float32), (h, w, 4)).copy()
    img = np.zeros((h, w, 4), dtype=np.float32)
    img[:, :w // 2], img[:, w // 2:] = (1.0, 0.25, 3.0, 0.0), (0.1, 4.0, 0.5, 0.0)
    p = params(gpu, 5, sigma_color=1e3)
    out = device_denoise(gpu, img, nrm, alb, p)
    assert np.array_equal(bits(out), bits(gpu.denoise(img, nrm, alb, p)))
    assert np.abs(out - img).max() <= 2e-5 * 4.1


def test_cli_denoise_and_aux_on_the_gpu(gpu, tmp_path):
    """bin/mrt on the GPU backend, four ranks sharing the device (-gpus 4: the host assembly): the
    three files equal the Python API's arrays bit for bit."""
    import os
    import subprocess
    from conftest import ROOT
    out, pre = tmp_path / "x.pfm", tmp_path / "p"
    subprocess.run([os.path.join(ROOT, "bin", "mrt"), "-scene", "5", "-width", "32", "-height", "32", "-samples", "16", "-numerics", "exact",
                    "-gpus", "4", "-tilesize", "8", "-denoise", "2", "-o", str(out), "-aux", str(pre)], capture_output=True, text=True,
                   timeout=120, check=True)
    p = gpu.ParseArgv(["mrt", "-scene", "5", "-width", "32", "-height", "32", "-samples", "16"])
    r = gpu.Renderer(ref_scene(gpu, 5), 0)
    d = gpu.render_desc(32, 32, 16, depth=p.max_bounces, max_luminance=p.max_luminance, mode=p.threading_mode, seed=p.seed)
    img, _ = r.render(d)
    nrm, alb = r.render_aux(d)
    r.close()
    assert np.array_equal(bits(gpu.read_pfm(str(out))), bits(gpu.denoise(img, nrm, alb, params(gpu, 2))[..., :3]))
    assert np.array_equal(bits(gpu.read_pfm(str(pre) + "_normal.pfm")), bits(nrm[..., :3]))
    assert np.array_equal(bits(gpu.read_pfm(str(pre) + "_albedo.pfm")), bits(alb[..., :3]))


# ---------------------------------------------------------------- 8 / 9. the Cornell frame, and one graph capture
def test_denoised_16spp_fast_render_and_graph_capture(gpu):
    """Item 5 on the GPU with the render made under numerics="fast": denoised RMSE < raw RMSE against
    the reference at 1024 spp; denoise_device == host mrt_denoise on that frame; and one
    torch.cuda.graph capture of aux + denoise (a row-major pixel list, so the local-pixel order is
    the frame's), replayed twice, gives those bits both times."""
    import torch
    ref, img, nrm, alb = cornell_16spp(gpu, 0, numerics="fast")
    h, w = img.shape[:2]
    want = gpu.denoise(img, nrm, alb)
    raw, den = rmse(img, ref), rmse(want, ref)
    print(f"fast render, RMSE vs the reference at 1024 spp: raw {raw:.5f}, denoised {den:.5f}, ratio {den / raw:.4f}")
    assert den < raw
    assert np.array_equal(bits(device_denoise(gpu, img, nrm, alb, gpu.default_denoise_params())), bits(want))

    r = gpu.Renderer(ref_scene(gpu, 5), 0)
    d = gpu.render_desc(w, h, 16, pixels=np.arange(w * h, dtype=np.uint32))
    r.prepare(d)
    rgb = torch.from_numpy(img).cuda()
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(4)]  # normal, albedo, out, tmp

    def enqueue(stream_ptr):
        r.render_aux_device(d, bufs[0].data_ptr(), bufs[1].data_ptr(), stream_ptr)
        gpu.denoise_device(rgb.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), w, h, bufs[2].data_ptr(), bufs[3].data_ptr(),
                           stream_ptr=stream_ptr)

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    enqueue(side.cuda_stream)  # once outside the capture
    side.synchronize()
    assert np.array_equal(bits(bufs[2].cpu().numpy()), bits(want))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        for b in bufs:
            b.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(bufs[0].cpu().numpy()), bits(nrm)) and np.array_equal(bits(bufs[1].cpu().numpy()), bits(alb))
        assert np.array_equal(bits(bufs[2].cpu().numpy()), bits(want))
    del graph
    r.close()
