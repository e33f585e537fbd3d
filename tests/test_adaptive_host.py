"""Per-pixel sample moments (mrt_moments) and the adaptive render (mrt_render_adaptive) on the host
and the CPU backend: tied to a numpy float32 restatement of include/mrt_adaptive.h, to the render
path (the C restatement's per-path radiance), to a restatement of the passes made of plain
pixel-list renders, and to the purpose -- fewer samples than a uniform render for a smaller error
against the 1024-spp reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_aux_host import bits, ref_scene, rmse

MASK64 = (1 << 64) - 1
LUM = (np.float32(0.212655), np.float32(0.715158), np.float32(0.072187))


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def pass_seed(seed, k):
    return splitmix64((seed + k) & MASK64)


def np_moments(path_rgb, n_pixels, n_samples, out=None):
    """include/mrt_adaptive.h mrt_moments_add in numpy float32, samples in order; identity slots."""
    L = np.asarray(path_rgb, dtype=np.float32).reshape(n_samples, n_pixels, 3)
    m = np.zeros((n_pixels, 4), dtype=np.float32) if out is None else out.copy()
    with np.errstate(all="ignore"):
        for s in range(n_samples):
            fin = np.isfinite(L[s]).all(axis=1)
            l = (L[s, :, 0] * LUM[0] + L[s, :, 1] * LUM[1]) + L[s, :, 2] * LUM[2]
            m[:, 3] = m[:, 3] + np.float32(1)
            m[:, 0] = np.where(fin, m[:, 0] + l, m[:, 0])
            m[:, 1] = np.where(fin, m[:, 1] + l * l, m[:, 1])
            m[:, 2] = np.where(fin, m[:, 2] + np.float32(1), m[:, 2])
    return m


def np_refine(mrt, m, atol, rtol):
    """mrt_moments_refine in numpy float32: !(se <= atol + rtol * mean)."""
    m = np.asarray(m, dtype=np.float32)
    with np.errstate(all="ignore"):
        mean = m[..., 0] / m[..., 2]
        return ~(mrt.moments_se(m) <= np.float32(atol) + np.float32(rtol) * mean)


def wild_radiance(rng, n_pixels, n_samples):
    """Random radiance with NaN, +inf, -inf and 1e30 entries ([s][pixel] float3)."""
    a = (rng.random((n_samples, n_pixels, 3)) * 4).astype(np.float32)
    n = a.size
    flat = a.reshape(-1)
    for val in (np.nan, np.inf, -np.inf, 1e30):
        flat[rng.integers(0, n, size=max(1, n // 40))] = np.float32(val)
    return a


# ---------------------------------------------------------------- 1. the moments against numpy
@pytest.mark.parametrize("n_pixels", [1, 63, 65, 1000])
@pytest.mark.parametrize("n_samples", [1, 15, 17, 33])
def test_moments_equal_the_numpy_restatement(mrt, n_pixels, n_samples):
    rng = np.random.default_rng(n_pixels * 100 + n_samples)
    a = wild_radiance(rng, n_pixels, n_samples)
    want = np_moments(a, n_pixels, n_samples)
    got = mrt.moments(a, n_pixels, n_samples)
    assert np.array_equal(bits(got), bits(want))
    assert (got[:, 3] == n_samples).all() and (got[:, 2] <= got[:, 3]).all()
    if n_pixels * n_samples >= 63:
        assert (got[:, 2] < got[:, 3]).any()  # some samples were not finite
    # a shuffled slot map = identity followed by the permutation
    perm = rng.permutation(n_pixels).astype(np.uint32)
    shuf = mrt.moments(a, n_pixels, n_samples, slots=perm)
    back = np.zeros_like(want)
    back[perm] = want
    assert np.array_equal(bits(shuf), bits(back))
    # two calls on the halves of the samples = one call
    if n_samples > 1:
        h = n_samples // 2
        two = mrt.moments(a[:h], n_pixels, h)
        two = mrt.moments(a[h:], n_pixels, n_samples - h, out=two)
        assert np.array_equal(bits(two), bits(want))


def test_moments_se_and_refine_edge_cases(mrt):
    one = mrt.moments(np.full((1, 3, 3), 0.5, dtype=np.float32), 3, 1)
    assert np.isposinf(mrt.moments_se(one)).all()  # n_finite < 2
    const = mrt.moments(np.full((8, 5, 3), 0.25, dtype=np.float32), 5, 8)
    assert (mrt.moments_se(const) == 0).all() and (const[:, 2] == 8).all()
    a = np.full((4, 4, 3), 0.5, dtype=np.float32)
    a[:, 0, 0] = np.nan        # no finite sample: n_finite 0, se +inf
    a[:3, 1, 1] = np.inf       # one finite sample: se +inf
    a[:, 2, :] = 1e30          # squares overflow: var = inf - inf, se NaN
    a[0, 3, :] = 0.75          # an ordinary pixel
    m = mrt.moments(a, 4, 4)
    se = mrt.moments_se(m)
    assert np.isposinf(se[0]) and np.isposinf(se[1]) and not np.isfinite(se[2]) and np.isfinite(se[3]) and se[3] > 0
    L = mrt.lib()
    lib_se = np.zeros(4, dtype=np.float32)
    ref = np.zeros(4, dtype=np.uint8)
    assert L.mrt_moments_decide(m.ctypes.data, 4, 1e30, 0.0, ref.ctypes.data, lib_se.ctypes.data) == 0
    assert np.array_equal(bits(lib_se), bits(se))
    assert list(ref) == [1, 1, 1, 0]  # a NaN or infinite se refines whatever the tolerance
    assert list(mrt.moments_refine(m, 0.0, 0.0)) == [True, True, True, True]
    assert list(mrt.moments_refine(const, 0.0, 0.0)) == [False] * 5  # se 0 <= 0
    assert np.array_equal(mrt.moments_refine(m, 0.01, 0.5), np_refine(mrt, m, 0.01, 0.5))


# ---------------------------------------------------------------- 2. tie to the render path
@pytest.mark.parametrize("sid", [5, 2])
def test_zero_passes_is_the_render_plus_moments_of_its_paths(mrt, orc, sid):
    """max_passes = 0: the image of Renderer.render bit for bit, and the moments of the C
    restatement's per-path radiance (scene 5: a light, no sky; scene 2: the sky, no light)."""
    w = h = 32
    sc = ref_scene(mrt, sid)
    r = mrt.Renderer(sc, "cpu")
    d = mrt.render_desc(w, h, 16)
    img, rays = r.render(d)
    aimg, mom, arays = r.render_adaptive(d, mrt.default_adaptive_params(0))
    r.close()
    assert np.array_equal(bits(aimg), bits(img)) and arays == rays
    _, orays, prgb, _ = orc.render(sc, orc.desc(w, h, 16, threads=4), paths=True)
    assert orays == rays
    sm = np.ascontiguousarray(prgb.reshape(w * h, 16, 3).transpose(1, 0, 2))  # [s][pixel]
    want = mrt.moments(sm, w * h, 16)
    assert np.array_equal(bits(mom.reshape(-1, 4)), bits(want))
    assert (mom[..., 3] == 16).all()
    assert np.array_equal(bits(want), bits(np_moments(sm, w * h, 16)))


# ---------------------------------------------------------------- 3. refinement
W3, H3, BASE3 = 40, 24, 4


def refine_case(mrt):
    """(renderer, desc, plain image, pass-0 moments, atol = their median se)."""
    r = mrt.Renderer(ref_scene(mrt, 5, W3 / H3), "cpu")
    d = mrt.render_desc(W3, H3, BASE3)
    img0, m0, _ = r.render_adaptive(d, mrt.default_adaptive_params(0))
    atol = float(np.median(mrt.moments_se(m0)))
    assert np.isfinite(atol) and atol > 0
    return r, d, img0, m0, atol


def restate_passes(mrt, orc, sc, r, d, atol, rtol, passes=2):
    """The passes from plain pixel-list renders, the merge formula in float32, and mrt_moments of the
    C restatement's per-path radiance; (image, moments) in pixel order."""
    w, h, sq = d.width, d.height, d.sqrt_samples
    px0 = mrt.local_pixels(d)
    img, rays = r.render(d)
    C_ = img.reshape(-1, 4).copy()
    _, _, prgb, _ = orc.render(sc, orc.desc(w, h, sq * sq, depth=d.max_bounces, seed=d.seed, threads=4), paths=True)
    m = np.zeros((w * h, 4), dtype=np.float32)
    m = mrt.moments(np.ascontiguousarray(prgb.reshape(w * h, sq * sq, 3).transpose(1, 0, 2)), w * h, sq * sq, out=m)
    N = np.float32(sq * sq)
    counts = []
    for k in range(1, passes + 1):
        ref = np_refine(mrt, m[px0], atol, rtol)  # in local order
        lst = px0[ref]
        counts.append(len(lst))
        if len(lst) == 0:
            break
        ns = (sq << k) ** 2
        seed = pass_seed(d.seed, k)
        c, kr = r.render(mrt.render_desc(w, h, ns, depth=d.max_bounces, max_luminance=d.max_luminance, seed=seed, tile_size=d.tile_size,
                                         pixels=lst))
        rays += kr
        c = c.reshape(-1, 4)
        nsf = np.float32(ns)
        wgt = nsf / (N + nsf)
        for ch in range(3):
            C_[lst, ch] = C_[lst, ch] + (c[lst, ch] - C_[lst, ch]) * wgt
        N = N + nsf
        _, _, prgb, _ = orc.render(sc, orc.desc(w, h, ns, depth=d.max_bounces, seed=seed, threads=4), paths=True)
        sm = np.ascontiguousarray(prgb.reshape(w * h, ns, 3)[lst].transpose(1, 0, 2))
        m = mrt.moments(sm, len(lst), ns, slots=lst, out=m)
    return C_.reshape(h, w, 4), m.reshape(h, w, 4), rays, counts


def test_refined_pixels_equal_a_restatement_and_the_rest_the_plain_render(mrt, orc):
    r, d, img0, m0, atol = refine_case(mrt)
    plain, _ = r.render(d)
    img, mom, rays = r.render_adaptive(d, mrt.default_adaptive_params(2, atol, 0.0))
    spent = mom[..., 3]
    assert set(np.unique(spent)) == {4.0, 20.0, 84.0}
    un = spent == 4
    assert un.any() and (~un).any()
    assert np.array_equal(bits(img[un]), bits(plain[un])) and np.array_equal(bits(mom[un]), bits(m0[un]))
    assert not np.array_equal(bits(img[~un]), bits(plain[~un]))
    wimg, wmom, wrays, counts = restate_passes(mrt, orc, ref_scene(mrt, 5, W3 / H3), r, d, atol, 0.0)
    r.close()
    assert counts == [int((spent > 4).sum()), int((spent > 20).sum())]
    assert np.array_equal(bits(img), bits(wimg))
    assert np.array_equal(bits(mom), bits(wmom))
    assert rays == wrays
    # the refined set is the library's own decision on the pass-0 moments
    assert np.array_equal(~un, mrt.moments_refine(m0, atol, 0.0))


def test_zero_tolerance_refines_every_pixel_with_variance(mrt):
    r, d, img0, m0, _ = refine_case(mrt)
    img, mom, _ = r.render_adaptive(d, mrt.default_adaptive_params(2, 0.0, 0.0))
    r.close()
    se0 = mrt.moments_se(m0)
    noisy = ~(se0 <= 0)  # non-zero variance (or no finite pair of samples)
    assert noisy.any()
    assert (mom[..., 3][noisy] == 84).all() and (mom[..., 3][~noisy] == 4).all()
    assert np.array_equal(bits(img[~noisy]), bits(img0[~noisy]))


def test_ranks_pixel_lists_and_chunks_equal_the_whole_image(mrt):
    r, d, img0, m0, atol = refine_case(mrt)
    p = mrt.default_adaptive_params(2, atol, 0.0)
    img, mom, rays = r.render_adaptive(d, p)
    # the union of three ranks
    uimg, umom, urays = np.zeros_like(img), np.zeros_like(mom), 0
    owned = np.zeros(W3 * H3, dtype=int)
    for rank in range(3):
        dr = mrt.render_desc(W3, H3, BASE3, tile_size=8, rank=rank, world=3)
        ri, rm, rr = r.render_adaptive(dr, p)
        px = mrt.local_pixels(dr)
        owned[px] += 1
        uimg.reshape(-1, 4)[px] = ri.reshape(-1, 4)[px]
        umom.reshape(-1, 4)[px] = rm.reshape(-1, 4)[px]
        urays += rr
        rest = np.setdiff1d(np.arange(W3 * H3), px)
        assert not ri.reshape(-1, 4)[rest].any() and not rm.reshape(-1, 4)[rest].any()  # owned pixels only
    assert (owned == 1).all()
    assert np.array_equal(bits(uimg), bits(img)) and np.array_equal(bits(umom), bits(mom)) and urays == rays
    # a shuffled pixel list
    lst = np.random.default_rng(3).permutation(W3 * H3)[: W3 * H3 // 2].astype(np.uint32)
    li, lm, _ = r.render_adaptive(mrt.render_desc(W3, H3, BASE3, pixels=lst), p)
    assert np.array_equal(bits(li.reshape(-1, 4)[lst]), bits(img.reshape(-1, 4)[lst]))
    assert np.array_equal(bits(lm.reshape(-1, 4)[lst]), bits(mom.reshape(-1, 4)[lst]))
    assert (lm.reshape(-1, 4)[lst][:, 3] > 4).any()
    # several launches per pass (the CPU backend ignores chunk_samples; the GPU test asserts the same)
    ci, cm, cr = r.render_adaptive(mrt.render_desc(W3, H3, BASE3, chunk_samples=3), p)
    r.close()
    assert np.array_equal(bits(ci), bits(img)) and np.array_equal(bits(cm), bits(mom)) and cr == rays


# ---------------------------------------------------------------- 4. purpose
def purpose_figures(mrt, device, numerics="exact"):
    """The Cornell box at 128 x 128, 16-spp base, 2 passes, atol 0.03, rtol 0, against the reference
    as shipped at 1024 spp and uniform renders at 49 and 64 spp; prints and returns the figures."""
    g = np.load(os.path.join(GOLDEN, "shipped_stream_5_small.npz"))
    _, w, h, _, depth = (int(x) for x in g["meta"])
    ref = g["image"].astype(np.float64)
    r = mrt.Renderer(ref_scene(mrt, 5), device)
    img, mom, rays = r.render_adaptive(mrt.render_desc(w, h, 16, depth=depth, numerics=numerics), mrt.default_adaptive_params(2, 0.03, 0.0))
    u49, rays49 = r.render(mrt.render_desc(w, h, 49, depth=depth, numerics=numerics))
    u64, rays64 = r.render(mrt.render_desc(w, h, 64, depth=depth, numerics=numerics))
    r.close()
    spent = mom[..., 3]
    out = dict(n=w * h, spp=float(spent.mean()), rmse=rmse(img, ref), rmse49=rmse(u49, ref), rmse64=rmse(u64, ref),
               refined=[int((spent > 16).sum()), int((spent > 80).sum())], rays=rays, rays49=rays49, rays64=rays64)
    print(f"adaptive 16-spp base, 2 passes, atol 0.03 ({device}, {numerics}): {out['spp']:.1f} spp mean, RMSE {out['rmse']:.4f}, refined "
          f"{out['refined']} of {out['n']}, {rays} rays; uniform 49 spp: RMSE {out['rmse49']:.4f}, {rays49} rays; uniform 64 spp: RMSE "
          f"{out['rmse64']:.4f}, {rays64} rays")
    return out


def assert_purpose(f):
    assert f["spp"] <= 49
    assert f["rmse"] < f["rmse49"]
    for n in f["refined"]:
        assert 0 < n < f["n"]
    assert f["refined"][1] < f["refined"][0]


def test_adaptive_beats_uniform_49spp_with_fewer_samples(mrt):
    assert_purpose(purpose_figures(mrt, "cpu"))


# ---------------------------------------------------------------- 5. API surface
def test_api_rejects_bad_arguments(mrt):
    L = mrt.lib()
    r = mrt.Renderer(ref_scene(mrt, 5), "cpu")
    ok = mrt.render_desc(8, 8, 1)
    p = mrt.default_adaptive_params()
    assert (p.max_passes, p.rtol) == (2, 0.0) and abs(p.atol - 0.03) < 1e-7
    with pytest.raises(mrt.MrtError, match="invalid"):
        r.render_adaptive(mrt.render_desc(8, 8, 1, mode=1))
    for flags in (0x1, 0x4, 0x8, 0x10, 0x40, 0x80, 0x2 | 0x1):
        with pytest.raises(mrt.MrtError, match="invalid"):
            r.render_adaptive(mrt.render_desc(8, 8, 1, flags=flags))
    for bad in (dict(max_passes=5), dict(atol=-0.1), dict(rtol=-0.1), dict(atol=float("nan")), dict(rtol=float("nan")),
                dict(atol=float("inf")), dict(rtol=float("inf"))):
        with pytest.raises(mrt.MrtError, match="invalid"):
            r.render_adaptive(ok, mrt.default_adaptive_params(**bad))
    for wh in ((0, 8), (8, 0)):
        with pytest.raises(mrt.MrtError, match="invalid"):
            r.render_adaptive(mrt.render_desc(wh[0], wh[1], 1))
    buf = np.zeros((8, 8, 4), dtype=np.float32)
    rays = C.c_uint64()
    b = buf.ctypes.data
    for args in ((None, C.byref(ok), C.byref(p), b, b, C.byref(rays), None), (r._h, None, C.byref(p), b, b, C.byref(rays), None),
                 (r._h, C.byref(ok), None, b, b, C.byref(rays), None), (r._h, C.byref(ok), C.byref(p), None, b, C.byref(rays), None)):
        assert L.mrt_render_adaptive(*args) == 1
    # moments_out and rays_out may be NULL
    assert L.mrt_render_adaptive(r._h, C.byref(ok), C.byref(p), b, None, None, None) == 0
    img, _, _ = r.render_adaptive(ok)
    assert np.array_equal(bits(buf), bits(img))
    r.close()
    rad = np.zeros((2, 4, 3), dtype=np.float32)
    m = np.zeros((4, 4), dtype=np.float32)
    for args in ((None, 4, 2, None, m.ctypes.data), (rad.ctypes.data, 4, 2, None, None), (rad.ctypes.data, 0, 2, None, m.ctypes.data),
                 (rad.ctypes.data, 4, 0, None, m.ctypes.data)):
        assert L.mrt_moments(*args) == 1
    for args in ((None, 4, 2, None, m.ctypes.data, None), (rad.ctypes.data, 4, 2, None, None, None), (rad.ctypes.data, 0, 2, None, m.ctypes.data, None),
                 (rad.ctypes.data, 4, 0, None, m.ctypes.data, None)):
        assert L.mrt_moments_device(*args) == 1
    assert L.mrt_moments_decide(None, 4, 0.0, 0.0, m.ctypes.data, None) == 1
    assert L.mrt_moments_decide(m.ctypes.data, 4, 0.0, 0.0, None, None) == 1
    assert set(["mrt_moments", "mrt_moments_device", "mrt_default_adaptive_params", "mrt_render_adaptive"]) <= set(mrt._lib.EXPORTS)
    assert L.mrt_abi_version() == 6


CLI = ["-backend", "cpu", "-order", "path", "-scene", "5", "-width", "40", "-height", "24", "-samples", "4"]


@pytest.mark.parametrize("gpus", [1, 4])
def test_cli_adaptive_equals_the_python_api(mrt, tmp_path, gpus):
    """bin/mrt -adaptive 2 -atol X -samplemap: the image, the sample map and the printed line, on the
    CPU backend as one rank and as four (each refining its own pixels of the shared host buffers)."""
    out, smap = tmp_path / "x.pfm", tmp_path / "n.pfm"
    res = subprocess.run([os.path.join(ROOT, "bin", "mrt")] + CLI + ["-gpus", str(gpus), "-tilesize", "8", "-adaptive", "2", "-atol", "0.05",
                         "-rtol", "0.01", "-o", str(out), "-samplemap", str(smap)], capture_output=True, text=True, timeout=120, check=True)
    p = mrt.ParseArgv(["mrt"] + CLI)
    r = mrt.Renderer(ref_scene(mrt, 5, 40 / 24), "cpu")
    d = mrt.render_desc(40, 24, 4, depth=p.max_bounces, max_luminance=p.max_luminance, mode=0, seed=p.seed, tile_size=8)  # (-adaptive renders in mode 0)
    img, mom, rays = r.render_adaptive(d, mrt.default_adaptive_params(2, 0.05, 0.01))
    r.close()
    assert np.array_equal(bits(mrt.read_pfm(str(out))), bits(img[..., :3]))
    spent = mom[..., 3]
    assert np.array_equal(bits(mrt.read_pfm(str(smap))), bits(np.repeat(spent[..., None], 3, axis=2)))
    lines = res.stdout.splitlines()
    k = [i for i, ln in enumerate(lines) if "Trace:" in ln]
    assert len(k) == 1
    m = re.fullmatch(r"adaptive: ([0-9.]+) spp mean, atol 0.05 rtol 0.01, refined (\d+) (\d+) of 960 pixels", lines[k[0] + 1])
    assert m, lines
    assert m.group(1) == f"{float(spent.astype(np.float64).sum()) / 960:.2f}"
    assert [int(m.group(2)), int(m.group(3))] == [int((spent > 4).sum()), int((spent > 20).sum())]
    assert 0 < int(m.group(3)) < int(m.group(2)) < 960
    assert f"rays {rays}" in lines


def test_cli_refuses_adaptive_with_the_rccl_gather(mrt):
    res = subprocess.run([os.path.join(ROOT, "bin", "mrt")] + CLI + ["-adaptive", "2", "-gather", "rccl"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 1 and "-adaptive" in res.stderr and "RCCL" in res.stderr
    res = subprocess.run([os.path.join(ROOT, "bin", "mrt")] + CLI + ["-adaptive", "5"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "1 to 4" in res.stderr
    res = subprocess.run([os.path.join(ROOT, "bin", "mrt")] + CLI + ["-adaptive", "2", "-mode", "1"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "-mode 0" in res.stderr
