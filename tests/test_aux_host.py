"""First-hit feature buffers (mrt_render_aux) on the CPU backend and the a-trous filter on the host
(mrt_denoise): tied to the render path, to analytic geometry, to a float64 restatement of the
filter's formulas (include/mrt_denoise.h), and to the purpose -- a 16-spp Cornell box closer to the
1024-spp reference after the filter than before."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import synth_scenes as ss
from conftest import GOLDEN, ROOT
from synth_scenes import Synth

_scenes = {}


def ref_scene(mrt, sid, aspect=1.0):
    if (sid, aspect) not in _scenes:
        _scenes[(sid, aspect)] = mrt.select_scene(sid, aspect)
    return _scenes[(sid, aspect)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def seq_mean(x):
    """float32 sum over axis 1 in order, divided by float32(n): the fold of the buffers."""
    acc = np.zeros((x.shape[0],) + x.shape[2:], dtype=np.float32)
    for s in range(x.shape[1]):
        acc = acc + x[:, s]
    return acc / np.float32(x.shape[1])


# ---------------------------------------------------------------- 1. tie to the render path
# scene 5: a front-facing light's albedo is its emitted radiance (15), every other hit's is at most 1
# (material colours, 1 for glass) and a miss's is 0 (no sky); scene 2: no light, a miss is the sky
@pytest.mark.parametrize("sid", [5, 2])
def test_depth0_render_equals_albedo_on_light_and_miss_pixels(mrt, sid):
    """max_bounces=0, one sample: the render is the first hit's emitted term or the miss radiance,
    and 0 on every scattering surface.  Bit for bit: the render's fold of one sample is (0 + L) / 1,
    the buffer's is the same sum and quotient."""
    w = h = 32
    r = mrt.Renderer(ref_scene(mrt, sid), "cpu")
    d = mrt.render_desc(w, h, 1, depth=0, max_luminance=1000.0)
    img, _ = r.render(d)
    nrm, alb = r.render_aux(d)
    r.close()
    miss = nrm[..., 3] == 0
    light = (alb[..., :3].max(axis=2) > 1.0) & ~miss
    assert miss.any() and (~miss & ~light).any()
    if sid == 5:
        assert light.any()
    else:
        assert not light.any() and (alb[miss][:, :3] >= 0.5).all()  # the sky
    want = np.where((miss | light)[..., None], alb[..., :3], np.float32(0))
    assert np.array_equal(bits(img[..., :3]), bits(want))
    assert set(np.unique(nrm[..., 3])) <= {0.0, 1.0}
    assert (alb[..., 3][miss] == 0).all() and (nrm[miss] == 0).all() and (alb[..., 3][~miss] > 0).all()


def black_cornell(mrt):
    """Scene 5 with black walls and box and without its glass sphere (node 16 of its root list):
    every first hit contributes its emitted term or 0, so EVERY pixel's albedo is the mean of its
    depth-0 radiances -- also the pixels the light covers in part."""
    s = Synth(ref_scene(mrt, 5))
    for m in (0, 1, 2):  # red, white, green
        s.textures[int(s.materials[m]["tex"])]["f"][:3] = 0
    s.set_list(s.root, [i for i in s.list_items(s.root) if i != 16])
    assert (s.nodes[16]["kind"] & 0xFF) == ss.K_SPHERE
    return s


@pytest.mark.parametrize("which", ["5", "2", "5-black"])
def test_depth0_paths_fold_to_albedo(mrt, orc, which):
    """16 samples: the depth-0 per-path radiance (the C restatement's per-path output -- the CPU
    backend takes no MRT_RF_PATH_DEBUG; tests/test_aux_gpu.py reads Renderer.paths), summed in
    float32 in sample order and divided by 16, equals the albedo buffer bit for bit on the pixels
    whose 16 first hits are all front-facing light or all misses.  At 32 x 32 scene 5 has no such
    pixel (the light covers at most 12 of a pixel's 16 samples, the room's opening none entirely), so
    its blackened copy carries the case: there the equality holds on every pixel."""
    w = h = 32
    sc = black_cornell(mrt) if which == "5-black" else ref_scene(mrt, int(which))
    r = mrt.Renderer(sc, "cpu")
    nrm, alb = r.render_aux(mrt.render_desc(w, h, 16, depth=0))
    r.close()
    _, _, prgb, _ = orc.render(sc, orc.desc(w, h, 16, depth=0, threads=4), paths=True)
    prgb = prgb.reshape(w * h, 16, 3)
    allmiss = (nrm[..., 3] == 0).ravel()
    alllight = (prgb.max(axis=2) > 1.0).all(axis=1) & (nrm[..., 3] == 1).ravel()
    mask = np.ones(w * h, dtype=bool) if which == "5-black" else allmiss | alllight
    if which == "2":
        assert allmiss.any()
    if which == "5-black":
        lit = (prgb.max(axis=2) > 1.0).sum(axis=1)
        assert ((lit > 0) & (lit < 16)).any() and (alb[..., :3].max() > 1.0)  # pixels the light covers in part
    assert np.array_equal(bits(seq_mean(prgb)[mask]), bits(alb.reshape(-1, 4)[mask][:, :3]))


# ---------------------------------------------------------------- 2. analytic geometry
def down_camera(s):
    """A pinhole at (0, 10, 0) looking down -y: ray(u, v) = llcorner + u horz + v vert - origin."""
    cam = s.camera
    for name, val in (("origin", (0, 10, 0)), ("llcorner", (-1, 9, -1)), ("horz", (2, 0, 0)), ("vert", (0, 0, 2)),
                      ("u", (1, 0, 0)), ("v", (0, 0, 1)), ("w", (0, 1, 0))):
        a = getattr(cam, name)
        for i in range(3):
            a[i] = float(val[i])
        a[3] = 0.0
    cam.lens_radius, cam.time0, cam.time1 = 0.0, 0.0, 0.0
    s._view = None


def centre_rays(s, w, h):
    """float64 (origin, unit directions (h, w, 3)) of the pixel-centre rays, from the view's camera."""
    cam = s.camera
    o, ll, hz, vt = (np.array([getattr(cam, n)[i] for i in range(3)], dtype=np.float64) for n in ("origin", "llcorner", "horz", "vert"))
    u = (np.arange(w, dtype=np.float64) + 0.5) / w
    v = (np.arange(h, dtype=np.float64) + 0.5) / h
    d = ll + u[None, :, None] * hz + v[:, None, None] * vt - o
    return o, d / np.linalg.norm(d, axis=2, keepdims=True)


def synth_base(mrt):
    s = Synth(ref_scene(mrt, 5)).clear()
    s.sky = 0
    down_camera(s)
    return s


def test_floor_rect_normal_coverage_depth(mrt):
    w = h = 48
    s = synth_base(mrt)
    s.root = s.list([s.rect(ss.K_XZ, -100, 100, -100, 100, 0.25, s.lambertian(0.2, 0.5, 0.7), 1.0)])
    r = mrt.Renderer(s, "cpu")
    nrm, alb = r.render_aux(mrt.render_desc(w, h, 1))
    r.close()
    o, d = centre_rays(s, w, h)
    assert np.array_equal(nrm, np.broadcast_to(np.array([0, 1, 0, 1], dtype=np.float32), nrm.shape))  # exactly (0, +1, 0), coverage 1
    assert np.array_equal(alb[..., :3], np.broadcast_to(np.array([0.2, 0.5, 0.7], dtype=np.float32), (h, w, 3)))
    depth = (0.25 - o[1]) / d[..., 1]
    assert np.abs(alb[..., 3] / depth - 1).max() < 1e-4


def test_sphere_normal_and_depth(mrt):
    """Against the float64 solution at each pixel's centre ray: 1e-4 absolute on the normal, 1e-4
    relative on the depth (float32 epsilon 6e-8 x at most 1/cos^2 = 25 x a few dozen operations);
    grazing pixels (|cos| < 0.2) and pixels within one pixel of the silhouette are left out, and they
    are at most 20 % of the sphere's pixels."""
    w = h = 48
    c, rad = np.array([0.3, 5.0, -0.2]), 3.2
    s = synth_base(mrt)
    s.root = s.list([s.sphere(tuple(c), rad, s.lambertian(0.6, 0.3, 0.2))])
    r = mrt.Renderer(s, "cpu")
    nrm, alb = r.render_aux(mrt.render_desc(w, h, 1))
    r.close()
    o, d = centre_rays(s, w, h)
    oc = o - c
    b = d @ oc
    disc = b * b - (oc @ oc - rad * rad)
    hit = disc > 0
    t = -b - np.sqrt(np.where(hit, disc, 0))
    n = (o + t[..., None] * d - c) / rad
    cos = (n * d).sum(axis=2)
    pad = np.pad(hit, 1, mode="edge")
    neigh = np.stack([pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    edge = neigh.any(axis=0) != neigh.all(axis=0)
    keep = hit & ~edge & (np.abs(cos) >= 0.2)
    out = ~hit & ~edge
    excluded = (hit & ~keep).sum() / hit.sum()
    print(f"sphere: {hit.sum()} hit pixels, {excluded:.1%} excluded")
    assert hit.sum() > 800 and excluded <= 0.20
    assert (nrm[..., 3][keep] == 1).all() and (nrm[out] == 0).all() and (alb[out] == 0).all()
    assert np.abs(nrm[..., :3][keep] - n[keep]).max() < 1e-4
    assert np.abs(alb[..., 3][keep] / t[keep] - 1).max() < 1e-4
    assert ((nrm[..., :3][keep] * d[keep]).sum(axis=1) < 0).all()  # facing the ray


# ---------------------------------------------------------------- 3. schedule independence
@pytest.mark.parametrize("sid", [5, 6, 7, 8])
def test_ranks_and_pixel_lists_equal_whole_image(mrt, sid):
    w, h, spp, ts = 40, 24, 4, 16
    r = mrt.Renderer(ref_scene(mrt, sid, w / h), "cpu")
    whole = r.render_aux(mrt.render_desc(w, h, spp, tile_size=ts))
    assert (whole[0][..., 3] > 0).any()
    union = [np.zeros_like(whole[0]), np.zeros_like(whole[1])]
    seen = np.zeros(w * h, dtype=np.int32)
    for rank in range(3):
        d = mrt.render_desc(w, h, spp, tile_size=ts, rank=rank, world=3)
        px = mrt.local_pixels(d)
        seen[px] += 1
        part = r.render_aux(d)
        for k in range(2):
            own = np.zeros(w * h, dtype=bool)
            own[px] = True
            assert not part[k].reshape(-1, 4)[~own].any()  # only owned pixels are written
            union[k] += part[k]
    assert (seen == 1).all()
    for k in range(2):
        assert np.array_equal(bits(union[k]), bits(whole[k]))
    px = np.random.default_rng(sid).permutation(w * h)[:300].astype(np.uint32)
    part = r.render_aux(mrt.render_desc(w, h, spp, tile_size=ts, pixels=px))
    r.close()
    for k in range(2):
        want = np.zeros((w * h, 4), dtype=np.float32)
        want[px] = whole[k].reshape(-1, 4)[px]
        assert np.array_equal(bits(part[k].reshape(-1, 4)), bits(want))


# ---------------------------------------------------------------- 4. the filter
def params(mrt, iterations=None, **kw):
    p = mrt.default_denoise_params()
    if iterations is not None:
        p.iterations = iterations
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def random_guides(rng, h, w):
    nrm = rng.normal(size=(h, w, 4)).astype(np.float32)
    nrm[rng.random((h, w)) < 0.2] = 0  # misses: zero normals
    alb = rng.random((h, w, 4)).astype(np.float32)
    alb[..., 3] = rng.uniform(1, 50, size=(h, w)).astype(np.float32)
    alb[..., 3][nrm[..., 3] == 0] = 0
    return nrm, alb


def filter_f64(img, nrm, alb, p):
    """The formulas of include/mrt_denoise.h in float64 (small frames only)."""
    h, w = img.shape[:2]
    k = [0.375, 0.25, 0.0625]
    cur = img.astype(np.float64)
    nrm, alb = nrm.astype(np.float64), alb.astype(np.float64)
    ln = np.linalg.norm(nrm[..., :3], axis=2)
    nh = nrm[..., :3] / np.where(ln > 0, ln, 1)[..., None]
    for i in range(p.iterations):
        step, sc = 1 << i, p.sigma_color * 0.5 ** i
        out = cur.copy()
        for y in range(h):
            for x in range(w):
                sw, acc = 0.0, np.zeros(3)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qy, qx = y + dy * step, x + dx * step
                        if not (0 <= qy < h and 0 <= qx < w):
                            continue
                        wt = k[abs(dx)] * k[abs(dy)]
                        if (dy, dx) != (0, 0):
                            if ln[y, x] == 0 or ln[qy, qx] == 0:
                                wn = 1.0 if ln[y, x] == 0 and ln[qy, qx] == 0 else 0.0
                            else:
                                wn = max(0.0, nh[y, x] @ nh[qy, qx]) ** p.sigma_normal
                            zp, zq = alb[y, x, 3], alb[qy, qx, 3]
                            ez = abs(zp - zq) / (max(zp, zq) * p.sigma_depth) if zp != zq else 0.0
                            ea = ((alb[y, x, :3] - alb[qy, qx, :3]) ** 2).sum() / p.sigma_albedo ** 2
                            ec = ((cur[y, x, :3] - cur[qy, qx, :3]) ** 2).sum() / sc ** 2
                            wt = wt * wn * np.exp(-(ez + ea + ec))
                        sw += wt
                        acc += wt * cur[qy, qx, :3]
                out[y, x, :3] = acc / sw
        cur = out
    return cur


# per pass at most 25 products, 25 adds and one divide: ~52 half-ulps, 3e-6 relative; 5 passes
BOUND = 2e-5


@pytest.mark.parametrize("w,h", [(37, 23), (1, 1), (5, 3)])
def test_constant_colour_survives_any_guides(mrt, w, h):
    rng = np.random.default_rng(w * 100 + h)
    nrm, alb = random_guides(rng, h, w)
    c = np.array([0.7, 2.5, 0.01, 0.0], dtype=np.float32)
    img = np.broadcast_to(c, (h, w, 4)).copy()
    out = mrt.denoise(img, nrm, alb, params(mrt, 5))
    assert np.abs(out - img).max() <= BOUND * float(np.linalg.norm(c))
    assert np.array_equal(out[..., 3], img[..., 3])


def test_nothing_crosses_a_zero_normal_weight(mrt):
    w, h = 32, 20
    nrm = np.zeros((h, w, 4), dtype=np.float32)
    nrm[:, :w // 2, 0] = 1
    nrm[:, w // 2:, 2] = 1
    nrm[..., 3] = 1
    alb = np.broadcast_to(np.array([0.5, 0.5, 0.5, 7.0], dtype=np.float32), (h, w, 4)).copy()
    left, right = np.array([1.0, 0.25, 3.0, 0.0], dtype=np.float32), np.array([0.1, 4.0, 0.5, 0.0], dtype=np.float32)
    img = np.zeros((h, w, 4), dtype=np.float32)
    img[:, :w // 2], img[:, w // 2:] = left, right
    out = mrt.denoise(img, nrm, alb, params(mrt, 5, sigma_color=1e3))
    assert np.abs(out[:, :w // 2] - left).max() <= BOUND * float(np.linalg.norm(left))
    assert np.abs(out[:, w // 2:] - right).max() <= BOUND * float(np.linalg.norm(right))


def test_zero_iterations_copy(mrt):
    rng = np.random.default_rng(0)
    nrm, alb = random_guides(rng, 9, 11)
    img = rng.random((9, 11, 4)).astype(np.float32)
    assert np.array_equal(bits(mrt.denoise(img, nrm, alb, params(mrt, 0))), bits(img))


@pytest.mark.parametrize("w,h,it", [(1, 1, 3), (5, 3, 3), (9, 7, 2)])
def test_filter_equals_its_formulas_in_float64(mrt, w, h, it):
    """Border taps and every weight: random frames against the float64 restatement.  Bound: the
    float32 weights carry ~1e-6 relative error each (exponents up to ~10 here, times 6e-8, plus the
    pow), the colours are in [0, 1): 2e-5 absolute."""
    rng = np.random.default_rng(w + h)
    nrm, alb = random_guides(rng, h, w)
    nrm[..., :3] += np.float32(2.0) * (nrm[..., :3] != 0)  # mostly agreeing normals: weights that matter
    img = rng.random((h, w, 4)).astype(np.float32)
    p = params(mrt, it, sigma_color=1.0, sigma_normal=4.0, sigma_albedo=0.8, sigma_depth=1.5)
    out = mrt.denoise(img, nrm, alb, p)
    want = filter_f64(img, nrm, alb, p)
    assert np.abs(out[..., :3] - want[..., :3]).max() < BOUND
    assert np.abs(out[..., :3] - img[..., :3]).max() > 1e-3 or w == 1  # it did filter


EDGE_SIGMA_NORMALS = [0.25, 5.0, 128.0]  # 5: mrt_powf's pow5 shortcut; 128: the library default's order


def edge_weight_frames(sigma_normal, w=37, h=23):
    """(img, nrm, alb, params) whose weights sit at the edges of mrt_expf / mrt_powf: colours and albedos are
    constant per 6 x 6 block plus 1 % noise, so the summed exponent e_z + e_a + e_c of a tap is ~0 inside a
    block and up to ~110 across blocks (sigma_color 0.19, sigma_albedo 0.155, colours in [0, 1)): weights that
    are ordinary, float-subnormal (exponent 87.3 ... 104) and exactly zero (past 104) in one frame, twice --
    the second pass quarters sigma_color^2."""
    rng = np.random.default_rng(7)  # one frame for every sigma_normal
    nrm, alb = random_guides(rng, h, w)
    nrm[..., :3] += np.float32(2.0) * (nrm[..., :3] != 0)
    by, bx = np.arange(h)[:, None] // 6, np.arange(w)[None, :] // 6
    blocks = lambda: rng.random((h // 6 + 1, w // 6 + 1, 3))[by, bx]
    img = np.zeros((h, w, 4), dtype=np.float32)
    img[..., :3] = (0.99 * blocks() + 0.01 * rng.random((h, w, 3))).astype(np.float32)
    img[..., 3] = rng.random((h, w)).astype(np.float32)
    alb[..., :3] = (0.99 * blocks() + 0.01 * rng.random((h, w, 3))).astype(np.float32)
    return img, nrm, alb, (2, dict(sigma_color=0.19, sigma_normal=sigma_normal, sigma_albedo=0.155, sigma_depth=1.5))


def first_pass_exponents(img, alb, sc, sa, sz):
    """e_z + e_a + e_c of the right-hand and the upper neighbour taps of pass 0, in float64."""
    out = []
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1], np.s_[1:])):
        c, q = img.astype(np.float64), alb.astype(np.float64)
        zp, zq = q[a][..., 3], q[b][..., 3]
        ez = np.where(zp != zq, np.abs(zp - zq) / np.where(zp != zq, np.maximum(zp, zq) * sz, 1), 0)
        out.append((ez + ((q[a][..., :3] - q[b][..., :3]) ** 2).sum(-1) / sa ** 2 + ((c[a][..., :3] - c[b][..., :3]) ** 2).sum(-1) / sc ** 2).ravel())
    return np.concatenate(out)


@pytest.mark.parametrize("sn", EDGE_SIGMA_NORMALS)
def test_filter_with_weights_at_the_edges_of_exp_and_pow(mrt, sn):
    """The float64 restatement's bound on frames with float-subnormal and exactly-zero weights.  No pixel is
    left out: the centre tap's weight is exactly 9/64, so sum w is never below it, let alone subnormal, and
    the bound's reasoning (relative error of the weights that matter, colours in [0, 1)) holds everywhere."""
    img, nrm, alb, (it, kw) = edge_weight_frames(sn)
    e = first_pass_exponents(img, alb, kw["sigma_color"], kw["sigma_albedo"], kw["sigma_depth"])
    assert e.min() < 0.5 and ((e > 87.4) & (e < 103.9)).any() and (e > 104.0).any() and 100 < e.max() < 125, (e.min(), e.max())
    p = params(mrt, it, **kw)
    out = mrt.denoise(img, nrm, alb, p)
    want = filter_f64(img, nrm, alb, p)
    err = np.abs(out[..., :3] - want[..., :3]).max()
    print(f"sigma_normal {sn}: exponents {e.min():.3f} .. {e.max():.1f}, max |host - float64| {err:.3e}")
    assert err < BOUND
    assert np.abs(out[..., :3] - img[..., :3]).max() > 1e-3  # it did filter


# ---------------------------------------------------------------- 5. purpose
def cornell_16spp(mrt, device, numerics="exact"):
    g = np.load(os.path.join(GOLDEN, "shipped_stream_5_small.npz"))
    _, w, h, _, depth = (int(x) for x in g["meta"])
    r = mrt.Renderer(ref_scene(mrt, 5), device)
    img, _ = r.render(mrt.render_desc(w, h, 16, depth=depth, numerics=numerics))
    nrm, alb = r.render_aux(mrt.render_desc(w, h, 16))
    r.close()
    return g["image"].astype(np.float64), img, nrm, alb


def rmse(img, ref):
    return float(np.sqrt(((img[..., :3].astype(np.float64) - ref) ** 2).mean()))


def test_denoised_16spp_is_closer_to_the_1024spp_reference(mrt):
    ref, img, nrm, alb = cornell_16spp(mrt, "cpu")
    assert ref.shape == (128, 128, 3)
    raw, den = rmse(img, ref), rmse(mrt.denoise(img, nrm, alb), ref)
    print(f"RMSE vs the reference at 1024 spp: raw {raw:.5f}, denoised {den:.5f}, ratio {den / raw:.4f}")
    assert den < raw


# ---------------------------------------------------------------- 6. API surface
def test_api_rejects_bad_arguments(mrt):
    L = mrt.lib()
    r = mrt.Renderer(ref_scene(mrt, 5), "cpu")
    buf = np.zeros((8, 8, 4), dtype=np.float32)
    ok = mrt.render_desc(8, 8, 1)
    for flags in (0x1, 0x4, 0x8, 0x10, 0x40, 0x80, 0x2 | 0x1):
        with pytest.raises(mrt.MrtError, match="invalid"):
            r.render_aux(mrt.render_desc(8, 8, 1, flags=flags))
    n0, a0 = r.render_aux(ok)
    n1, a1 = r.render_aux(mrt.render_desc(8, 8, 1, numerics="fast"))  # accepted and ignored
    assert np.array_equal(bits(n0), bits(n1)) and np.array_equal(bits(a0), bits(a1))
    for args in ((None, C.byref(ok), buf.ctypes.data, buf.ctypes.data), (r._h, None, buf.ctypes.data, buf.ctypes.data),
                 (r._h, C.byref(ok), None, buf.ctypes.data), (r._h, C.byref(ok), buf.ctypes.data, None)):
        assert L.mrt_render_aux(*args) == 1
    for wh in ((0, 8), (8, 0)):
        with pytest.raises(mrt.MrtError, match="invalid"):
            r.render_aux(mrt.render_desc(wh[0], wh[1], 1))
    with pytest.raises(mrt.MrtError, match="GPU-backend"):
        r.render_aux_device(ok, buf.ctypes.data, buf.ctypes.data)
    r.close()
    p = mrt.default_denoise_params()
    assert p.iterations > 0 and min(p.sigma_color, p.sigma_normal, p.sigma_albedo, p.sigma_depth) > 0
    b = buf.ctypes.data
    for args in ((None, b, b, 8, 8, C.byref(p), b), (b, None, b, 8, 8, C.byref(p), b), (b, b, None, 8, 8, C.byref(p), b),
                 (b, b, b, 8, 8, None, b), (b, b, b, 8, 8, C.byref(p), None), (b, b, b, 0, 8, C.byref(p), b),
                 (b, b, b, 8, 0, C.byref(p), b)):
        assert L.mrt_denoise(*args) == 1
    for args in ((None, b, b, 8, 8, C.byref(p), b, b, None), (b, b, b, 8, 8, C.byref(p), None, b, None),
                 (b, b, b, 8, 8, C.byref(p), b, None, None), (b, b, b, 0, 0, C.byref(p), b, b, None), (b, b, b, 8, 8, None, b, b, None)):
        assert L.mrt_denoise_device(*args) == 1
    assert set(["mrt_render_aux", "mrt_render_aux_device", "mrt_default_denoise_params", "mrt_denoise", "mrt_denoise_device"]) <= set(
        mrt._lib.EXPORTS)


def test_cli_denoise_and_aux_files_equal_the_python_api(mrt, tmp_path):
    """bin/mrt -backend cpu ... -denoise 5 -o x.pfm -aux p.  (-order path: the CPU backend's default
    is the reference's per-thread RNG order, whose image depends on thread scheduling; with per-path
    streams "equal to the Python API's arrays" is well defined.)"""
    out, pre = tmp_path / "x.pfm", tmp_path / "p"
    subprocess.run([os.path.join(ROOT, "bin", "mrt"), "-backend", "cpu", "-order", "path", "-scene", "5", "-width", "32", "-height", "32",
                    "-samples", "16", "-denoise", "5", "-o", str(out), "-aux", str(pre)], capture_output=True, text=True, timeout=120,
                   check=True)
    p = mrt.ParseArgv(["mrt", "-backend", "cpu", "-order", "path", "-scene", "5", "-width", "32", "-height", "32", "-samples", "16"])
    r = mrt.Renderer(ref_scene(mrt, 5), "cpu")
    d = mrt.render_desc(32, 32, 16, depth=p.max_bounces, max_luminance=p.max_luminance, mode=p.threading_mode, seed=p.seed,
                        tile_size=p.tile_size)
    img, _ = r.render(d)
    nrm, alb = r.render_aux(d)
    r.close()
    den = mrt.denoise(img, nrm, alb, params(mrt, 5))
    assert np.array_equal(bits(mrt.read_pfm(str(out))), bits(den[..., :3]))
    assert np.array_equal(bits(mrt.read_pfm(str(pre) + "_normal.pfm")), bits(nrm[..., :3]))
    assert np.array_equal(bits(mrt.read_pfm(str(pre) + "_albedo.pfm")), bits(alb[..., :3]))
    assert not np.array_equal(den, img)
    # three ranks, each filling its own pixels of the shared host buffers: the same three files
    out3, pre3 = tmp_path / "x3.pfm", tmp_path / "p3"
    subprocess.run([os.path.join(ROOT, "bin", "mrt"), "-backend", "cpu", "-order", "path", "-gpus", "3", "-tilesize", "8", "-scene", "5",
                    "-width", "32", "-height", "32", "-samples", "16", "-denoise", "5", "-o", str(out3), "-aux", str(pre3)],
                   capture_output=True, text=True, timeout=120, check=True)
    for a, b in ((out, out3), (str(pre) + "_normal.pfm", str(pre3) + "_normal.pfm"), (str(pre) + "_albedo.pfm", str(pre3) + "_albedo.pfm")):
        assert np.array_equal(bits(mrt.read_pfm(str(a))), bits(mrt.read_pfm(str(b))))
