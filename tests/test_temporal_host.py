"""Camera control and temporal reprojection on the host (CPU only): mrt_make_camera is the scene
builders' own camera arithmetic, mrt_scene_set_camera on the CPU backend equals a fresh upload,
mrt_reproject follows the formulas of include/mrt_temporal.h on synthetic frames (blend, each
rejection alone, the sign and row conventions on a shifted plane), and the Cornell orbit it was
built for: accumulated frames are closer to a 1024-spp render than the raw frame is."""
import ctypes as C
import types

import numpy as np
import pytest

from test_aux_host import bits, ref_scene, rmse

F32 = np.float32


def cam_bytes(cam):
    return bytes(cam)


def with_camera(scene, cam):
    """A scene whose view carries `cam`: what Renderer uploads (the arrays stay the blob's)."""
    view = type(scene.view)()
    C.memmove(C.byref(view), C.byref(scene.view), C.sizeof(view))
    view.camera = cam
    return types.SimpleNamespace(view=view, scene_id=scene.scene_id, _keep=scene)


def second_camera(mrt, scene):
    """Camera B of a scene: its own parameters, moved, turned and narrowed."""
    p = scene.camera_params()
    d = np.array(p.pos[:]) - np.array(p.lookat[:])
    return mrt.make_camera(p, pos=np.array(p.pos[:]) + 0.07 * np.array([d[2], 0.3 * np.linalg.norm(d), -d[0]]), vfov_deg=p.vfov_deg * 0.8)


# ---------------------------------------------------------------- 1. the camera builder
@pytest.mark.parametrize("sid,aspect", [(s, 1.0) for s in range(10)] + [(0, 2.0), (5, 2.0)])
def test_make_camera_is_the_builders_camera(mrt, sid, aspect):
    sc = ref_scene(mrt, sid, aspect)
    p = sc.camera_params()
    assert p.aspect == aspect and p.vfov_deg > 0 and p.focus_dist > 0
    assert cam_bytes(mrt.make_camera(p)) == cam_bytes(sc.view.camera)


def test_make_camera_rejects_degenerate_frames(mrt):
    L = mrt.lib()
    good = dict(pos=(1, 2, 3), lookat=(0, 0, 0), up=(0, 1, 0), vfov_deg=40, aspect=1.5, aperture=0.1, focus_dist=3, time0=0, time1=1)
    mrt.make_camera(**good)
    bad = [dict(lookat=good["pos"]), dict(pos=(0, 5, 0)), dict(pos=(0, -5, 0)), dict(up=(0, 0, 0)), dict(vfov_deg=0), dict(vfov_deg=180),
           dict(vfov_deg=-3), dict(focus_dist=0), dict(focus_dist=-1), dict(aspect=0)]
    bad += [{k: v} for k in ("vfov_deg", "aspect", "aperture", "focus_dist", "time0", "time1") for v in (np.nan, np.inf)]
    bad += [{k: (1, v, 3)} for k in ("pos", "lookat", "up") for v in (np.nan, -np.inf)]
    for b in bad:
        with pytest.raises(mrt.MrtError):
            mrt.make_camera(**{**good, **b})
    p, cam = mrt._lib.MrtCameraParams(), mrt._lib.MrtCamera()
    assert L.mrt_make_camera(None, C.byref(cam)) == 1 and L.mrt_make_camera(C.byref(p), None) == 1
    assert L.mrt_scene_camera_params(None, C.byref(p)) == 1
    assert {"mrt_make_camera", "mrt_scene_camera_params", "mrt_scene_set_camera", "mrt_scene_set_camera_device", "mrt_default_temporal_params",
            "mrt_reproject", "mrt_reproject_device"} <= set(mrt._lib.EXPORTS)
    assert L.mrt_abi_version() == 6


# ---------------------------------------------------------------- 2. set_camera on the CPU backend
@pytest.mark.parametrize("sid", [0, 5])
def test_set_camera_equals_an_upload_with_that_camera(mrt, sid):
    sc = ref_scene(mrt, sid)
    cam_a, cam_b = sc.view.camera, second_camera(mrt, sc)
    d = mrt.render_desc(32, 32, 16)
    rb = mrt.Renderer(with_camera(sc, cam_b), "cpu")
    want_b, rays_b = rb.render(d)
    aux_b = rb.render_aux(d)
    rb.close()
    r = mrt.Renderer(sc, "cpu")
    want_a, rays_a = r.render(d)
    aux_a = r.render_aux(d)
    assert not np.array_equal(bits(want_a), bits(want_b)) and not np.array_equal(bits(aux_a[1]), bits(aux_b[1]))
    for cam, want, rays, aux in ((cam_b, want_b, rays_b, aux_b), (cam_a, want_a, rays_a, aux_a)):
        r.set_camera(cam)
        got, n = r.render(d)
        assert n == rays and np.array_equal(bits(got), bits(want))
        g = r.render_aux(d)
        assert np.array_equal(bits(g[0]), bits(aux[0])) and np.array_equal(bits(g[1]), bits(aux[1]))
    bad = mrt._lib.MrtCamera()
    C.memmove(C.byref(bad), C.byref(cam_a), C.sizeof(bad))
    bad.horz[1] = np.nan
    with pytest.raises(mrt.MrtError):
        r.set_camera(bad)
    with pytest.raises(mrt.MrtError):
        r.set_camera(cam_a, stream_ptr=0)  # the stream-ordered form is the GPU backend's
    r.close()


# ---------------------------------------------------------------- 3. reprojection on synthetic frames
def plane_camera(mrt, w, h, shift=(0.0, 0.0)):
    """Looks down -z from (shift, 0): u = +x, v = +y, w = +z, the image plane at distance 1."""
    return mrt.make_camera(pos=(shift[0], shift[1], 0), lookat=(shift[0], shift[1], -1), up=(0, 1, 0), vfov_deg=50, aspect=w / h, aperture=0,
                           focus_dist=1)


def camera_f64(cam):
    return {k: np.array(getattr(cam, k)[:3], dtype=np.float64) for k in ("origin", "w", "llcorner", "horz", "vert")}


def pixel_dirs(cam, w, h):
    """float64 unit rays through the pixel centres, (h, w, 3)."""
    c = camera_f64(cam)
    s = ((np.arange(w) + 0.5) / w)[None, :, None]
    t = ((np.arange(h) + 0.5) / h)[:, None, None]
    d = c["llcorner"] + s * c["horz"] + t * c["vert"] - c["origin"]
    return d / np.linalg.norm(d, axis=2, keepdims=True)


def project_f64(cam, pts, w, h):
    """float64 restatement of step 3: continuous pixel coordinates and camera depth of world points."""
    c = camera_f64(cam)
    e = pts - c["origin"]
    zc = -(e @ c["w"])
    focus = (c["origin"] - c["llcorner"]) @ c["w"]
    q = e * (focus / zc)[..., None] - (c["llcorner"] - c["origin"])
    return (q @ c["horz"]) / (c["horz"] @ c["horz"]) * w - 0.5, (q @ c["vert"]) / (c["vert"] @ c["vert"]) * h - 0.5, zc


def synth(rng, w, h):
    """Colour, history (N = 3) and valid guides: random unit normals, albedo and depth, full coverage."""
    c = rng.random((h, w, 4)).astype(F32)
    hist = rng.random((h, w, 4)).astype(F32)
    hist[..., 3] = 3
    nrm = rng.normal(size=(h, w, 4)).astype(F32)
    nrm[..., 3] = 1
    alb = rng.random((h, w, 4)).astype(F32)
    alb[..., 3] = rng.uniform(2, 50, size=(h, w)).astype(F32)
    return c, hist, nrm, alb


def blend(c, hist, cap):
    """Step 5 in numpy float32 for a single tap of weight 1."""
    nn = np.minimum(hist[..., 3] + F32(1), F32(cap)).astype(F32)
    out = np.empty_like(c)
    out[..., :3] = hist[..., :3] + (c[..., :3] - hist[..., :3]) * (F32(1) / nn)[..., None]
    out[..., 3] = nn
    return out


def fresh(c):
    out = c.copy()
    out[..., 3] = 1
    return out


SHAPES = [(37, 23), (1, 1)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_same_camera_blends_each_pixel_with_its_own_history(mrt, w, h):
    rng = np.random.default_rng(w * 100 + h)
    c, hist, nrm, alb = synth(rng, w, h)
    cam = plane_camera(mrt, w, h)
    keep = [a.copy() for a in (c, hist, nrm, alb)]
    got = mrt.reproject(c, nrm, alb, cam, hist, nrm, alb, cam)
    assert np.array_equal(bits(got), bits(blend(c, hist, 32))) and (got[..., 3] == 4).all()  # N below the cap
    hist[..., 3] = 32
    got = mrt.reproject(c, nrm, alb, cam, hist, nrm, alb, cam)
    assert np.array_equal(bits(got), bits(blend(c, hist, 32))) and (got[..., 3] == 32).all()  # N at the cap
    hist[..., 3] = 3
    got = mrt.reproject(c, nrm, alb, cam, hist, nrm, alb, cam, mrt.default_temporal_params(max_history=2.5))
    assert np.array_equal(bits(got), bits(blend(c, hist, 2.5))) and (got[..., 3] == 2.5).all()
    assert np.array_equal(bits(mrt.reproject(c, nrm, alb, cam)), bits(fresh(c)))  # NULL history: the first frame
    for a, b in zip((c, hist, nrm, alb), keep):
        assert np.array_equal(bits(a), bits(b))  # the inputs are not written


def rotated(nrm, cos):
    """Unit-length copies of the normals turned so that n^ . n'^ = cos."""
    n = nrm[..., :3].astype(np.float64)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    t = np.cross(n, np.where(np.abs(n[..., :1]) < 0.9, [1.0, 0, 0], [0, 1.0, 0]))
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    out = nrm.copy()
    out[..., :3] = (cos * n + np.sqrt(1 - cos * cos) * t).astype(F32)
    return out


def _cur_coverage(n, a, pn, pa, m):
    n[..., 3][m] = 0.9375


def _prev_coverage(n, a, pn, pa, m):
    pn[..., 3][m] = 0.9375


def _cur_zero_normal(n, a, pn, pa, m):
    n[..., :3][m] = 0


def _prev_zero_normal(n, a, pn, pa, m):
    pn[..., :3][m] = 0


def _cur_no_depth(n, a, pn, pa, m):
    a[..., 3][m] = 0


def _normal_below_min(n, a, pn, pa, m):
    pn[m] = rotated(pn, 0.8)[m]  # normal_min is 0.9


def _depth_off(n, a, pn, pa, m):
    pa[..., 3][m] *= F32(1 + 2 * 0.02)


def _depth_off_below(n, a, pn, pa, m):
    pa[..., 3][m] *= F32(1 - 2 * 0.02)


def _albedo_off(n, a, pn, pa, m):
    pa[..., 1][m] += F32(2 * 0.1)


REJECTIONS = [_cur_coverage, _prev_coverage, _cur_zero_normal, _prev_zero_normal, _cur_no_depth, _normal_below_min, _depth_off, _depth_off_below,
              _albedo_off]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("violate", REJECTIONS, ids=[f.__name__[1:] for f in REJECTIONS])
def test_each_violation_alone_rejects_exactly_its_pixels(mrt, violate, w, h):
    rng = np.random.default_rng(w * 100 + h + 7)
    c, hist, nrm, alb = synth(rng, w, h)
    cam = plane_camera(mrt, w, h)
    m = rng.random((h, w)) < 0.3
    m.flat[0] = True
    pn, pa = nrm.copy(), alb.copy()
    violate(nrm, alb, pn, pa, m)
    got = mrt.reproject(c, nrm, alb, cam, hist, pn, pa, cam)
    want = np.where(m[..., None], fresh(c), blend(c, hist, 32))
    assert np.array_equal(bits(got), bits(want))
    # just inside each tolerance nothing is rejected
    with np.errstate(all="ignore"):
        pn, pa = rotated(nrm, 0.95), alb.copy()
    pn[..., 3] = nrm[..., 3]
    pa[..., 3] *= F32(1.01)
    pa[..., 0] += F32(0.05)
    ok = (nrm[..., 3] == 1) & (alb[..., 3] > 0) & (np.abs(nrm[..., :3]).sum(axis=2) > 0)
    got = mrt.reproject(c, nrm, alb, cam, hist, pn, pa, cam)
    assert np.array_equal(bits(got), bits(np.where(ok[..., None], blend(c, hist, 32), fresh(c))))


@pytest.mark.parametrize("w,h", SHAPES)
def test_points_behind_or_beside_the_previous_camera_have_no_history(mrt, w, h):
    rng = np.random.default_rng(w + h)
    c, hist, nrm, alb = synth(rng, w, h)
    cam = plane_camera(mrt, w, h)
    pts = camera_f64(cam)["origin"] + alb[..., 3:4].astype(np.float64) * pixel_dirs(cam, w, h)
    # behind: the previous camera stands beyond every point (depths are below 50) and looks on, away from them
    behind = mrt.make_camera(pos=(0, 0, -60), lookat=(0, 0, -61), up=(0, 1, 0), vfov_deg=50, aspect=w / h, aperture=0, focus_dist=1)
    assert (project_f64(behind, pts, w, h)[2] < 0).all()
    # off screen: it looks along +x from far to the left, so every point is in front of it and beside its narrow view
    beside = mrt.make_camera(pos=(-200, 400, -20), lookat=(-199, 400, -20), up=(0, 1, 0), vfov_deg=20, aspect=w / h, aperture=0, focus_dist=1)
    fx, fy, zc = project_f64(beside, pts, w, h)
    assert (zc > 0).all() and (fy < -1.5).all()
    for prev in (behind, beside):
        pa = alb.copy()
        pa[..., 3] = np.linalg.norm(pts - camera_f64(prev)["origin"], axis=2).astype(F32).reshape(h, w)  # (the depth test would pass)
        assert np.array_equal(bits(mrt.reproject(c, nrm, alb, cam, hist, nrm, pa, prev)), bits(fresh(c)))


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kx,ky", [(3, 0), (-3, 0), (0, 2), (0, -2)])
def test_plane_shift_takes_the_neighbours_history(mrt, w, h, kx, ky):
    """A fronto-parallel plane at z = -4; the camera moves by exactly kx pixels' worth to the right
    (ky: up).  A pixel's world point then sits kx pixels further right in the previous frame: pixel
    (x, y) takes the history of (x + kx, y + ky) where that pixel exists and none elsewhere.  The
    float64 projection below, not the code under test, says which pixel that is."""
    rng = np.random.default_rng(w * 10 + h + kx + ky)
    c, hist, nrm, alb = synth(rng, w, h)
    dist = 4.0
    prev = plane_camera(mrt, w, h)
    pc = camera_f64(prev)
    pitch = np.array([pc["horz"][0] / w, pc["vert"][1] / h]) * dist  # a pixel's size on the plane (focus_dist 1)
    cam = plane_camera(mrt, w, h, shift=(kx * pitch[0], ky * pitch[1]))
    dirs = pixel_dirs(prev, w, h)  # both cameras: the same rays, a plane parallel to the shift
    nrm[..., :3] = (0, 0, 1)
    alb[..., :3] = (0.5, 0.25, 0.75)
    alb[..., 3] = (dist / -dirs[..., 2]).astype(F32)
    pts = camera_f64(cam)["origin"] + alb[..., 3:4].astype(np.float64) * pixel_dirs(cam, w, h)
    fx, fy, _ = project_f64(prev, pts, w, h)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    assert np.abs(fx - (xs + kx)).max() < 1e-3 and np.abs(fy - (ys + ky)).max() < 1e-3
    got = mrt.reproject(c, nrm, alb, cam, hist, nrm, alb, prev)
    sx, sy = xs + kx, ys + ky
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    taken = hist[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
    assert np.array_equal(bits(got), bits(np.where(inside[..., None], blend(c, taken, 32), fresh(c))))
    if w > 1:
        assert inside.any() and not inside.all()


def test_half_pixel_shift_is_the_bilinear_mean(mrt):
    """Half a pixel sideways: the two taps of a row weigh 1/2 each (not snapped: 1/2 > 1/32), and a
    rejected tap leaves the other one's history alone."""
    w, h = 9, 4
    rng = np.random.default_rng(5)
    c, hist, nrm, alb = synth(rng, w, h)
    prev = plane_camera(mrt, w, h)
    pc = camera_f64(prev)
    cam = plane_camera(mrt, w, h, shift=(0.5 * pc["horz"][0] / w * 4.0, 0.0))
    nrm[..., :3] = (0, 0, 1)
    alb[..., :3] = 0.5
    alb[..., 3] = (4.0 / -pixel_dirs(prev, w, h)[..., 2]).astype(F32)
    hist[..., 3] = rng.integers(1, 9, size=(h, w)).astype(F32)
    pn = nrm.copy()
    pn[2, 4, 3] = 0.5  # one previous pixel without full coverage
    # (the plane's depth along neighbouring rays of this wide, coarse image differs by more than 2 %)
    got = mrt.reproject(c, nrm, alb, cam, hist, pn, alb, prev, mrt.default_temporal_params(depth_tol=0.2)).astype(np.float64)
    h64, c64 = hist.astype(np.float64), c.astype(np.float64)
    for y in range(h):
        for x in range(w):
            taps = [(x + i, 0.5) for i in (0, 1) if x + i < w and pn[y, x + i, 3] == 1]
            sw = sum(t[1] for t in taps)
            if sw < 0.25:
                want = np.append(c64[y, x, :3], 1)
            else:
                hq = sum(wt * h64[y, xx] for xx, wt in taps) / sw
                want = np.append(hq[:3] + (c64[y, x, :3] - hq[:3]) / (hq[3] + 1), hq[3] + 1)
            assert np.abs(got[y, x] - want).max() < 1e-4, (x, y)


def test_reproject_rejects_bad_arguments(mrt):
    L = mrt.lib()
    rng = np.random.default_rng(1)
    c, hist, nrm, alb = synth(rng, 8, 8)
    cam = plane_camera(mrt, 8, 8)
    for kw in (dict(max_history=0.5), dict(max_history=np.nan), dict(normal_min=1.5), dict(normal_min=-1.5), dict(depth_tol=0), dict(depth_tol=-1),
               dict(albedo_tol=0), dict(min_weight=0), dict(min_weight=1.5), dict(min_weight=np.nan)):
        with pytest.raises(mrt.MrtError):
            mrt.reproject(c, nrm, alb, cam, hist, nrm, alb, cam, mrt.default_temporal_params(**kw))
    p = mrt.default_temporal_params()
    assert [round(getattr(p, k), 6) for k, _ in p._fields_] == [32, 0.9, 0.02, 0.1, 0.25]
    out = np.zeros_like(c)
    b, o, cm, pp = c.ctypes.data, out.ctypes.data, C.byref(cam), C.byref(p)
    for args in ((None, b, b, cm, b, b, b, cm, 8, 8, pp, o), (b, None, b, cm, b, b, b, cm, 8, 8, pp, o), (b, b, None, cm, b, b, b, cm, 8, 8, pp, o),
                 (b, b, b, None, b, b, b, cm, 8, 8, pp, o), (b, b, b, cm, b, None, b, cm, 8, 8, pp, o), (b, b, b, cm, b, b, None, cm, 8, 8, pp, o),
                 (b, b, b, cm, b, b, b, None, 8, 8, pp, o), (b, b, b, cm, b, b, b, cm, 0, 8, pp, o), (b, b, b, cm, b, b, b, cm, 8, 0, pp, o),
                 (b, b, b, cm, b, b, b, cm, 8, 8, None, o), (b, b, b, cm, b, b, b, cm, 8, 8, pp, None), (b, b, b, cm, b, b, b, cm, 8, 8, pp, b),
                 (b, b, b, cm, b, b, b, cm, 1 << 17, 1, pp, o)):
        assert L.mrt_reproject(*args) == 1
        assert L.mrt_reproject_device(*args, None) == 1  # checked before anything touches a device
    assert L.mrt_reproject(b, b, b, cm, None, None, None, None, 8, 8, pp, o) == 0  # the first frame needs no previous one


# ---------------------------------------------------------------- 4. the Cornell orbit
def splitmix64(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


ORBIT_CENTRE = (278.0, 278.0, 278.0)


def orbit_camera(mrt, scene, k, deg, centre=ORBIT_CENTRE):
    """Frame k of an orbit: the scene's camera looking at `centre`, its position turned about the
    vertical axis through it by k * deg (float64 trigonometry, rounded once)."""
    p = scene.camera_params()
    a = np.radians(k * deg)
    dx, dz = p.pos[0] - centre[0], p.pos[2] - centre[2]
    pos = (centre[0] + dx * np.cos(a) + dz * np.sin(a), p.pos[1], centre[2] - dx * np.sin(a) + dz * np.cos(a))
    return mrt.make_camera(p, pos=pos, lookat=centre)


def orbit_frames(mrt, r, scene, frames, deg, w=128, h=128, spp=16):
    """[(camera, colour, normal, albedo)] of an orbit on renderer r: frame k under the seed
    splitmix64(seed + k), the feature buffers at the render's 16 samples."""
    out = []
    for k in range(frames):
        cam = orbit_camera(mrt, scene, k, deg)
        r.set_camera(cam)
        d = mrt.render_desc(w, h, spp, seed=splitmix64(mrt.MAIN_SEED + k))
        img, _ = r.render(d)
        out.append((cam, img) + tuple(r.render_aux(d)))
    return out


def accumulate(mrt, seq, params=None):
    hist = None
    for k, (cam, img, nrm, alb) in enumerate(seq):
        if hist is None:
            hist = mrt.reproject(img, nrm, alb, cam, params=params)
        else:
            pcam, _, pn, pa = seq[k - 1]
            hist = mrt.reproject(img, nrm, alb, cam, hist, pn, pa, pcam, params)
    return hist


@pytest.mark.parametrize("deg", [2.0, 0.0], ids=["orbit_2deg", "static"])
def test_cornell_orbit_accumulates_towards_the_1024spp_frame(mrt, deg):
    """Six 16-spp frames of the Cornell box at 128 x 128 on the CPU backend, the camera orbiting the
    box centre by `deg` per frame, default parameters; the truth is the CPU backend's 1024-spp
    render at frame 5's camera.  Measured (float32 library code, this test): 2 degrees per frame:
    history share 0.8298 of the pixels (0.8574 fully covered), RMSE accumulated 0.05296 against raw
    0.07841, ratio 0.6755 (the float64 prototype: share 0.83, ratio 0.72); static camera: share
    0.9077 (every fully covered pixel), 0.07218 against 0.09227, ratio 0.7823 (the prototype: 0.073
    against 0.105).  The ratios are printed, not asserted."""
    sc = ref_scene(mrt, 5)
    r = mrt.Renderer(sc, "cpu")
    seq = orbit_frames(mrt, r, sc, 6, deg)
    truth, _ = r.render(mrt.render_desc(128, 128, 1024))  # (the camera is still frame 5's)
    r.close()
    hist = accumulate(mrt, seq)
    cam, img, nrm, alb = seq[-1]
    share = float((hist[..., 3] > 1).mean())
    covered = float(((nrm[..., 3] == 1) & (alb[..., 3] > 0)).mean())
    raw, acc = rmse(img, truth[..., :3].astype(np.float64)), rmse(hist, truth[..., :3].astype(np.float64))
    print(f"{deg} deg per frame: history share {share:.4f} (fully covered {covered:.4f}), mean N {hist[..., 3].mean():.3f}; "
          f"RMSE vs 1024 spp: raw {raw:.5f}, accumulated {acc:.5f}, ratio {acc / raw:.4f}")
    assert share >= 0.75
    assert acc < raw


# ---------------------------------------------------------------- the command line
def test_cli_camera_flags_and_temporal_sequence_equal_the_python_api(mrt, tmp_path):
    """bin/mrt -lookfrom / -lookat / -vfov move the camera of the uploaded scene; -frames 3 -orbit 2
    -temporal -denoise 1 writes NAME_000.pfm ...: frame k under the orbit camera and the seed
    splitmix64(seed + k), accumulated through mrt_reproject, filtered for output only (the history
    that frame 2 builds on is the unfiltered one).  Two ranks fill one host frame."""
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "bin", "mrt")
    base = ["-backend", "cpu", "-order", "path", "-scene", "5", "-width", "32", "-height", "32", "-samples", "16"]
    camflags = ["-lookfrom", "250", "300", "-760", "-lookat", "278", "278", "278", "-vfov", "35"]
    sc = ref_scene(mrt, 5)
    p = mrt.ParseArgv(["mrt"] + base)
    kw = dict(depth=p.max_bounces, max_luminance=p.max_luminance, mode=p.threading_mode, tile_size=p.tile_size)
    cp = sc.camera_params()
    cp.pos[:] = (250, 300, -760)
    cp.lookat[:] = (278, 278, 278)
    cp.vfov_deg = 35
    r = mrt.Renderer(sc, "cpu")
    # a still frame from the moved camera
    still = tmp_path / "still.pfm"
    subprocess.run([exe] + base + camflags + ["-o", str(still)], capture_output=True, text=True, timeout=120, check=True)
    r.set_camera(mrt.make_camera(cp))
    img, _ = r.render(mrt.render_desc(32, 32, 16, seed=p.seed, **kw))
    assert np.array_equal(bits(mrt.read_pfm(str(still))), bits(img[..., :3]))
    # the sequence
    run = subprocess.run([exe] + base + camflags + ["-gpus", "2", "-tilesize", "8", "-frames", "3", "-orbit", "2", "-temporal", "-denoise", "1", "-o",
                                                    str(tmp_path / "seq.pfm")], capture_output=True, text=True, timeout=120, check=True)
    assert run.stdout.count("frame 0") == 3, run.stdout
    hist = prev = None
    for k in range(3):
        a = np.radians(k * 2.0)
        dx, dz = cp.pos[0] - cp.lookat[0], cp.pos[2] - cp.lookat[2]
        cam = mrt.make_camera(cp, pos=(cp.lookat[0] + dx * np.cos(a) + dz * np.sin(a), cp.pos[1], cp.lookat[2] - dx * np.sin(a) + dz * np.cos(a)))
        r.set_camera(cam)
        d = mrt.render_desc(32, 32, 16, seed=splitmix64(p.seed + k), **kw)
        img, _ = r.render(d)
        nrm, alb = r.render_aux(d)
        hist = mrt.reproject(img, nrm, alb, cam) if hist is None else mrt.reproject(img, nrm, alb, cam, hist, prev[1], prev[2], prev[0])
        prev = (cam, nrm, alb)
        p1 = mrt.default_denoise_params()
        p1.iterations = 1
        assert np.array_equal(bits(mrt.read_pfm(str(tmp_path / f"seq_{k:03d}.pfm"))), bits(mrt.denoise(hist, nrm, alb, p1)[..., :3])), k
    assert (hist[..., 3] == 3).mean() > 0.5
    r.close()
    for bad in (["-temporal"], ["-orbit", "2"], ["-frames", "0"], ["-frames", "2", "-adaptive", "1"], ["-vfov", "0"]):
        assert subprocess.run([exe] + base + bad, capture_output=True, text=True, timeout=120).returncode == 1, bad
