"""Ray queries (include/mrt.h "ray queries") without a GPU: the CPU backend's mrt_cast_rays against
the reference's own closest hits (tests/golden/hits_<0..9>.npz) and the C restatement, the pixel-ray
helper against its formula, the argument checks, and bin/mrt -pick / -focusat with -backend cpu.

Every comparison is of bits.  EXPECTED_MISMATCHES lists the fixture rays the product's hit code is
known to answer differently from the reference (none)."""
import os
import subprocess

import numpy as np
import pytest

import synth_scenes as ss
from conftest import GOLDEN, ROOT, SCENE_SIZES
from test_synthetic_scenes import CATALOGUE, built

F32 = np.float32
INF_BITS, NO_HIT = 0x7F800000, 0xFFFFFFFF
# (scene, fixture row) pairs the fixture test skips, each with its cause: at most 8 per scene, none
# for scenes 5, 7, 8, 9
EXPECTED_MISMATCHES = ()

BY_NAME = {e.name: e for e in CATALOGUE}
# one catalogue entry per kernel variant (the literal it names) ...
PER_VARIANT = ["b_cornell_lookalike", "c_room_mesh_lookalike", "c_room_mesh_lookalike_metal", "a_cornell_plus_sphere",
               "c_room_mesh_plus_sphere", "j_tree_list_leaves", "l_smoke_plus_lambertian_sphere", "h_moving_sphere",
               "d_biased_light_and_sphere", "n_bvh_with_instance_leaf"]
# ... the mesh under instances, the live constant_volume, the deep chains, the pod_bvh with 100-triangle leaves
EXTRA = ["i_teapot_translate_rotate", "l_live_volume_biased_sphere", "j_chain_depth_40", "j_chain_depth_70", "m_mesh_reshaped"]
ENTRIES = [BY_NAME[n] for n in PER_VARIANT + EXTRA]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def words(hits):
    """HIT_DTYPE records as (n, 8) uint32 words: t, p, n, mat."""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 8)


def miss_words(n):
    w = np.zeros((n, 8), dtype=np.uint32)
    w[:, 0], w[:, 7] = INF_BITS, NO_HIT
    return w


_fixtures = {}


def fixture(mrt, sid):
    """(scene, rays, hit flags, the reference's t p n words) of hits_<sid>.npz; rows: o 0:3, d 3:6,
    time 6, inside 7 and hit 8 as int32 bits, t p n 9:16."""
    if sid not in _fixtures:
        w, h = SCENE_SIZES[sid]
        rec = np.load(os.path.join(GOLDEN, f"hits_{sid}.npz"))["rays"]
        rays = np.zeros(len(rec), dtype=mrt.RAY_DTYPE)
        rays["o"], rays["d"], rays["time"], rays["tmax"] = rec[:, 0:3], rec[:, 3:6], rec[:, 6], np.inf
        rays["inside"] = np.ascontiguousarray(rec[:, 7]).view(np.int32)
        hit = np.ascontiguousarray(rec[:, 8]).view(np.int32) != 0
        _fixtures[sid] = (mrt.select_scene(sid, w / h), rays, hit, bits(rec[:, 9:16]))
    return _fixtures[sid]


def assert_equals_fixture(sid, got, hit, tpn):
    """The hit flag equals the fixture's and, where it hits, t p n are the fixture's bits; a miss is
    the miss record."""
    w = words(got)
    keep = np.ones(len(hit), dtype=bool)
    keep[[i for s, i in EXPECTED_MISMATCHES if s == sid]] = False
    flag = w[:, 7] != NO_HIT
    bad = keep & ((flag != hit) | (hit & (w[:, :7] != tpn).any(axis=1)))
    assert not bad.any(), (sid, int(bad.sum()), np.nonzero(bad)[0][:8])
    assert np.array_equal(w[~flag], miss_words(int((~flag).sum())))
    assert hit.any() and not hit.all()


_cpu = {}


def cpu_renderer(mrt, sid):
    if sid not in _cpu:
        _cpu[sid] = mrt.Renderer(fixture(mrt, sid)[0], "cpu")
    return _cpu[sid]


_full = {}


def cpu_full(mrt, sid):
    """The CPU backend's cast of the whole fixture, seed 0 (computed once)."""
    if sid not in _full:
        _full[sid] = cpu_renderer(mrt, sid).cast_rays(fixture(mrt, sid)[1], seed=0)
    return _full[sid]


# ---------------------------------------------------------------- 1. the fixtures
def sphere_material_by_geometry(s, rays, w):
    """Scenes whose hittable surfaces are all spheres in world space (scenes 0-4): the material of the
    sphere whose surface holds each hit point, or -1 where two spheres are about equally near."""
    nodes = ss._arr(s.view.nodes, s.view.n_nodes, ss.NODE)
    sp = nodes[(nodes["kind"] & 0xFF) == ss.K_SPHERE]
    f = sp["f"].astype(np.float64)
    p = w[:, 1:4].view(np.float32).astype(np.float64)
    tm = rays["time"].astype(np.float64)[:, None, None]
    moving = ((sp["kind"] >> 16) & ss.F_MOVING) != 0
    span = np.where(moving, f[:, 7] - f[:, 6], 1.0)
    c = f[None, :, 0:3] + np.where(moving, 1.0, 0.0)[None, :, None] * ((tm - f[None, :, 6:7]) / span[None, :, None]) * (f[None, :, 3:6] - f[None, :, 0:3])
    err = np.abs(np.linalg.norm(p[:, None, :] - c, axis=2) - np.abs(f[None, :, 8]))  # (float32 points on a radius of up to 1000: ~1e-4)
    order = np.argsort(err, axis=1)
    best, second = np.take_along_axis(err, order[:, :1], 1)[:, 0], np.take_along_axis(err, order[:, 1:2], 1)[:, 0]
    mat = sp["mat"][order[:, 0]].astype(np.int64)
    mat[~((best < 1e-3) & (second > 1e-2))] = -1
    return mat


@pytest.mark.parametrize("sid", sorted(SCENE_SIZES))
def test_cast_equals_reference_hits(mrt, sid):
    """All 2048 rays of hits_<sid>.npz, seed 0: the reference's own closest hit, bit for bit.  mat is
    an index into the view's materials; in the sphere scenes 0-4 it is the material of the sphere the
    hit point lies on."""
    s, rays, hit, tpn = fixture(mrt, sid)
    got = cpu_full(mrt, sid)
    assert_equals_fixture(sid, got, hit, tpn)
    w = words(got)
    flag = w[:, 7] != NO_HIT
    assert (w[flag, 7] < s.view.n_materials).all()
    if sid <= 4:
        want = sphere_material_by_geometry(s, rays, w)
        known = flag & (want >= 0)
        assert known.sum() > 0.9 * flag.sum()
        assert np.array_equal(w[known, 7].astype(np.int64), want[known])


# ---------------------------------------------------------------- 2. split batches
@pytest.mark.parametrize("sid", [6, 7])
def test_split_batch_equals_the_whole(mrt, sid):
    """Ray i draws from the stream keyed by seed + i: rows k: cast with seed = k are rows k: of the
    whole cast (scenes 6 and 7: constant_volumes draw)."""
    _, rays, _, _ = fixture(mrt, sid)
    full = words(cpu_full(mrt, sid))
    r = cpu_renderer(mrt, sid)
    for k in (1, 63, 64, 2047):
        assert np.array_equal(words(r.cast_rays(rays[k:], seed=k)), full[k:]), k
    # the stream matters: under another seed book2's volume hits move (no fixture ray of scene 6
    # ends inside its smoke, in the reference's own records either)
    if sid == 7:
        assert not np.array_equal(words(r.cast_rays(rays, seed=1)), full)


# ---------------------------------------------------------------- 3. tmax
def tmax_cases(rays, full):
    """(label, the batch with a new tmax on its hitting rays, their rows, the words expected there):
    tmax = t keeps the record; nextafter(t, 0), NaN, 0 and 0.001 miss.  The batch keeps its length, so
    every ray keeps its stream."""
    w = words(full)
    at = np.nonzero(w[:, 7] != NO_HIT)[0]
    t = w[at, 0].view(np.float32)
    out = []
    for label, tmax, keeps in (("t", t, True), ("below t", np.nextafter(t, F32(0)), False), ("nan", np.nan, False), ("0", 0.0, False),
                               ("0.001", F32(0.001), False)):
        whole = rays.copy()
        whole["tmax"][at] = tmax
        out.append((label, whole, at, w[at] if keeps else miss_words(len(at))))
    return out


@pytest.mark.parametrize("sid", [5, 7])
def test_tmax_rule(mrt, sid):
    _, rays, _, _ = fixture(mrt, sid)
    r = cpu_renderer(mrt, sid)
    for label, whole, at, want in tmax_cases(rays, cpu_full(mrt, sid)):
        assert np.array_equal(words(r.cast_rays(whole, seed=0))[at], want), label


# ---------------------------------------------------------------- 4. the synthetic catalogue
def scene_bounds(s):
    """A box around the primitives of a view, from the numbers of its sphere, rect and mesh nodes
    (instances move their children by a little; the box only seeds ray origins)."""
    lo, hi = [np.full(3, np.inf)], [np.full(3, -np.inf)]
    nodes = np.asarray(s.nodes)
    kind = nodes["kind"] & 0xFF
    for n in nodes[kind == ss.K_SPHERE]:
        f = n["f"].astype(np.float64)
        for c in (f[0:3], f[3:6]):
            lo.append(c - abs(f[8]))
            hi.append(c + abs(f[8]))
    for k, (a, b, c) in ((ss.K_XY, (0, 1, 2)), (ss.K_XZ, (0, 2, 1)), (ss.K_YZ, (1, 2, 0))):
        for n in nodes[kind == k]:
            f = n["f"].astype(np.float64)
            p0, p1 = np.zeros(3), np.zeros(3)
            p0[a], p1[a], p0[b], p1[b], p0[c], p1[c] = f[0], f[1], f[2], f[3], f[4], f[4]
            lo.append(p0)
            hi.append(p1)
    if len(s.mesh_nodes):
        lo.append(np.asarray(s.mesh_nodes["bmin"], dtype=np.float64).min(axis=0))
        hi.append(np.asarray(s.mesh_nodes["bmax"], dtype=np.float64).max(axis=0))
    lo, hi = np.min(lo, axis=0), np.max(hi, axis=0)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()
    return lo, hi


def entry_rays(mrt, s, seed):
    """24 x 24 pixel-centre camera rays, then 512 seeded rays from inside the scene's bounds with
    non-unit directions, a third of them flagged inside, at random times."""
    ys, xs = np.divmod(np.arange(24 * 24), 24)
    cam = mrt.camera_pixel_rays(s.camera, 24, 24, xs, ys)
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(s)
    rnd = np.zeros(512, dtype=mrt.RAY_DTYPE)
    rnd["o"] = (lo + rng.random((512, 3)) * (hi - lo)).astype(F32)
    rnd["d"] = (rng.uniform(-1, 1, (512, 3)) * rng.uniform(0.05, 20.0, (512, 1))).astype(F32)
    rnd["time"] = rng.random(512).astype(F32)
    rnd["tmax"] = np.inf
    rnd["inside"] = rng.integers(0, 3, 512) == 0
    return np.concatenate([cam, rnd])


_entry = {}


def entry_reference(mrt, orc, e):
    """(view, rays, the restatement's records as words with mat left 0, its hit flags) of a catalogue
    entry (computed once): ray i against oracle.hit(..., seed=i)."""
    if e.name not in _entry:
        s, _ = built(mrt, e)
        rays = entry_rays(mrt, s, 1000 + CATALOGUE.index(e))
        want = miss_words(len(rays))
        flag = np.zeros(len(rays), dtype=bool)
        for i, q in enumerate(rays):
            h, out = orc.hit(s, q["o"], q["d"], q["time"], int(q["inside"]), seed=i)
            if h:
                want[i, :7], want[i, 7], flag[i] = bits(out), 0, True
        _entry[e.name] = (s, rays, want, flag)
    return _entry[e.name]


def assert_equals_restatement(s, got, want, flag):
    w = words(got)
    assert np.array_equal(w[:, 7] != NO_HIT, flag)
    assert np.array_equal(w[:, :7], want[:, :7])
    assert np.array_equal(w[~flag], want[~flag])
    # mat: an index into the view's materials that some node of the graph carries
    used = np.unique(np.asarray(s.nodes["mat"]))
    assert (w[flag, 7] < len(s.materials)).all() and np.isin(w[flag, 7], used).all()
    assert flag[:576].any() and flag[576:].any()


@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: e.name)
def test_catalogue_cast_equals_restatement(mrt, orc, e):
    """Graphs no reference scene builds: the CPU backend's records equal the restatement's hit bit
    for bit, for camera rays and for rays from inside the scene.  Where every surface is a sphere in
    world space (the bvh_node trees and chains) mat is the material of the sphere hit."""
    s, rays, want, flag = entry_reference(mrt, orc, e)
    r = mrt.Renderer(s, "cpu")
    got = r.cast_rays(rays, seed=0)
    r.close()
    assert_equals_restatement(s, got, want, flag)
    kinds = set(int(k) for k in np.unique(np.asarray(s.nodes["kind"]) & 0xFF))
    if kinds <= {ss.K_LIST, ss.K_BVH, ss.K_SPHERE}:
        w = words(got)
        mat = sphere_material_by_geometry(s, rays, w)
        known = flag & (mat >= 0)
        assert known.sum() > 0.5 * flag.sum()
        assert np.array_equal(w[known, 7].astype(np.int64), mat[known])


def test_catalogue_selection_covers_every_variant():
    assert len({BY_NAME[n].kernel for n in PER_VARIANT}) == len(PER_VARIANT) == 10


# ---------------------------------------------------------------- 5. mrt_camera_pixel_ray
def pixel_rays_numpy(cam, W, H, xs, ys):
    """The stated formula in numpy float32 (every operation rounds to float32, in this order)."""
    c = {k: np.array(getattr(cam, k)[:3], dtype=F32) for k in ("origin", "llcorner", "horz", "vert")}
    s = ((xs.astype(F32) + F32(0.5)) / F32(W))[:, None]
    t = ((ys.astype(F32) + F32(0.5)) / F32(H))[:, None]
    d = ((c["llcorner"] + s * c["horz"]) + t * c["vert"]) - c["origin"]
    return c["origin"], d.astype(F32)


@pytest.mark.parametrize("W,H", [(1, 1), (37, 23), (500, 500)])
def test_camera_pixel_ray_equals_its_formula(mrt, W, H):
    cam = fixture(mrt, 7)[0].view.camera  # book2: an oblique camera, time0 = 0, time1 = 1
    rng = np.random.default_rng(W * 1000 + H)
    xs = np.concatenate([[0, W - 1, 0, W - 1], rng.integers(0, W, 64)])
    ys = np.concatenate([[0, 0, H - 1, H - 1], rng.integers(0, H, 64)])
    rays = mrt.camera_pixel_rays(cam, W, H, xs, ys)
    o, d = pixel_rays_numpy(cam, W, H, xs, ys)
    assert np.array_equal(bits(rays["d"]), bits(d))
    assert np.array_equal(bits(rays["o"]), bits(np.broadcast_to(o, d.shape)))
    assert np.array_equal(bits(rays["time"]), bits(np.full(len(xs), cam.time0, F32)))
    assert (bits(rays["tmax"]) == INF_BITS).all() and not rays["inside"].any() and not rays["reserved"].any()
    for x, y, w, h in ((W, 0, W, H), (0, H, W, H), (0, 0, 0, H), (0, 0, W, 0)):
        with pytest.raises(mrt.MrtError):
            mrt.camera_pixel_rays(cam, w, h, [x], [y])


# ---------------------------------------------------------------- 6. arguments
def test_argument_checks(mrt):
    import ctypes as C
    s, rays, _, _ = fixture(mrt, 5)
    r = cpu_renderer(mrt, 5)
    L = mrt.lib()
    hits = np.zeros(4, dtype=mrt.HIT_DTYPE)
    rp, hp = C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data)
    INVALID = 1
    assert L.mrt_cast_rays(None, rp, 4, 0, hp) == INVALID
    assert L.mrt_cast_rays(r._h, None, 4, 0, hp) == INVALID
    assert L.mrt_cast_rays(r._h, rp, 4, 0, None) == INVALID
    # the device form on a CPU-backend scene
    assert L.mrt_cast_rays_device(r._h, rp, 4, 0, hp, None) == INVALID
    with pytest.raises(mrt.MrtError):
        r.cast_rays_device(rays.ctypes.data, 4, hits.ctypes.data)
    # n == 0: nothing read, nothing written (null pointers are fine)
    assert L.mrt_cast_rays(r._h, None, 0, 0, None) == 0
    assert len(r.cast_rays(rays[:0])) == 0 and r.cast_rays(np.zeros((0, 8), F32)).dtype == mrt.HIT_DTYPE
    # the (n, 8) form: o, time, d, tmax with inside = 0
    q = rays[:256].copy()
    q["inside"] = 0
    q["tmax"][::3] = 300.0
    flat = np.zeros((256, 8), dtype=F32)
    flat[:, 0:3], flat[:, 3], flat[:, 4:7], flat[:, 7] = q["o"], q["time"], q["d"], q["tmax"]
    assert np.array_equal(words(r.cast_rays(flat)), words(r.cast_rays(q)))
    # reserved is ignored, inside is read
    junk = q.copy()
    junk["reserved"] = 0xDEADBEEF
    assert np.array_equal(words(r.cast_rays(junk)), words(r.cast_rays(q)))
    for bad in (np.zeros((3, 7), F32), np.zeros((3, 8), np.float64), np.zeros(8, F32)):
        with pytest.raises(ValueError):
            r.cast_rays(bad)
    # a seed near 2^64 wraps
    assert np.array_equal(words(r.cast_rays(q, seed=2 ** 64 - 3)), words(r.cast_rays(q, seed=-3)))
    # no ray is rejected: non-finite origins and directions, a zero direction
    odd = rays[:8].copy()
    odd["o"][0, 0], odd["d"][1, 1], odd["o"][2, 2], odd["d"][3] = np.nan, np.nan, np.inf, (np.inf, 0, -np.inf)
    odd["d"][4] = 0
    odd["o"][5], odd["d"][5] = (1e38, -1e38, 1e38), (3e38, 3e38, 3e38)
    w = words(r.cast_rays(odd))
    miss = w[:, 7] == NO_HIT
    assert np.array_equal(w[miss], miss_words(int(miss.sum()))) and (w[~miss, 7] < s.view.n_materials).all()
    assert np.array_equal(w[6:], words(cpu_full(mrt, 5))[6:8])


# ---------------------------------------------------------------- 7. the command line
EXE = os.path.join(ROOT, "bin", "mrt")


def cli(*args, check=True):
    return subprocess.run([EXE, "-backend", "cpu", "-order", "path"] + [str(a) for a in args], capture_output=True, text=True, timeout=120, check=check)


def test_cli_pick(mrt):
    """-pick X Y prints, before the Trace line, what cast_rays returns for that pixel's ray."""
    s = fixture(mrt, 5)[0]
    x, y = 40, 9
    out = cli("-scene", 5, "-width", 64, "-height", 64, "-samples", 1, "-pick", x, y).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("pick ")]
    assert len(line) == 1 and out.index("pick ") < out.index("Trace:")
    sc = mrt.select_scene(5, 1.0)
    r = mrt.Renderer(sc, "cpu")
    h = r.cast_rays(mrt.camera_pixel_rays(sc.view.camera, 64, 64, [x], [y]))[0]
    r.close()
    assert h["mat"] != NO_HIT
    f = lambda v: "%.9g" % float(v)
    assert line[0] == (f"pick {x} {y}: t={f(h['t'])} p=({f(h['p'][0])} {f(h['p'][1])} {f(h['p'][2])}) "
                       f"n=({f(h['n'][0])} {f(h['n'][1])} {f(h['n'][2])}) mat={int(h['mat'])}")
    # the sky of scene 0
    out = cli("-scene", 0, "-width", 64, "-height", 32, "-samples", 1, "-pick", 32, 31).stdout
    assert "pick 32 31: miss\n" in out
    out = cli("-scene", 0, "-width", 64, "-height", 32, "-samples", 1, "-focusat", 32, 31).stdout
    assert "focusat 32 31: miss\n" in out
    for bad in (["-pick", 64, 0], ["-pick", 0, 32], ["-focusat", -1, 0], ["-pick", 3], ["-focusat", "a", 1]):
        assert cli("-scene", 0, "-width", 64, "-height", 32, "-samples", 1, *bad, check=False).returncode != 0, bad


def test_cli_focusat_renders_as_focus(mrt, tmp_path):
    """-focusat X Y writes the image -focus F writes, F from its printed line; the focus is the hit's
    depth along the view axis."""
    base = ["-scene", 5, "-width", 32, "-height", 32, "-samples", 4, "-aperture", 20]
    a, b = tmp_path / "a.pfm", tmp_path / "b.pfm"
    out = cli(*base, "-focusat", 20, 7, "-o", a).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("focusat 20 7: focus=")]
    assert len(line) == 1
    F = line[0].split("=")[1]
    cli(*base, "-focus", F, "-o", b)
    assert a.read_bytes() == b.read_bytes()
    plain = tmp_path / "c.pfm"
    cli(*base, "-o", plain)
    assert plain.read_bytes() != a.read_bytes()
    sc = mrt.select_scene(5, 1.0)
    cam = mrt.make_camera(sc.camera_params(), aperture=20.0)
    q = mrt.camera_pixel_rays(cam, 32, 32, [20], [7])
    r = mrt.Renderer(sc, "cpu")
    h = r.cast_rays(q)[0]
    r.close()
    d = q["d"][0]
    dl = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    w = np.array(cam.w[:3], dtype=F32)
    dw = ((d[0] / dl) * w[0] + (d[1] / dl) * w[1]) + (d[2] / dl) * w[2]
    assert F32(float(F)) == F32(h["t"]) * -dw
