"""The exact contract's range guards on edge-operand rays, without a GPU (tests/edge_rays.py).

The host forms of the short cores are IEEE operations (recip_nr is 1.0f / b, sqrt_core is sqrtf), so
this leg says nothing about the device's guards: it pins the EXPECTED values the GPU leg
(test_edge_rays_gpu.py) compares with -- the CPU backend's cast of every finite edge class equals the C
restatement bit for bit, and both equal the reference's own closest hits of the same rays
(tests/golden/edge_hits_<sid>.npz, written by tools/make_golden.py from the exact reference build) --
and it checks the inputs: each side of each guard a ray decides holds rays that hit.

Two rules throughout: a restatement (or reference) "hit" whose t is NaN is a miss record (cast_one
reports rec.t <= tmax; a rect reports such a hit for a zero direction component, as the reference
does), and a NaN equals a NaN (x86 and gfx950 produce default NaNs of different sign)."""
import os

import numpy as np
import pytest

import edge_rays as er
import synth_scenes as ss
from conftest import GOLDEN
from test_cast_host import BY_NAME, ENTRIES, NO_HIT, bits, fixture, miss_words, words
from test_synthetic_scenes import Synth, built, degenerate_normals

REF_SCENES = (0, 5, 6, 7, 8)
FIXTURE_SCENES = (5, 6, 7, 8)
KEYS = [f"scene_{sid}" for sid in REF_SCENES] + [e.name for e in ENTRIES]
# (key, guard side) pairs no ray of which can hit, each with its cause (DESIGN.md "Numerics", the
# guard inventory, says the same)
NO_HIT_SIDES = {
    # From an origin component above 2^60 the floats are 2^37 apart, wider than any of these scenes: the
    # two slab distances of the root's box along that axis are one float, so aabb::hit's hi > lo fails
    # (every graph here has a boxed root list or a bvh_node root), and a sphere's c = |oc|^2 - r^2 rounds
    # to |oc|^2 >= b^2.  No ray of that side hits in any of them (measured: 0 of 48 / 96 per scene); the
    # side is reached by rects in a list without a box, test_slowdiv_planes_beside_ordinary_rects.
    (key, "ray_nice: origin above 2^60") for key in KEYS
}
# (key, row) pairs of the reference fixtures that are known to differ, each with its cause: at most 8
# per scene, none in the axis class
EXPECTED_MISMATCHES = ()

_batch = {}


def view_of(mrt, key):
    """(the view to cast at, a Synth of it for the generator)."""
    if key.startswith("scene_"):
        sc = fixture(mrt, int(key[6:]))[0]
        return sc, Synth(sc)
    s, _ = built(mrt, BY_NAME[key])
    return s, s


def batch(mrt, key):
    """(view, rays, labels) of a key (computed once): FIXTURE_LIMIT rays for the fixture scenes, LIMIT otherwise."""
    if key not in _batch:
        sc, syn = view_of(mrt, key)
        limit = er.FIXTURE_LIMIT if key.startswith("scene_") and int(key[6:]) in FIXTURE_SCENES else er.LIMIT
        rays, labels = er.edge_rays(mrt, syn, 7000 + KEYS.index(key), limit)
        _batch[key] = (sc, rays, labels)
    return _batch[key]


def restate(orc, sc, rays, seed=0):
    """The restatement's records as words (mat left 0) and hit flags: ray i against oracle.hit(...,
    seed + i), under the cast's tmax rule (a NaN t is a miss)."""
    want = miss_words(len(rays))
    flag = np.zeros(len(rays), dtype=bool)
    for i, q in enumerate(rays):
        h, out = orc.hit(sc, q["o"], q["d"], q["time"], int(q["inside"]), seed=seed + i)
        if h and not np.isnan(out[0]):
            want[i, :7], want[i, 7], flag[i] = bits(out), 0, True
    return want, flag


_restated = {}


def restated(mrt, orc, key):
    if key not in _restated:
        sc, rays, _ = batch(mrt, key)
        _restated[key] = restate(orc, sc, rays)
    return _restated[key]


def same_words(a, b):
    """Equal bits, or NaN on both sides, per float word (t p n)."""
    fa, fb = a[:, :7].view(np.float32), b[:, :7].view(np.float32)
    return ((a[:, :7] == b[:, :7]) | (np.isnan(fa) & np.isnan(fb))).all(axis=1)


def assert_same_records(got, want, flag, labels, n_materials, skip=()):
    """got (HIT_DTYPE) against (want words, flag): the hit flags, t p n bit for bit (NaN == NaN), the
    miss records whole, mat a material index."""
    w = words(got)
    keep = np.ones(len(w), dtype=bool)
    keep[list(skip)] = False
    gflag = w[:, 7] != NO_HIT
    bad = keep & ((gflag != flag) | ~same_words(w, want))
    assert not bad.any(), (int(bad.sum()), [(int(i), str(labels[i])) for i in np.nonzero(bad)[0][:8]])
    assert np.array_equal(w[~gflag], miss_words(int((~gflag).sum())))
    assert (w[gflag, 7] < n_materials).all()


# ---------------------------------------------------------------- 1. the inputs
def test_guard_restatement_on_known_operands():
    o = np.zeros((6, 3), dtype=np.float32)
    d = np.array([[1, 1, 1], [1, 0, 0], [1, 2.0 ** -25, 1], [1, 2.0 ** -27, 1], [2.0 ** -27, 0, 0], [2.0 ** 26, 0, 0]], dtype=np.float32)
    f = er.ray_flags(o, d)
    assert f["dir_ok"].tolist() == [True, False, True, False, False, False]
    assert f["norm_ok"].tolist() == [True, True, True, True, False, False]
    o = np.array([[0, -0.0, 1], [2.0 ** -77, 1, 1], [np.nextafter(np.float32(2.0 ** -77), np.float32(0)), 1, 1], [-2.0 ** -149, 0, 0],
                  [2.0 ** 60, 1, 1], [np.nextafter(np.float32(2.0 ** 60), np.float32(np.inf)), 1, 1]], dtype=np.float32)
    f = er.ray_flags(o, np.ones((6, 3), dtype=np.float32))
    assert f["o_small"].tolist() == [False, False, True, True, False, False]
    assert f["o_large"].tolist() == [False, False, False, False, False, True]
    assert f["nice"].tolist() == [True, True, False, False, True, False]


@pytest.mark.parametrize("key", KEYS)
def test_each_guard_side_holds_rays_that_hit(mrt, orc, key):
    """Conditions on the inputs: per scene at least 32 rays on each side of normalize's and ray_nice's
    range tests hit something (by the restatement), the batch has every finite class within its limit,
    and the thin class sits on the values it names."""
    sc, rays, labels = batch(mrt, key)
    _, flag = restated(mrt, orc, key)
    assert len(rays) <= er.LIMIT and rays["tmax"].min() == np.inf
    kinds = set(int(k) & 0xFF for k in np.asarray(view_of(mrt, key)[1].nodes["kind"]))
    need = {"axis", "thin", "norm", "origin", "ordinary"}
    need |= {"plane"} if kinds & {ss.K_XY, ss.K_XZ, ss.K_YZ} else set()
    need |= {"box"} if kinds & {ss.K_BVH, ss.K_MESH} else set()
    need |= {"instance"} if kinds & {ss.K_TRANSLATE, ss.K_ROTY} else set()
    assert need <= set(labels), need - set(labels)
    assert np.isfinite(rays["o"]).all() and np.isfinite(rays["d"]).all()
    f = er.ray_flags(rays["o"], rays["d"])
    counts = {name: (int(mask(f).sum()), int((mask(f) & flag).sum())) for name, mask in er.GUARD_SIDES}
    print(key, len(rays), "rays,", int(flag.sum()), "hit;", counts)
    for name, (n, hits) in counts.items():
        if (key, name) not in NO_HIT_SIDES:
            assert hits >= 32, (key, name, n, hits)
    thin = np.abs(er.unit(rays["d"][labels == "thin"])[0]).min(axis=1)
    for v in (2.0 ** -26, np.nextafter(np.float32(2.0 ** -26), np.float32(0)), 2.0 ** -25, 2.0 ** -27):
        assert (thin == np.float32(v)).sum() >= 3, v
    dd = er.unit(rays["d"][labels == "norm"])[1]
    for v in (2.0 ** -52, 2.0 ** 52):
        assert (dd == np.float32(v)).any() and (dd == np.nextafter(np.float32(v), np.float32(0))).any(), v


# ---------------------------------------------------------------- 2. CPU backend == restatement
@pytest.mark.parametrize("key", KEYS)
def test_cpu_backend_equals_restatement_on_edge_rays(mrt, orc, key):
    sc, rays, labels = batch(mrt, key)
    want, flag = restated(mrt, orc, key)
    r = mrt.Renderer(sc, "cpu")
    got = r.cast_rays(rays, seed=0)
    r.close()
    assert_same_records(got, want, flag, labels, sc.view.n_materials)
    assert flag.any() and not flag.all()


# ---------------------------------------------------------------- 3. the reference itself
@pytest.mark.parametrize("sid", FIXTURE_SCENES)
def test_edge_rays_equal_the_reference_s_hits(mrt, orc, sid):
    """edge_hits_<sid>.npz: the exact reference build's own closest hits of this batch (the hits_<sid>
    layout: o 0:3, d 3:6, time 6, inside 7 and hit 8 as int32 bits, t p n 9:16).  The fixture's rays
    are the generator's, so a changed generator needs the fixture rewritten (tools/make_golden.py
    --only-edge)."""
    key = f"scene_{sid}"
    sc, rays, labels = batch(mrt, key)
    rec = np.load(os.path.join(GOLDEN, f"edge_hits_{sid}.npz"))["rays"]
    assert len(rec) == len(rays) <= er.FIXTURE_LIMIT
    assert np.array_equal(bits(rec[:, 0:3]), bits(rays["o"])) and np.array_equal(bits(rec[:, 3:6]), bits(rays["d"]))
    assert np.array_equal(bits(rec[:, 6]), bits(rays["time"])) and np.array_equal(bits(rec[:, 7]), rays["inside"])
    t = rec[:, 9]
    flag = (bits(rec[:, 8]) != 0) & ~np.isnan(t)
    want = miss_words(len(rec))
    want[flag, :7] = bits(rec[:, 9:16])[flag]
    want[flag, 7] = 0
    skip = [i for k, i in EXPECTED_MISMATCHES if k == key]
    assert len(skip) <= 8 and not (labels[skip] == "axis").any()
    rwant, rflag = restated(mrt, orc, key)
    keep = np.ones(len(rec), dtype=bool)
    keep[skip] = False
    bad = keep & ((rflag != flag) | ~same_words(rwant, want))
    assert not bad.any(), ("restatement", int(bad.sum()), [(int(i), str(labels[i])) for i in np.nonzero(bad)[0][:8]])
    r = mrt.Renderer(sc, "cpu")
    got = r.cast_rays(rays, seed=0)
    r.close()
    assert_same_records(got, want, flag, labels, sc.view.n_materials, skip)
    assert flag.sum() >= 256


# ---------------------------------------------------------------- 4. degenerate mesh normals
def mesh_rays(mrt, s, seed, n=1536):
    """Rays from around the mesh's box at points inside it."""
    rng = np.random.default_rng(seed)
    lo = np.asarray(s.mesh_nodes["bmin"], dtype=np.float64).min(axis=0)
    hi = np.asarray(s.mesh_nodes["bmax"], dtype=np.float64).max(axis=0)
    c, ext = 0.5 * (lo + hi), 0.5 * (hi - lo)
    u = rng.normal(size=(n, 3))
    o = c + 2.5 * ext.max() * u / np.linalg.norm(u, axis=1)[:, None]
    rays = np.zeros(n, dtype=mrt.RAY_DTYPE)
    rays["o"], rays["tmax"] = o.astype(np.float32), np.inf
    rays["d"] = ((lo + rng.random((n, 3)) * (hi - lo)) - o).astype(np.float32)
    return rays


def test_degenerate_mesh_normals(mrt, orc):
    s = degenerate_normals(mrt)
    rays = mesh_rays(mrt, s, 31)
    want, flag = restate(orc, s, rays)
    r = mrt.Renderer(s, "cpu")
    got = r.cast_rays(rays)
    r.close()
    assert_same_records(got, want, flag, np.full(len(rays), "mesh"), s.view.n_materials)
    nn = want[flag, 4:7].view(np.float32).astype(np.float64)
    ln = np.linalg.norm(nn, axis=1)
    # all three kinds of normal are hit: 0 / 0 = NaN, and unit normals from both rescaled thirds
    assert np.isnan(ln).sum() >= 32 and (np.abs(ln - 1) < 1e-5).sum() >= 256


# ---------------------------------------------------------------- 5. rects on slow-division planes
SLOW_PLANES = (1e-30, 2.0 ** -80, 2.0 ** 61, 2.0 ** -140)   # outside {0} U [2^-77, 2^60]: MRT_F_SLOWDIV on upload
PLAIN_PLANES = (0.0, 10.0, -25.0)


def slowdiv_rects(mrt):
    """Rects of all three kinds on ordinary and on MRT_F_SLOWDIV planes, both facings, in one list
    WITHOUT a box (no slab test in front of them: origins above 2^60 reach the rect tests)."""
    s = Synth(fixture(mrt, 5)[0]).clear()
    mats = [s.lambertian(0.6, 0.1, 0.1), s.lambertian(0.2, 0.5, 0.7)]
    items = []
    for i, kind in enumerate((ss.K_XY, ss.K_XZ, ss.K_YZ)):
        for j, k in enumerate(PLAIN_PLANES + SLOW_PLANES):
            items.append(s.rect(kind, -50, 50, -50, 50, k, mats[j % 2], 1.0 if (i + j) % 2 else -1.0))
    s.root = s.list(items)
    return s


def slowdiv_rays(mrt, s, seed):
    """Origins on each plane and one ulp to either side (perpendicular and oblique directions), axis
    rays from origins above 2^60, and ordinary rays from inside the rects' extent."""
    rng = np.random.default_rng(seed)
    F = np.float32
    o, d = [], []
    for n in s.nodes[:-1]:
        a, b, c = er.RECT_AXES[int(n["kind"]) & 0xFF]
        k = F(n["f"][4])
        for off in (k, np.nextafter(k, F(-np.inf)), np.nextafter(k, F(np.inf))):
            for j in range(4):
                p = rng.uniform(-45, 45, 3).astype(F)
                p[c] = off
                v = rng.uniform(-1, 1, 3).astype(F)
                if j < 2:
                    v[:] = 0
                    v[c] = 1 - 2 * j
                o.append(p)
                d.append(v)
    for c in range(3):
        for sign in (1.0, -1.0):
            for far in (np.nextafter(F(2.0 ** 60), F(np.inf)), F(2.0 ** 62), F(2.0 ** 100)):
                for _ in range(8):
                    p = rng.uniform(-45, 45, 3).astype(F)
                    p[c] = sign * far
                    v = np.zeros(3, dtype=F)
                    v[c] = -sign
                    o.append(p)
                    d.append(v)
    n_edge = len(o)
    o += list(rng.uniform(-50, 50, (512, 3)).astype(F))
    d += list((rng.uniform(-1, 1, (512, 3)) * rng.uniform(0.05, 20.0, (512, 1))).astype(F))
    rays = np.zeros(len(o), dtype=mrt.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = np.asarray(o), np.asarray(d), np.inf
    labels = np.array(["plane"] * n_edge + ["ordinary"] * 512)
    return rays, labels


_slow = {}


def slowdiv_case(mrt, orc):
    """(view, rays, labels, the restatement's words, its hit flags), computed once."""
    if not _slow:
        s = slowdiv_rects(mrt)
        rays, labels = slowdiv_rays(mrt, s, 61)
        _slow["case"] = (s, rays, labels) + restate(orc, s, rays)
    return _slow["case"]


def test_slowdiv_planes_beside_ordinary_rects(mrt, orc):
    s, rays, labels, want, flag = slowdiv_case(mrt, orc)
    r = mrt.Renderer(s, "cpu")
    got = r.cast_rays(rays)
    r.close()
    assert_same_records(got, want, flag, labels, s.view.n_materials)
    f = er.ray_flags(rays["o"], rays["d"])
    mat = words(got)[:, 7]
    assert (f["o_large"] & flag).sum() >= 32 and (f["o_small"] & flag).sum() >= 32 and (f["nice"] & flag).sum() >= 32
    # hits on the planes near zero (0, 1e-30, 2^-80, 2^-140 are one place to a hit point), at 2^61 and on
    # the ordinary ones, per axis
    t = want[:, 0].view(np.float32)
    assert flag.sum() > 400 and np.isfinite(t[flag]).all()
    for c in range(3):
        pc = want[flag, 1 + c].view(np.float32).astype(np.float64)
        on_axis = want[flag, 4 + c].view(np.float32) != 0
        print("axis", c, {k: int((on_axis & (np.abs(pc - k) <= 1e-3 + 1e-6 * abs(k))).sum()) for k in (0.0, 10.0, -25.0, 2.0 ** 61)})
        for k, least in ((0.0, 16), (10.0, 4), (-25.0, 4), (2.0 ** 61, 4)):
            assert (on_axis & (np.abs(pc - k) <= 1e-3 + 1e-6 * abs(k))).sum() >= least, (c, k)
    assert set(np.unique(mat[flag])) == {0, 1}


# ---------------------------------------------------------------- 6. the non-finite class, arrangements
@pytest.mark.parametrize("key", ["scene_5", "scene_7", "scene_8", "n_bvh_with_instance_leaf"])
def test_non_finite_rays_on_cpu_backend(mrt, orc, key):
    """NaN / inf operands, a zero direction, 3e38 directions: the CPU backend rejects none and equals
    the restatement (the records the GPU leg's last test expects)."""
    sc, syn = view_of(mrt, key)
    rays, labels = er.nonfinite_rays(mrt, syn, 99)
    assert 64 <= len(rays) <= 256 and not (np.isfinite(rays["o"]).all(axis=1) & np.isfinite(rays["d"]).all(axis=1) &
                                            (np.abs(rays["d"]).max(axis=1) < 1e38) & (rays["d"] != 0).any(axis=1)).any()
    want, flag = restate(orc, sc, rays)
    r = mrt.Renderer(sc, "cpu")
    got = r.cast_rays(rays)
    r.close()
    assert_same_records(got, want, flag, labels, sc.view.n_materials)


def test_arrangements():
    labels = np.array(["ordinary"] * 300 + ["axis"] * 20 + ["thin"] * 5)
    a = er.arrangements(labels, 3)
    assert sorted(a["sorted"]) == sorted(a["shuffled"]) == list(range(325)) and (labels[a["sorted"]][:20] == "axis").all()
    lone = labels[a["lone"]].reshape(-1, 64)
    assert len(lone) == 8 + 5 and ((lone != "ordinary").sum(axis=1) == 1).all()
    assert {int(np.nonzero(g != "ordinary")[0][0]) for g in lone} == {0, 31, 32, 63}
