"""Radiance queries (include/mrt.h "radiance queries") without a GPU: the CPU backend's mrt_trace_rays
against the reference's own per-path results (tests/golden/stream_<0..9>.npz) and the C restatement's
oracle_path, mrt_radiance_fold against the render's image, the records' rules, the argument checks, the
panorama helper and bin/mrt -pano with -backend cpu.

Every comparison of radiance is of bits.  At most 4096 paths per test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edge_rays as er
from conftest import ROOT, golden_stream
from test_cast_host import BY_NAME, ENTRIES
from test_edge_rays_host import view_of
from test_synthetic_scenes import built

F32 = np.float32
M64 = 2 ** 64 - 1
INVALID = 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def words(rad):
    """RADIANCE_DTYPE records as (n, 4) uint32 words: L, rays."""
    return np.ascontiguousarray(rad).view(np.uint32).reshape(-1, 4)


# ---------------------------------------------------------------- shared references (computed once)
_streams = {}


def stream_case(mrt, sid):
    """(scene, desc, fixture, the 256 path indices, their probes) of stream_<sid>.npz: paths spread
    over the image and the samples, the first and last pixel each with its first and last sample."""
    if sid not in _streams:
        g = golden_stream(f"stream_{sid}.npz")
        sc = mrt.select_scene(g["sid"], g["w"] / g["h"])
        d = mrt.render_desc(g["w"], g["h"], g["spp"], depth=g["depth"], mode=g["mode"])
        ns = d.sqrt_samples ** 2
        assert ns == g["spp"]
        n = g["w"] * g["h"] * ns
        ends = [0, ns - 1, n - ns, n - 1]
        rest = np.setdiff1d(np.unique(np.linspace(0, n - 1, 300).astype(np.int64) * 7919 % n), ends)[:252]
        idx = np.concatenate([ends, rest]).astype(np.int64)
        assert len(idx) == 256 and len(np.unique(idx)) == 256
        probes = mrt.camera_path_probes(sc.view.camera, d, idx // ns, idx % ns)
        _streams[sid] = (sc, d, g, idx, probes)
    return _streams[sid]


_cpu = {}


def cpu_renderer(mrt, sid):
    if sid not in _cpu:
        _cpu[sid] = mrt.Renderer(stream_case(mrt, sid)[0], "cpu")
    return _cpu[sid]


_cpu_stream = {}


def cpu_stream_records(mrt, sid):
    """The CPU backend's records of stream_case's probes at the fixture's depth (computed once)."""
    if sid not in _cpu_stream:
        _cpu_stream[sid] = cpu_renderer(mrt, sid).trace_rays(stream_case(mrt, sid)[4], stream_case(mrt, sid)[2]["depth"])
    return _cpu_stream[sid]


def entry_paths(mrt, e, w=37, h=23, spp=4, n=48):
    """(view, desc arguments, pixel and sample arrays, probes) of a catalogue entry at a ragged size:
    n seeded paths plus the four corners of (pixel, sample)."""
    s, _ = built(mrt, e)
    rng = np.random.default_rng(500 + ENTRIES.index(e))
    px = np.concatenate([[0, 0, w * h - 1, w * h - 1], rng.integers(0, w * h, n - 4)])
    sm = np.concatenate([[0, spp - 1, 0, spp - 1], rng.integers(0, spp, n - 4)])
    d = mrt.render_desc(w, h, spp)
    return s, (w, h, spp), px, sm, mrt.camera_path_probes(s.camera, d, px, sm)


_entry = {}


def entry_reference(mrt, orc, e, depth):
    """(view, probes, the restatement's records as words) of a catalogue entry at `depth` (computed once)."""
    key = (e.name, depth)
    if key not in _entry:
        s, (w, h, spp), px, sm, probes = entry_paths(mrt, e)
        od = orc.desc(w, h, spp, depth=depth)
        want = np.zeros((len(px), 4), dtype=np.uint32)
        for k in range(len(px)):
            rgb, rays = orc.path(s, od, int(px[k]) % w, int(px[k]) // w, int(sm[k]))
            want[k, :3], want[k, 3] = bits(rgb), rays
        _entry[key] = (s, probes, want)
    return _entry[key]


def edge_probes(mrt, rays, seed):
    """Caller rays (RAY_DTYPE) as probes: the ray's o, d, time and inside, stream i keyed by (seed, i)."""
    p = np.zeros(len(rays), dtype=mrt.PROBE_DTYPE)
    p["o"], p["d"], p["time"], p["inside"] = rays["o"], rays["d"], rays["time"], rays["inside"]
    for i in range(len(p)):
        p["rng_state"][i], p["rng_inc"][i] = mrt.probe_seed(seed, i)
    return p


EDGE_KEYS = ["scene_5", "scene_7", "scene_8", "n_bvh_with_instance_leaf"]
EDGE_DEPTH = 8
_edge = {}


def edge_case(mrt, key):
    """(view, probes) of a key: 1024 edge-operand rays of every finite class (tests/edge_rays.py, the
    generator's smallest batch) followed by the non-finite class, as probes (computed once)."""
    if key not in _edge:
        sc, syn = view_of(mrt, key)
        fin, _ = er.edge_rays(mrt, syn, 8100 + EDGE_KEYS.index(key), 1024)
        non, _ = er.nonfinite_rays(mrt, syn, 98)
        _edge[key] = (sc, edge_probes(mrt, np.concatenate([fin, non]), 77))
    return _edge[key]


_edge_cpu = {}


def cpu_edge_records(mrt, key):
    if key not in _edge_cpu:
        sc, probes = edge_case(mrt, key)
        r = mrt.Renderer(sc, "cpu")
        _edge_cpu[key] = r.trace_rays(probes, EDGE_DEPTH)[0]
        r.close()
    return _edge_cpu[key]


# ---------------------------------------------------------------- 1. the reference's own paths
@pytest.mark.parametrize("sid", range(10))
def test_camera_path_probes_trace_to_the_reference_s_paths(mrt, sid):
    """camera_path_probes -> trace_rays on the CPU backend: the fixture's path_rgb words and path_rays,
    at the fixture's depth.  Pins mrt_camera_path_probe's stream position (lens and motion blur on
    scenes 0, 1 and 7)."""
    _, _, g, idx, probes = stream_case(mrt, sid)
    rad, total = cpu_stream_records(mrt, sid)
    assert np.array_equal(bits(rad["L"]), bits(g["path_rgb"][idx]))
    assert np.array_equal(rad["rays"], g["path_rays"][idx].astype(np.uint32))
    assert total == int(g["path_rays"][idx].sum())
    assert not probes["inside"].any() and (rad["rays"] >= 1).all() and (rad["rays"] <= g["depth"] + 1).all()


# ---------------------------------------------------------------- 2. the C restatement
@pytest.mark.parametrize("depth", [0, 1, 32])
@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: e.name)
def test_catalogue_paths_equal_restatement(mrt, orc, e, depth):
    s, probes, want = entry_reference(mrt, orc, e, depth)
    r = mrt.Renderer(s, "cpu")
    rad, total = r.trace_rays(probes, depth)
    r.close()
    assert np.array_equal(words(rad), want)
    assert total == int(want[:, 3].sum()) and (rad["rays"] <= depth + 1).all()
    if depth == 0:
        assert (rad["rays"] == 1).all()


# ---------------------------------------------------------------- 3. the fold
@pytest.mark.parametrize("sid", [5, 7])
def test_fold_of_every_pixel_s_probes_is_the_render(mrt, sid):
    sc = stream_case(mrt, sid)[0]
    W, H, spp = 24, 16, 4
    d = mrt.render_desc(W, H, spp, depth=16)
    r = mrt.Renderer(sc, "cpu")
    cam = mrt.make_camera(sc.camera_params(), aspect=W / H)
    r.set_camera(cam)
    img, rays = r.render(d)
    px, sm = np.divmod(np.arange(W * H * spp), spp)
    rad, total = r.trace_rays(mrt.camera_path_probes(cam, d, px, sm), 16)
    r.close()
    out = mrt.radiance_fold(rad, spp, d.max_luminance)
    assert np.array_equal(bits(out), bits(img.reshape(-1, 4)))
    assert total == rays and img[..., :3].any()


def test_fold_nan_rule_and_clamp(mrt):
    rad = np.zeros(12, dtype=mrt.RADIANCE_DTYPE)
    rad["L"][0:4] = [(1, 2, 3), (np.nan, 0, 0), (0.5, 0.5, 0.5), (0, np.inf, 0)]  # the NaN rule, twice
    rad["L"][4:8] = [(4000, 4000, 4000), (0, 0, 0), (0, 0, 0), (0, 0, 0)]           # a mean above max_luminance
    rad["L"][8:12] = [(8000, 100, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    out = mrt.radiance_fold(rad, 4, 10.0)
    # group 0 in float32: c = (1,2,3); NaN sample -> c doubles (2,4,6); + 0.5 -> (2.5,4.5,6.5); inf sample -> doubles (5,9,13); / 4
    c = np.array([5, 9, 13], dtype=F32) / F32(4)
    lum = lambda v: (v[0] * F32(0.212655) + v[1] * F32(0.715158)) + v[2] * F32(0.072187)
    assert lum(c) <= F32(10.0)
    assert np.array_equal(bits(out[0]), bits(np.append(c, F32(0))))
    for g, first in ((1, (4000, 4000, 4000)), (2, (8000, 100, 0))):
        m = np.array(first, dtype=F32) / F32(4)
        l = lum(m)
        assert l > F32(10.0)
        want = m * (F32(10.0) / l)
        assert np.array_equal(bits(out[g]), bits(np.append(want, F32(0))))
        assert abs(float(lum(want)) - 10.0) < 1e-4
    # a large max_luminance leaves the mean alone
    big = mrt.radiance_fold(rad, 4, 1e30)
    assert np.array_equal(bits(big[1, :3]), bits(np.full(3, 1000.0, F32)))
    # group = 1: the record itself; a lone non-finite record folds to the empty sum
    one = mrt.radiance_fold(rad[:2], 1, 1e30)
    assert np.array_equal(bits(one), bits(np.array([[1, 2, 3, 0], [0, 0, 0, 0]], dtype=F32)))
    for bad_group in (0, 5):
        with pytest.raises(ValueError):
            mrt.radiance_fold(rad, bad_group)
    L = mrt.lib()
    o = np.zeros((3, 4), dtype=F32)
    assert L.mrt_radiance_fold(None, 3, 4, 1.0, C.c_void_p(o.ctypes.data)) == INVALID
    assert L.mrt_radiance_fold(C.c_void_p(rad.ctypes.data), 3, 4, 1.0, None) == INVALID
    assert L.mrt_radiance_fold(C.c_void_p(rad.ctypes.data), 3, 0, 1.0, C.c_void_p(o.ctypes.data)) == INVALID
    assert L.mrt_radiance_fold(None, 0, 4, 1.0, None) == 0


# ---------------------------------------------------------------- 4. records
def test_direction_length_does_not_matter(mrt):
    """d scaled by 3 and by 2^-20 where the normalised direction is the same bits: axis-aligned d
    (3 / sqrt(9) == 1, 2^-20 / sqrt(2^-40) == 1)."""
    _, _, _, _, probes = stream_case(mrt, 5)
    r = cpu_renderer(mrt, 5)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=F32)
    p = probes.copy()
    p["o"] = (278, 278, 278)  # inside the Cornell box
    p["d"] = axes[np.arange(len(p)) % 6]
    base = words(r.trace_rays(p, 16)[0])
    assert len(np.unique(base[:, 3])) > 2 and base[:, :3].any()
    for scale in (3.0, 2.0 ** -20):
        q = p.copy()
        q["d"] = p["d"] * F32(scale)
        assert np.array_equal(words(r.trace_rays(q, 16)[0]), base), scale


def test_inside_flag_is_zero_or_one(mrt):
    """inside = 7 equals inside = 1 (scene 0: glass spheres), and the flag is read: it changes paths."""
    _, _, g, _, probes = stream_case(mrt, 0)
    r = cpu_renderer(mrt, 0)
    one, seven = probes.copy(), probes.copy()
    one["inside"], seven["inside"] = 1, 7
    a = words(r.trace_rays(one, g["depth"])[0])
    assert np.array_equal(words(r.trace_rays(seven, g["depth"])[0]), a)
    assert not np.array_equal(a, words(cpu_stream_records(mrt, 0)[0]))


def py_splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_pcg32_srandom(initstate, initseq):
    mult = 6364136223846793005
    inc = ((initseq << 1) | 1) & M64
    state = (0 * mult + inc) & M64
    state = (state + initstate) & M64
    state = (state * mult + inc) & M64
    return state, inc


def test_streams(mrt):
    for seed, pid in ((0, 0), (mrt.MAIN_SEED, 1), (mrt.MAIN_SEED, 2 ** 40 + 12345), (M64, M64), (123, 2 ** 63)):
        assert mrt.probe_seed(seed, pid) == py_pcg32_srandom(py_splitmix64(seed ^ pid), pid), (seed, pid)
    # two probes that differ only in rng_state differ; an even rng_inc is used as given
    _, _, g, _, probes = stream_case(mrt, 5)
    r = cpu_renderer(mrt, 5)
    base = words(cpu_stream_records(mrt, 5)[0])
    other = probes.copy()
    other["rng_state"] += np.uint64(1)
    assert (words(r.trace_rays(other, g["depth"])[0]) != base).any(axis=1).sum() > 64
    even = probes.copy()
    even["rng_inc"] &= np.uint64(M64 - 1)
    a = words(r.trace_rays(even, g["depth"])[0])
    assert np.array_equal(a, words(r.trace_rays(even, g["depth"])[0])) and (a != base).any()


@pytest.mark.parametrize("sid", [6, 7])
def test_split_batch_equals_the_whole(mrt, sid):
    _, _, g, _, probes = stream_case(mrt, sid)
    r = cpu_renderer(mrt, sid)
    full, total = cpu_stream_records(mrt, sid)
    for k in (1, 63, 64, 255):
        (a, ra), (b, rb) = r.trace_rays(probes[:k], g["depth"]), r.trace_rays(probes[k:], g["depth"])
        assert np.array_equal(words(np.concatenate([a, b])), words(full)) and ra + rb == total, k


@pytest.mark.parametrize("key", EDGE_KEYS)
def test_edge_and_non_finite_probes_return(mrt, key):
    """Edge-operand and non-finite rays as probes: the call returns, no path runs more than
    max_bounces + 1 segments, and a second run gives the same bytes."""
    sc, probes = edge_case(mrt, key)
    assert 1024 < len(probes) <= 4096
    assert not np.isfinite(probes["o"]).all() and not np.isfinite(probes["d"]).all()
    rad = cpu_edge_records(mrt, key)
    assert (rad["rays"] >= 1).all() and (rad["rays"] <= EDGE_DEPTH + 1).all() and rad["rays"].max() > 2
    r = mrt.Renderer(sc, "cpu")
    again, total = r.trace_rays(probes, EDGE_DEPTH)
    r.close()
    assert again.tobytes() == rad.tobytes() and total == int(rad["rays"].sum())


# ---------------------------------------------------------------- 5. arguments
def test_argument_checks(mrt):
    sc, d, g, _, probes = stream_case(mrt, 5)
    r = cpu_renderer(mrt, 5)
    L = mrt.lib()
    out = np.zeros(4, dtype=mrt.RADIANCE_DTYPE)
    pp, op = C.c_void_p(probes.ctypes.data), C.c_void_p(out.ctypes.data)
    assert L.mrt_trace_rays(None, pp, 4, 8, op, None) == INVALID
    assert L.mrt_trace_rays(r._h, None, 4, 8, op, None) == INVALID
    assert L.mrt_trace_rays(r._h, pp, 4, 8, None, None) == INVALID
    # rays_out may be NULL
    assert L.mrt_trace_rays(r._h, pp, 4, 8, op, None) == 0 and out["rays"].all()
    # n == 0: nothing touched (null pointers are fine)
    assert L.mrt_trace_rays(r._h, None, 0, 8, None, None) == 0
    rad, total = r.trace_rays(probes[:0])
    assert len(rad) == 0 and rad.dtype == mrt.RADIANCE_DTYPE and total == 0
    with pytest.raises(ValueError):
        r.trace_rays(np.zeros((3, 12), F32))
    # the device forms on a CPU-backend scene
    full, least = C.c_uint64(), C.c_uint64()
    assert L.mrt_trace_rays_workspace(r._h, 8, C.byref(full), C.byref(least)) == INVALID
    assert L.mrt_trace_rays_device(r._h, pp, 4, 8, op, pp, 1 << 20, None) == INVALID
    with pytest.raises(mrt.MrtError):
        r.trace_rays_workspace(8)
    with pytest.raises(mrt.MrtError):
        r.trace_rays_device(probes.ctypes.data, 4, out.ctypes.data, probes.ctypes.data, 1 << 20, 8)
    # mrt_camera_path_probe / mrt_pano_probe: null, a zero size, pixel or sample out of range
    cam, cp = sc.view.camera, sc.camera_params()
    one = np.zeros(1, dtype=mrt.PROBE_DTYPE)
    q = C.c_void_p(one.ctypes.data)
    ns = d.sqrt_samples ** 2
    for fn, first in ((L.mrt_camera_path_probe, cam), (L.mrt_pano_probe, cp)):
        assert fn(C.byref(first), C.byref(d), 0, 0, q) == 0
        assert fn(None, C.byref(d), 0, 0, q) == INVALID
        assert fn(C.byref(first), None, 0, 0, q) == INVALID
        assert fn(C.byref(first), C.byref(d), 0, 0, None) == INVALID
        assert fn(C.byref(first), C.byref(d), d.width * d.height, 0, q) == INVALID
        assert fn(C.byref(first), C.byref(d), 0, ns, q) == INVALID
        assert fn(C.byref(first), C.byref(d), d.width * d.height - 1, ns - 1, q) == 0
        for field in ("width", "height", "sqrt_samples"):
            z = mrt.render_desc(d.width, d.height, ns)
            setattr(z, field, 0)
            assert fn(C.byref(first), C.byref(z), 0, 0, q) == INVALID, field
    with pytest.raises(mrt.MrtError):
        mrt.camera_path_probes(cam, d, [d.width * d.height], [0])
    flat = mrt.make_camera(cp)
    bad = mrt._lib.MrtCameraParams()
    C.memmove(C.byref(bad), C.byref(cp), C.sizeof(bad))
    bad.lookat[:] = list(bad.pos)  # a degenerate frame
    assert L.mrt_pano_probe(C.byref(bad), C.byref(d), 0, 0, q) == INVALID
    del flat


# ---------------------------------------------------------------- 6. panorama
def pano_params(mrt, pos, lookat, up):
    p = mrt._lib.MrtCameraParams()
    p.pos[:], p.lookat[:], p.up[:] = pos, lookat, up
    p.vfov_deg, p.aspect, p.aperture, p.focus_dist, p.time0, p.time1 = 40.0, 1.0, 0.0, 1.0, 0.0, 1.0
    return p


@pytest.mark.parametrize("pos,lookat,up", [((0, 0, 0), (0, 0, -1), (0, 1, 0)), ((278, 278, -800), (278, 278, 0), (0, 1, 0)),
                                           ((3, 2, 1), (1, 2.5, -4), (0.2, 1, 0.1))])
def test_pano_directions(mrt, pos, lookat, up):
    """The centre of the image looks along the view direction, the top row up (the frame's v: `up`
    itself when up is perpendicular to the view), every direction has length 1 -- all within 1e-6.  The
    top row's direction is pi * 0.5 / H from the pole, so the pole is checked on a 1 x 2^21 image."""
    p = pano_params(mrt, pos, lookat, up)
    w = np.array(pos, dtype=np.float64) - np.array(lookat, dtype=np.float64)
    w /= np.linalg.norm(w)
    u = np.cross(np.array(up, dtype=np.float64), w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    if abs(np.dot(up, w)) < 1e-12:
        assert np.allclose(v, np.array(up) / np.linalg.norm(up), atol=1e-12)
    # centre: odd sizes, one sample per pixel (offset 0.5): s = t = 0.5 exactly
    d = mrt.render_desc(33, 17, 1)
    q = mrt.pano_probes(p, d, [16 + 8 * 33], [0])
    assert np.abs(q["d"][0].astype(np.float64) + w).max() <= 1e-6
    assert np.array_equal(bits(q["o"][0]), bits(np.array(pos, dtype=F32))) and q["inside"][0] == 0
    # the pole
    H = 2 ** 21
    d = mrt.render_desc(1, H, 1)
    q = mrt.pano_probes(p, d, [H - 1, 0], [0, 0])
    assert np.abs(q["d"][0].astype(np.float64) - v).max() <= 1e-6
    assert np.abs(q["d"][1].astype(np.float64) + v).max() <= 1e-6
    # every direction of a frame: unit length, and the direction the formula names (float64 restatement)
    W, H, spp = 37, 23, 4
    d = mrt.render_desc(W, H, spp)
    px, sm = np.divmod(np.arange(W * H * spp), spp)
    q = mrt.pano_probes(p, d, px, sm)
    dirs = q["d"].astype(np.float64)
    assert np.abs(np.linalg.norm(dirs, axis=1) - 1).max() <= 1e-6
    sq = d.sqrt_samples
    s = ((px % W) + ((sm // sq) + 0.5) / sq) / W
    t = ((px // W) + ((sm % sq) + 0.5) / sq) / H
    phi, th = (s - 0.5) * 2 * np.pi, (t - 0.5) * np.pi
    want = (np.cos(th) * np.sin(phi))[:, None] * u + np.sin(th)[:, None] * v - (np.cos(th) * np.cos(phi))[:, None] * w
    assert np.abs(dirs - want).max() <= 2e-6
    # the stream: keyed like the render's path, one draw (the time) taken
    k = W * H * spp - 1
    state, inc = mrt.probe_seed(d.seed, k)
    assert int(q["rng_inc"][k]) == inc and int(q["rng_state"][k]) == (state * 6364136223846793005 + inc) & M64
    assert (q["time"] >= 0).all() and (q["time"] < 1).all() and len(np.unique(q["time"])) > len(q) // 2


EXE = os.path.join(ROOT, "bin", "mrt")


def test_cli_pano_equals_python_composition(mrt, tmp_path):
    """bin/mrt -backend cpu -pano at 32 x 16 x 4 writes the image Python composes from pano_probes ->
    trace_rays -> radiance_fold; -aperture is ignored; -gpus 2 is refused."""
    W, H, spp = 32, 16, 4
    base = [EXE, "-backend", "cpu", "-order", "path", "-scene", 5, "-width", W, "-height", H, "-samples", spp, "-pano"]
    run = lambda extra, **kw: subprocess.run([str(a) for a in base + extra], capture_output=True, text=True, timeout=120, **kw)
    a, b = tmp_path / "a.pfm", tmp_path / "b.pfm"
    out = run(["-o", a], check=True).stdout
    sc = mrt.select_scene(5, W / H)
    d = mrt.render_desc(W, H, spp)
    px, sm = np.divmod(np.arange(W * H * spp), spp)
    r = mrt.Renderer(sc, "cpu")
    rad, total = r.trace_rays(mrt.pano_probes(sc.camera_params(), d, px, sm), 32)
    r.close()
    img = mrt.radiance_fold(rad, spp, 1000.0).reshape(H, W, 4)
    assert np.array_equal(bits(mrt.read_pfm(str(a))), bits(img[..., :3])) and img[..., :3].any()
    assert f"rays {total}\n" in out and "exact numerics" in out
    run(["-aperture", 25, "-o", b], check=True)
    assert a.read_bytes() == b.read_bytes()
    refused = run(["-gpus", 2])
    assert refused.returncode != 0 and "-pano" in refused.stderr
