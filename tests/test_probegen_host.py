"""The probe generators (include/mrt.h "probe generators", mrt_camera_pixel_rays) without a GPU: the
range forms against the per-record functions (which test_probe_host.py and test_cast_host.py pin to
the reference), byte for byte; the argument rules; the surface probes against a float64 restatement of
the header's formulas and their statistical properties; the host pipelines on the CPU backend; and
bin/mrt -pano with -backend cpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_probe_host import bits, stream_case

INVALID = 1
M64 = 2 ** 64 - 1
W, H, SPP = 24, 16, 4  # 1536 paths
NPATH = W * H * SPP
# (first, n): the whole range; first not a multiple of ns with n in {1, 63, 65, 1000}; the range that ends at the top
PROBE_RANGES = [(0, NPATH), (5, 1), (7, 63), (101, 65), (331, 1000), (NPATH - 65, 65)]
RAY_RANGES = [(0, W * H), (5, 1), (7, 63), (101, 65), (W * H - 65, 65)]


def camera(mrt, sid):
    return stream_case(mrt, sid)[0].view.camera


def desc(mrt, **kw):
    return mrt.render_desc(W, H, SPP, **kw)


_oracle = {}


def per_record(mrt, sid):
    """(camera probes, panorama probes, pixel rays) of the whole 24 x 16 x 4 render of scene sid's
    camera from the per-record functions (computed once)."""
    if sid not in _oracle:
        sc = stream_case(mrt, sid)[0]
        d = desc(mrt)
        px, sm = np.divmod(np.arange(NPATH), SPP)
        pix = np.arange(W * H)
        _oracle[sid] = (mrt.camera_path_probes(sc.view.camera, d, px, sm), mrt.pano_probes(sc.camera_params(), d, px, sm),
                        mrt.camera_pixel_rays(sc.view.camera, W, H, pix % W, pix // W))
    return _oracle[sid]


# ---------------------------------------------------------------- 1. ranges against the per-record functions
@pytest.mark.parametrize("sid", range(10))
def test_ranges_equal_the_per_record_functions(mrt, sid):
    sc = stream_case(mrt, sid)[0]
    cam, cp, d = sc.view.camera, sc.camera_params(), desc(mrt)
    want_cam, want_pano, want_rays = per_record(mrt, sid)
    if sid in (0, 1):
        assert cam.lens_radius > 0  # a lens: the disk's rejection loop runs (every other camera is a pinhole)
    for first, n in PROBE_RANGES:
        assert mrt.camera_path_probe_range(cam, d, first, n).tobytes() == want_cam[first:first + n].tobytes(), (first, n)
        assert mrt.pano_probe_range(cp, d, first, n).tobytes() == want_pano[first:first + n].tobytes(), (first, n)
    for first, n in RAY_RANGES:
        assert mrt.camera_pixel_ray_range(cam, W, H, first, n).tobytes() == want_rays[first:first + n].tobytes(), (first, n)


# ---------------------------------------------------------------- 2. arguments
def test_argument_rules(mrt):
    L = mrt._lib.lib()
    sc = stream_case(mrt, 5)[0]
    cam, cp, d = sc.view.camera, sc.camera_params(), desc(mrt)
    out = np.zeros(8, dtype=mrt.PROBE_DTYPE)
    rays = np.zeros(8, dtype=mrt.RAY_DTYPE)
    o, ro = C.c_void_p(out.ctypes.data), C.c_void_p(rays.ctypes.data)
    for fn, first in ((L.mrt_camera_path_probes, cam), (L.mrt_pano_probes, cp)):
        assert fn(C.byref(first), C.byref(d), NPATH - 4, 4, o) == 0
        assert fn(C.byref(first), C.byref(d), NPATH - 4, 5, o) == INVALID  # one past the top
        assert fn(C.byref(first), C.byref(d), NPATH, 1, o) == INVALID
        assert fn(C.byref(first), C.byref(d), M64, 2, o) == INVALID  # first + n wraps
        assert fn(None, C.byref(d), 0, 1, o) == INVALID
        assert fn(C.byref(first), None, 0, 1, o) == INVALID
        assert fn(C.byref(first), C.byref(d), 0, 1, None) == INVALID
        for field in ("width", "height", "sqrt_samples"):
            z = desc(mrt)
            setattr(z, field, 0)
            assert fn(C.byref(first), C.byref(z), 0, 1, o) == INVALID, field
        assert fn(None, None, 0, 0, None) == 0  # n == 0: nothing is read
    bad = sc.camera_params()
    bad.lookat[:] = bad.pos[:]
    assert L.mrt_pano_probes(C.byref(bad), C.byref(d), 0, 1, o) == INVALID  # a degenerate frame
    assert L.mrt_camera_pixel_rays(C.byref(cam), W, H, W * H - 4, 4, ro) == 0
    assert L.mrt_camera_pixel_rays(C.byref(cam), W, H, W * H - 4, 5, ro) == INVALID
    assert L.mrt_camera_pixel_rays(C.byref(cam), W, H, M64, 2, ro) == INVALID
    assert L.mrt_camera_pixel_rays(None, W, H, 0, 1, ro) == INVALID
    assert L.mrt_camera_pixel_rays(C.byref(cam), W, H, 0, 1, None) == INVALID
    assert L.mrt_camera_pixel_rays(C.byref(cam), 0, H, 0, 1, ro) == INVALID
    assert L.mrt_camera_pixel_rays(C.byref(cam), W, 0, 0, 1, ro) == INVALID
    assert L.mrt_camera_pixel_rays(None, 0, 0, 0, 0, None) == 0
    hits = np.zeros(4, dtype=mrt.HIT_DTYPE)
    h = C.c_void_p(hits.ctypes.data)
    big = np.zeros(64, dtype=mrt.PROBE_DTYPE)
    b = C.c_void_p(big.ctypes.data)
    assert L.mrt_surface_probes(h, None, 4, 2, 0, 0, b) == 0
    assert L.mrt_surface_probes(h, None, 4, 0, 0, 0, b) == INVALID  # sqrt_per_hit = 0
    assert L.mrt_surface_probes(None, None, 4, 1, 0, 0, b) == INVALID
    assert L.mrt_surface_probes(h, None, 4, 1, 0, 0, None) == INVALID
    # n_hits * P >= 2^32 is refused before anything is read or written
    assert L.mrt_surface_probes(h, None, 1 << 28, 4, 0, 0, b) == INVALID
    assert L.mrt_surface_probes(h, None, 1, 1 << 16, 0, 0, b) == INVALID
    assert L.mrt_surface_probes(h, None, 4, 0xFFFFFFFF, 0, 0, b) == INVALID
    assert L.mrt_surface_probes(None, None, 0, 0, 0, 0, None) == 0  # n_hits == 0
    with pytest.raises(mrt.MrtError):
        mrt.surface_probes(hits, sqrt_per_hit=0)
    with pytest.raises(ValueError):
        mrt.surface_probes(hits, rays=np.zeros(3, dtype=mrt.RAY_DTYPE))


# ---------------------------------------------------------------- 3. surface probes: the formulas
U = 2.0 ** -24  # float32 unit roundoff: a correctly rounded result of magnitude <= 1 is within U of the exact one
PCG_MULT = 6364136223846793005
PCG_MULT_INV = pow(PCG_MULT, -1, 2 ** 64)
TWO_PI_F = float(np.float32(2.0) * np.float32(3.14159265358979323846))


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def hit_records(mrt, rng, n, misses=()):
    hits = np.zeros(n, dtype=mrt.HIT_DTYPE)
    hits["t"] = rng.uniform(0.5, 9.0, n).astype(np.float32)
    hits["p"] = rng.uniform(-50.0, 50.0, (n, 3)).astype(np.float32)
    hits["n"] = unit_normals(rng, n)
    hits["mat"] = rng.integers(0, 7, n)
    for i in misses:
        hits[i] = (np.inf, (0, 0, 0), (0, 0, 0), mrt.NO_HIT)
    return hits


def stream_draws(mrt, seed, first_id, n):
    """(u1, u2, state, inc) of the streams keyed by first_id + j, j < n, as float32 / uint64 arrays: the
    words of n sqrt_per_hit = 1 records of misses (a miss takes the two draws as well), stepped back
    twice through the PCG32 recurrence to the seeded state, then randf restated."""
    miss = np.zeros(n, dtype=mrt.HIT_DTYPE)
    miss["t"], miss["mat"] = np.inf, mrt.NO_HIT
    rec = mrt.surface_probes(miss, sqrt_per_hit=1, seed=seed, first_id=first_id)
    state2, inc = rec["rng_state"].copy(), rec["rng_inc"].copy()
    with np.errstate(over="ignore"):
        inv = np.uint64(PCG_MULT_INV)
        state1 = (state2 - inc) * inv
        state0 = (state1 - inc) * inv

        def randf(old):
            xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
            rot = (old >> np.uint64(59)).astype(np.uint32)
            out = (xs >> rot) | (xs << ((np.uint32(0) - rot) & np.uint32(31)))
            return (np.uint32(0x3F800000) | (out & np.uint32(0x007FFFFF))).view(np.float32) - np.float32(1.0)

        u1, u2 = randf(state0), randf(state1)
    return u1, u2, state0, inc, state2


def onb64(w):
    """onb(n) (onb.h:19-24) in float64: rows U, V of the basis (U, V, w)."""
    a = np.where((np.abs(w[:, 0]) > np.float32(0.9))[:, None], [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    v = np.cross(w, a)
    v /= np.linalg.norm(v, axis=1)[:, None]
    return np.cross(w, v), v


def restated(w, u1, u2, k, sq):
    """The header's formulas in float64 from the float32 draws: (direction, its error bound) per record.

    The bound counts float32 roundings on values of magnitude <= 1 (U each, absolute):
      r1, r2    the sum (float)a + u and the quotient: 2 U each
      1 - r2    r2's error and the difference's rounding: 3 U
      z, s      a root's error for a radicand off by e is min(sqrt(e), e / (2 root)); one more U for its own rounding
      phi       2 pi times r1's 2 U, and its own rounding at magnitude <= 2 pi: 6 pi U < 19 U
      sin, cos  the argument's 19 U and include/mrt_mathfn.h's error (correctly rounded but for ~1e-8
                of arguments, so within 1.5 ulp of a value <= 1: 2 U): 21 U
      vec.x, y  cos * s: 21 U + e_s + the product's U
      onb       cross(w, a) with an axis a is exact products and one difference per component (U); its
                length is >= sqrt(1 - 0.81) > 0.43, so after the dot (5 U relative), the root (U) and the
                quotient (U) V is within U / 0.43 + 7 U < 10 U; U = cross(w, V): two products of V's error,
                two product roundings, one difference: 23 U
      d         per component three products and two sums of magnitude < 2: 3 U + 4 U, plus the operands'
                errors: 2 (22 U + e_s) + e_z + 23 U + 10 U
    in all 84 U + 2 e_s + e_z; second-order terms are below U^2 * 100 and covered by the roundings up."""
    a, b = k // sq, k % sq
    r1 = (a + u1.astype(np.float64)) / sq
    r2 = (b + u2.astype(np.float64)) / sq
    z, s = np.sqrt(np.maximum(1.0 - r2, 0.0)), np.sqrt(r2)
    phi = TWO_PI_F * r1
    vec = np.stack([np.cos(phi) * s, np.sin(phi) * s, z], axis=1)
    bu, bv = onb64(w.astype(np.float64))
    d = vec[:, 0:1] * bu + vec[:, 1:2] * bv + vec[:, 2:3] * w.astype(np.float64)
    tiny = 1e-300
    e_z = np.minimum(np.sqrt(3 * U), 3 * U / (2 * np.maximum(z, tiny))) + U
    e_s = np.minimum(np.sqrt(2 * U), 2 * U / (2 * np.maximum(s, tiny))) + U
    return d, 84 * U + 2 * e_s + e_z, r1, r2


def test_surface_probes_equal_the_restated_formulas(mrt):
    rng = np.random.default_rng(41)
    n, sq, seed, first_id = 257, 3, 0x1234567890ABCDEF, M64 - 1000  # the ids wrap past 2^64
    P = sq * sq
    hits = hit_records(mrt, rng, n)
    rays = np.zeros(n, dtype=mrt.RAY_DTYPE)
    rays["d"] = unit_normals(rng, n) * rng.uniform(0.5, 3.0, (n, 1)).astype(np.float32)
    rays["time"] = rng.uniform(0, 1, n).astype(np.float32)
    u1, u2, state0, inc, state2 = stream_draws(mrt, seed, first_id, n * P)
    for j in (0, 1, 999, 1000, 1001, n * P - 1):  # the stepped-back state is the seeded state
        assert mrt.probe_seed(seed, (first_id + j) & M64) == (int(state0[j]), int(inc[j]))
    k = np.arange(n * P) % P
    i = np.arange(n * P) // P
    for with_rays in (False, True):
        got = mrt.surface_probes(hits, rays if with_rays else None, sqrt_per_hit=sq, seed=seed, first_id=first_id)
        w = hits["n"][i].astype(np.float64)
        if with_rays:
            turn = np.einsum("ij,ij->i", hits["n"].astype(np.float64), rays["d"].astype(np.float64))[i] > 0
            assert 0.3 < turn.mean() < 0.7
            w = np.where(turn[:, None], -w, w)
        want, bound, _, _ = restated(w.astype(np.float32), u1, u2, k, sq)
        err = np.abs(got["d"].astype(np.float64) - want).max(axis=1)
        print("surface probes: max error", err.max(), "smallest bound", bound.min(), "largest error / bound", (err / bound).max())
        assert (err <= bound).all()
        assert bound.max() < 1e-3 and np.median(bound) < 1e-5
        assert np.array_equal(bits(got["o"]), bits(hits["p"][i]))
        assert np.array_equal(bits(got["time"]), bits(rays["time"][i] if with_rays else np.zeros(n * P, np.float32)))
        assert np.array_equal(got["rng_state"], state2) and np.array_equal(got["rng_inc"], inc)
        assert not got["inside"].any()


_props = {}


def property_batch(mrt):
    """4096 hits with random unit normals, sqrt_per_hit 4: (hits, the 65 536 records, u1, u2), once."""
    if not _props:
        rng = np.random.default_rng(42)
        hits = hit_records(mrt, rng, 4096)
        got = mrt.surface_probes(hits, sqrt_per_hit=4, seed=99, first_id=0)
        u1, u2, _, _, _ = stream_draws(mrt, 99, 0, len(got))
        _props["v"] = (hits, got, u1, u2)
    return _props["v"]


def test_surface_probes_are_cosine_weighted_unit_directions(mrt):
    hits, got, _, _ = property_batch(mrt)
    assert len(got) == 65536
    w = np.repeat(hits["n"].astype(np.float64), 16, axis=0)
    d = got["d"].astype(np.float64)
    cos = np.einsum("ij,ij->i", d, w)
    assert (cos >= 0).all()
    assert (np.abs(np.linalg.norm(d, axis=1) - 1) < 1e-5).all()
    print("mean cosine", cos.mean())
    assert abs(cos.mean() - 2 / 3) < 0.005  # cosine-weighted: 2/3 (the reference's factor-2 form: 0.472)


def test_surface_probes_fill_every_stratum_once_per_hit(mrt):
    """(a, b) from each record's direction through the inverse of the formulas: the local coordinates
    in onb(w), r2 = 1 - z^2 and r1 = atan2(y, x) / 2 pi, a = r1 sq - u1, b = r2 sq - u2."""
    hits, got, u1, u2 = property_batch(mrt)
    sq = 4
    w = np.repeat(hits["n"].astype(np.float64), 16, axis=0)
    bu, bv = onb64(w)
    d = got["d"].astype(np.float64)
    x, y, z = (np.einsum("ij,ij->i", d, e) for e in (bu, bv, w))
    r2 = 1 - z * z
    r1 = np.mod(np.arctan2(y, x), 2 * np.pi) / (2 * np.pi)
    fa, fb = r1 * sq - u1, r2 * sq - u2
    fa = np.where(fa < -0.5, fa + sq, fa)  # (phi = 2 pi - epsilon read back as just below 0)
    a, b = np.rint(fa).astype(np.int64), np.rint(fb).astype(np.int64)
    assert np.abs(fa - a).max() < 1e-3 and np.abs(fb - b).max() < 1e-3
    assert np.array_equal(a * sq + b, np.arange(len(got)) % 16)  # stratum k of every hit, each once


# ---------------------------------------------------------------- 4. further surface probe cases
def test_surface_probe_normal_faces_the_ray(mrt):
    rng = np.random.default_rng(43)
    hits = hit_records(mrt, rng, 64)
    rays = np.zeros(64, dtype=mrt.RAY_DTYPE)
    rays["d"] = hits["n"] * np.float32(2.5)  # dot(n, d) > 0: the normal is turned
    flipped = hits.copy()
    flipped["n"] = -hits["n"]
    a = mrt.surface_probes(hits, rays, sqrt_per_hit=2, seed=5)
    assert a.tobytes() == mrt.surface_probes(flipped, None, sqrt_per_hit=2, seed=5).tobytes()
    assert (np.einsum("ij,ij->i", a["d"], np.repeat(hits["n"], 4, axis=0)) <= 0).all()
    rays["d"] = -hits["n"]  # dot < 0: as it stands
    assert mrt.surface_probes(hits, rays, sqrt_per_hit=2, seed=5).tobytes() == mrt.surface_probes(hits, None, sqrt_per_hit=2, seed=5).tobytes()
    rays["d"] = np.nan  # a NaN dot does not turn the normal
    assert mrt.surface_probes(hits, rays, sqrt_per_hit=2, seed=5).tobytes() == mrt.surface_probes(hits, None, sqrt_per_hit=2, seed=5).tobytes()


def test_surface_probe_of_a_miss_is_the_null_record(mrt):
    rng = np.random.default_rng(44)
    hits = hit_records(mrt, rng, 33)
    missed = hit_records(mrt, np.random.default_rng(44), 33, misses=(0, 7, 32))
    rays = np.zeros(33, dtype=mrt.RAY_DTYPE)
    rays["d"], rays["time"] = (0, 0, 1), 0.25
    a = mrt.surface_probes(hits, rays, sqrt_per_hit=3, seed=6, first_id=17)
    b = mrt.surface_probes(missed, rays, sqrt_per_hit=3, seed=6, first_id=17)
    miss = np.repeat(missed["mat"] == mrt.NO_HIT, 9)
    assert miss.sum() == 27
    assert a[~miss].tobytes() == b[~miss].tobytes()
    for f in ("o", "d", "time", "inside"):
        assert not bits(b[f][miss]).any(), f
    assert np.array_equal(b["rng_state"], a["rng_state"]) and np.array_equal(b["rng_inc"], a["rng_inc"])


def test_surface_probe_batch_cut_in_two_is_the_whole(mrt):
    rng = np.random.default_rng(45)
    hits = hit_records(mrt, rng, 100, misses=(3,))
    rays = np.zeros(100, dtype=mrt.RAY_DTYPE)
    rays["d"], rays["time"] = unit_normals(rng, 100), rng.uniform(0, 1, 100).astype(np.float32)
    whole = mrt.surface_probes(hits, rays, sqrt_per_hit=3, seed=7, first_id=M64 - 50)
    cut = 37
    parts = [mrt.surface_probes(hits[:cut], rays[:cut], sqrt_per_hit=3, seed=7, first_id=M64 - 50),
             mrt.surface_probes(hits[cut:], rays[cut:], sqrt_per_hit=3, seed=7, first_id=M64 - 50 + cut * 9)]
    assert np.concatenate(parts).tobytes() == whole.tobytes()


# ---------------------------------------------------------------- 5. pipelines on the CPU backend
@pytest.mark.parametrize("sid", [5, 7])
def test_fold_of_the_camera_range_is_the_render(mrt, sid):
    sc = stream_case(mrt, sid)[0]
    d = desc(mrt, depth=16)
    r = mrt.Renderer(sc, "cpu")
    cam = mrt.make_camera(sc.camera_params(), aspect=W / H)
    r.set_camera(cam)
    img, rays = r.render(d)
    rad, total = r.trace_rays(mrt.camera_path_probe_range(cam, d, 0, NPATH), 16)
    r.close()
    assert np.array_equal(bits(mrt.radiance_fold(rad, SPP, d.max_luminance)), bits(img.reshape(-1, 4)))
    assert total == rays and img[..., :3].any()


PIPE_SQ, PIPE_DEPTH = 2, 8
_pipe = {}


def surface_pipeline(mrt, sid):
    """pixel rays -> cast -> surface probes -> trace -> fold on the CPU backend for a 24 x 16 frame of
    scene sid: (rays, hits, probes, radiance records, folded float4s).  Computed once, then shared
    (test_probegen_gpu.py compares the device chain against it)."""
    if sid not in _pipe:
        _pipe[sid] = run_surface_pipeline(mrt, sid)
    return _pipe[sid]


def run_surface_pipeline(mrt, sid):
    sc = stream_case(mrt, sid)[0]
    cam = mrt.make_camera(sc.camera_params(), aspect=W / H)
    r = mrt.Renderer(sc, "cpu")
    rays = mrt.camera_pixel_ray_range(cam, W, H, 0, W * H)
    hits = r.cast_rays(rays, seed=3)
    probes = mrt.surface_probes(hits, rays, sqrt_per_hit=PIPE_SQ, seed=11, first_id=0)
    rad, _ = r.trace_rays(probes, PIPE_DEPTH)
    r.close()
    return rays, hits, probes, rad, mrt.radiance_fold(rad, PIPE_SQ * PIPE_SQ, 1000.0)


def pano_pipeline(mrt, sid):
    if ("pano", sid) not in _pipe:
        sc = stream_case(mrt, sid)[0]
        d = desc(mrt, depth=PIPE_DEPTH)
        r = mrt.Renderer(sc, "cpu")
        probes = mrt.pano_probe_range(sc.camera_params(), d, 0, NPATH)
        rad, _ = r.trace_rays(probes, PIPE_DEPTH)
        r.close()
        _pipe[("pano", sid)] = (probes, rad, mrt.radiance_fold(rad, SPP, d.max_luminance))
    return _pipe[("pano", sid)]


@pytest.mark.parametrize("sid", [5, 7])
def test_surface_pipeline_is_deterministic(mrt, sid):
    rays, hits, probes, rad, rgb = surface_pipeline(mrt, sid)
    again = run_surface_pipeline(mrt, sid)
    for a, b in zip((rays, hits, probes, rad, rgb), again):
        assert a.tobytes() == b.tobytes()
    miss = np.repeat(hits["mat"] == mrt.NO_HIT, PIPE_SQ * PIPE_SQ)
    assert (~miss).any() and rgb[:, :3].any()
    if sid == 7:
        assert miss.any()  # book2's frame shows the background
    for f in ("o", "d", "time", "inside"):  # a missed pixel's records are the null record
        assert not bits(probes[f][miss]).any(), f


# ---------------------------------------------------------------- 6. the command line
EXE = os.path.join(ROOT, "bin", "mrt")


def test_cli_pano_on_the_cpu_backend_equals_the_range_chain(mrt, tmp_path):
    Wc, Hc, spp = 32, 16, 4
    a = tmp_path / "a.pfm"
    cmd = [EXE, "-backend", "cpu", "-order", "path", "-scene", 5, "-width", Wc, "-height", Hc, "-samples", spp, "-pano", "-o", a]
    out = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=120, check=True).stdout
    sc = mrt.select_scene(5, Wc / Hc)
    d = mrt.render_desc(Wc, Hc, spp)
    r = mrt.Renderer(sc, "cpu")
    rad, total = r.trace_rays(mrt.pano_probe_range(sc.camera_params(), d, 0, Wc * Hc * spp), 32)
    r.close()
    img = mrt.radiance_fold(rad, spp, 1000.0).reshape(Hc, Wc, 4)
    assert np.array_equal(bits(mrt.read_pfm(str(a))), bits(img[..., :3])) and img[..., :3].any()
    assert f"rays {total}\n" in out
