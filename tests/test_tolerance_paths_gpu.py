"""The tolerance contract (-numerics fast), path by path.

Image statistics (RMSE, means, ray totals) and digests of the parent's bits miss a subtle fault -- a
wrong throughput factor in one material branch, a dropped level, a retrace that writes the wrong
slot change well under 1 % of a 64-spp image's energy.  Three checks here do not:

path-exact build (pex)   exact arithmetic + forward fold (Makefile PEXFLAGS): geometry, draws and ray
                         counts are the exact contract's and only the fold differs, so it must equal
                         the C restatement's forward fold (oracle.desc(fold=1), checked against the
                         pinned fold by test_oracle_forward.py) BIT FOR BIT per path, per pixel and
                         in its ray total.  Scenes 6, 7, 8, their other walks, edge sizes, mode 1.
fast arithmetic (fastz)  against the exact contract on the same renderer: one-ray paths carry no
                         arithmetic of the fold and are bit-equal, no channel is negative, and the
                         share of diverged paths (tools/divergence.py's definition) stays within
                         twice the project's recorded share (profiles/r04_divergence.jsonl, tag intree).
hand-over                every pixel the retrace kernel changed is explained by substituting the
                         forward restatement's radiance for a few of its samples.

Measured shares: profiles/tolerance_paths.jsonl (the tests print one `tolerance_paths {json}` line per case)."""
import itertools
import json

import numpy as np
import pytest

from test_synthetic_scenes import bits, gpu_paths, launch_size

pytestmark = pytest.mark.gpu

GEN, NOSIG, NOBVHW = "MRT_FORCE_GENERIC", "MRT_NO_SIG", "MRT_NO_BVHW"
# Which build a walk of a reference scene runs under the tolerance contract, from mrt_launch.h kPathExact
# (FT_VOLUME in the KERNEL's features, or the room + mesh shape with metal) and kFtzVariant (the others
# without volumes): the generic machine and the catch-all interpreter are FT_ALL kernels (FT_VOLUME
# compiled in), so scenes 6 and 7 stay path-exact under every hook; scene 8 without its shape id runs
# the FT_LIN | FT_MESH | FT_METAL | FT_BIASED interpreter: no volume, no shape, the fast arithmetic.
BUILD = {(6, None): "pex", (7, None): "pex", (8, None): "pex",
         (6, GEN): "pex", (7, GEN): "pex", (7, NOBVHW): "pex", (8, NOSIG): "fastz",
         (5, None): "fastz", (9, None): "fastz", (5, NOSIG): "fastz",
         (0, None): "fastz", (1, None): "fastz", (2, None): "fastz", (3, None): "fastz", (4, None): "fastz"}
# diverged paths in percent, profiles/r04_divergence.jsonl tag intree (C2 = scene 5, C3 = 9, C4 = 8 under
# the fast arithmetic, before the path-exact build took that scene's shape walk over)
RECORDED_PCT = {5: 0.21333, 9: 0.13414, 8: 0.01543}


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


_scenes, _renderers, _refs = {}, {}, {}


def scene(mrt, sid):
    if sid not in _scenes:
        _scenes[sid] = mrt.select_scene(sid, 1.0)
    return _scenes[sid]


def renderer(mrt, sid, hook, monkeypatch):
    """The scene's renderer under a test hook (read at upload), after one tiny tolerance-contract
    render so that kernel_info() describes that contract's launch; the build is asserted."""
    if (sid, hook) not in _renderers:
        with monkeypatch.context() as mp:
            if hook:
                mp.setenv(hook, "1")
            r = mrt.Renderer(scene(mrt, sid), 0)
        r.render(mrt.render_desc(16, 16, 1, numerics="fast"))
        _renderers[(sid, hook)] = r
    r = _renderers[(sid, hook)]
    assert mrt._lib.BUILDS[r.kernel_info()["build"]] == BUILD[(sid, hook)], (sid, hook, r.kernel_info())
    return r


def forward_ref(mrt, orc, sid, w, h, spp, depth=32, mode=0, paths=True):
    """The forward restatement of a render: computed once, shared, never written to."""
    key = (sid, w, h, spp, depth, mode)
    if key not in _refs:
        _refs[key] = orc.render(scene(mrt, sid), orc.desc(w, h, spp, depth=depth, mode=mode, threads=16, fold=1), paths=paths)
        for a in _refs[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _refs[key]


def same_bits(a, b):
    """assert_exact's rule: a NaN equals a NaN (x86's default NaN is 0xFFC00000, the GPU's 0x7FC00000,
    and the sign of a NaN is no value); every other value by its bits."""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_equals_forward(mrt, r, ref, w, h, spp, what, depth=32, mode=0, tile_size=32):
    oimg, orays, prgb, prays = ref
    d = mrt.render_desc(w, h, spp, depth=depth, mode=mode, tile_size=tile_size, numerics="fast", flags=mrt._lib.RF_PATH_DEBUG)
    img, rays = r.render(d)
    assert mrt._lib.BUILDS[r.kernel_info()["build"]] == "pex", what
    grgb, grays = gpu_paths(mrt, r, d)
    bad_rays = np.nonzero(grays != prays)[0]
    bad = np.nonzero(~same_bits(grgb, prgb).all(axis=1))[0]
    print(f"{what}: {w}x{h}x{d.sqrt_samples ** 2} depth {depth} mode {mode}: rays {rays} vs {orays}, paths with other ray counts "
          f"{bad_rays.size}, with other bits {bad.size} of {len(prays)}")
    assert bad_rays.size == 0, (what, bad_rays[:5], grays[bad_rays[:5]], prays[bad_rays[:5]])
    assert bad.size == 0, (f"{what}: {bad.size} paths differ, first {bad[:5]} (rays {prays[bad[:5]]}): GPU "
                           f"{[hex(x) for x in bits(grgb)[bad[:5]].ravel()]} forward restatement {[hex(x) for x in bits(prgb)[bad[:5]].ravel()]}")
    assert same_bits(img, oimg).all(), what
    assert rays == orays, (what, rays, orays)


def scene_size(mrt, sid, monkeypatch):
    """launch_size of the scene's own tolerance-contract kernel; its other walks render the same size
    (one shared reference)."""
    return launch_size(renderer(mrt, sid, None, monkeypatch).kernel_info())


# ---------------------------------------------------------------- the fast arithmetic against the exact contract
def fast_against_exact(mrt, r, sid, hook, w, h, spp, sky, cap_pct=None):
    """Both contracts on one renderer, per path.  Exact assertions: one-ray paths (no level: T = 1 times
    the light's emission, or black; under a sky only the black ones, the sky's blend is arithmetic) have
    equal bits, no finite channel is negative.  cap_pct: the diverged share's ceiling in percent."""
    out = {}
    for num in ("exact", "fast"):
        d = mrt.render_desc(w, h, spp, numerics=num, flags=mrt._lib.RF_PATH_DEBUG)
        _, total = r.render(d)
        out[num] = gpu_paths(mrt, r, d) + (total,)
    assert mrt._lib.BUILDS[r.kernel_info()["build"]] == "fastz", (sid, hook)
    (a, ar, at), (b, br, bt) = out["exact"], out["fast"]
    one = (ar == 1) & (br == 1)
    if sky:
        one &= (bits(a) == 0).all(axis=1)
    else:
        assert one.any()
    bad = np.nonzero(one & ~same_bits(a, b).all(axis=1))[0]
    assert bad.size == 0, (sid, hook, bad[:5], a[bad[:5]], b[bad[:5]])
    assert not (b[np.isfinite(b)] < 0).any() and not (a[np.isfinite(a)] < 0).any()
    # diverged as tools/divergence.py defines it
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ok = np.isfinite(a64).all(axis=1) & np.isfinite(b64).all(axis=1)
    with np.errstate(invalid="ignore"):
        rel = np.abs(a64 - b64).max(axis=1) / np.maximum(np.abs(a64).max(axis=1), 1e-3)
    div = (ar != br) | ~ok | (rel > 1e-3)
    pct = 100.0 * float(div.mean())
    print("tolerance_paths " + json.dumps({
        "scene": sid, "hook": hook, "build": "fastz", "width": w, "height": h, "spp": spp, "paths": int(len(ar)),
        "diverged_pct": round(pct, 5), "rays_differ_pct": round(100.0 * float((ar != br).mean()), 5),
        "nonfinite_paths": int((~ok).sum()), "ray_ratio": round(bt / at, 6), "one_ray_paths_compared": int(one.sum()),
        "cap_pct": cap_pct}))
    if cap_pct is not None:
        assert pct <= cap_pct, (sid, hook, pct, cap_pct)
    return pct


# ---------------------------------------------------------------- part 3: pex == forward restatement
@pytest.mark.parametrize("sid", [6, 7, 8])
def test_path_exact_build_equals_forward_restatement(gpu, orc, sid, monkeypatch):
    r = renderer(gpu, sid, None, monkeypatch)
    w, spp = scene_size(gpu, sid, monkeypatch)
    assert_equals_forward(gpu, r, forward_ref(gpu, orc, sid, w, w, spp), w, w, spp, f"scene {sid}")


@pytest.mark.parametrize("sid,hook", [(6, GEN), (7, GEN), (7, NOBVHW), (8, NOSIG)])
def test_other_walks_of_the_path_exact_scenes(gpu, orc, sid, hook, monkeypatch):
    """The same scenes through the walks the test hooks force: the build each yields is BUILD's literal;
    a path-exact one equals the forward restatement bit for bit, the fast arithmetic (the bunny on the
    interpreter) holds the per-path bars against the exact contract, its diverged share within twice
    the share recorded for that scene under the fast arithmetic."""
    r = renderer(gpu, sid, hook, monkeypatch)
    assert r.kernel_info()["kernel_features"] != renderer(gpu, sid, None, monkeypatch).kernel_info()["kernel_features"] or hook == NOBVHW
    w, spp = scene_size(gpu, sid, monkeypatch)
    if BUILD[(sid, hook)] == "pex":
        assert_equals_forward(gpu, r, forward_ref(gpu, orc, sid, w, w, spp), w, w, spp, f"scene {sid} [{hook}]")
    else:
        fast_against_exact(gpu, r, sid, hook, w, w, spp, sky=False, cap_pct=2.0 * RECORDED_PCT[sid])


@pytest.mark.parametrize("w,h,spp,depth,ts", [(1, 1, 1, 32, 32), (37, 23, 9, 0, 7), (37, 23, 9, 1, 7)])
def test_path_exact_edges(gpu, orc, w, h, spp, depth, ts, monkeypatch):
    """Scene 6 at 1 x 1 x 1, and with ragged tiles at depth 0 (every path is its camera ray) and depth 1."""
    r = renderer(gpu, 6, None, monkeypatch)
    assert_equals_forward(gpu, r, forward_ref(gpu, orc, 6, w, h, spp, depth=depth), w, h, spp, "scene 6 edge", depth=depth, tile_size=ts)


def test_path_exact_mode1_chunked(gpu, orc, monkeypatch):
    """draw2()'s running average over launches of 5 samples (no debug flag: the chunks are real):
    image and ray total equal the forward restatement's mode 1."""
    w, h, spp = 37, 23, 16
    r = renderer(gpu, 6, None, monkeypatch)
    oimg, orays, _, _ = forward_ref(gpu, orc, 6, w, h, spp, mode=1, paths=False)
    img, rays = r.render(gpu.render_desc(w, h, spp, mode=1, chunk_samples=5, numerics="fast"))
    assert gpu._lib.BUILDS[r.kernel_info()["build"]] == "pex"
    assert rays == orays
    assert same_bits(img, oimg).all()


# ---------------------------------------------------------------- part 4: fastz against the exact contract
@pytest.mark.parametrize("sid,w,spp", [(5, 96, 64), (9, 64, 64)])
def test_fast_arithmetic_per_path(gpu, sid, w, spp, monkeypatch):
    """At these sizes (590 k and 262 k paths; about 1250 and 350 diverged) twice the recorded share is
    more than 20 standard deviations of the count above it; every ablation recorded in
    profiles/r04_divergence.jsonl lies within 10 % of it."""
    fast_against_exact(gpu, renderer(gpu, sid, None, monkeypatch), sid, None, w, w, spp, sky=False, cap_pct=2.0 * RECORDED_PCT[sid])


@pytest.mark.parametrize("sid", [0, 1, 2, 3, 4])
def test_fast_arithmetic_per_path_sky_scenes(gpu, sid, monkeypatch):
    """Scenes 0-4 have no recorded share: the two exact assertions, and the share on record (no cap).
    (Under the sky a one-ray path is the sky's blend, arithmetic the contracts round differently; only a
    black one would be exact, and these scenes have none today -- the printed line says how many were
    compared.  Measured shares 1.6 / 10.2 / 0.002 / 7.2 / 4.5 %: the textures on the 1000-unit ground
    sphere)"""
    fast_against_exact(gpu, renderer(gpu, sid, None, monkeypatch), sid, None, 64, 64, 64, sky=True)


# ---------------------------------------------------------------- part 5: the hand-over
def host_fold(p, ns, max_lum=1000.0):
    """draw()'s per-pixel rule over samples p[..., s, :] in float32, operation by operation as
    main.cpp:161-173: a non-finite sample is replaced by the running sum; the final divide; the
    luminance clamp."""
    f = np.float32
    c = np.zeros(p.shape[:-2] + (3,), dtype=f)
    for s in range(ns):
        smp = p[..., s, :]
        fin = np.isfinite(smp).all(axis=-1, keepdims=True)
        c = c + np.where(fin, smp, c)
    c = c / f(ns)
    lum = (c[..., 0] * f(0.212655) + c[..., 1] * f(0.715158)) + c[..., 2] * f(0.072187)
    big = lum > f(max_lum)
    if big.any():
        c[big] = c[big] * (f(max_lum) / lum[big])[..., None]
    return c


def explain_pixel(p_fast, p_fwd, want, ns, max_size=4, chunk=1 << 14):
    """The smallest set of samples (size 1..max_size, among those whose bits differ) whose substitution
    from p_fwd into p_fast folds to want's bits; None when there is none."""
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(~same_bits(p_fast, p_fwd).all(axis=1))[0]
    for k in range(1, max_size + 1):
        it = itertools.combinations(cand, k)
        while True:
            sets = np.array(list(itertools.islice(it, chunk)), dtype=np.int64).reshape(-1, k)
            if not len(sets):
                break
            p = np.repeat(p_fast[None], len(sets), axis=0)
            rows = np.arange(len(sets))[:, None]
            p[rows, sets] = p_fwd[sets]
            with np.errstate(invalid="ignore", over="ignore"):
                hit = np.nonzero((bits(host_fold(p, ns)) == bits(want)).all(axis=1))[0]
            if hit.size:
                return tuple(int(x) for x in sets[hit[0]])
    return None


@pytest.mark.parametrize("walk", ["specialised", "interpreter"])
def test_hand_over_writes_the_forward_restatement(gpu, orc, monkeypatch, walk):
    """The retrace kernel is the path-exact arithmetic at one path per lane: what it writes over a
    listed path's radiance must be the forward restatement's radiance of that path.  Image `a` (paths
    handed over) against image `b` (MRT_RETRACE=0) and the per-path radiance of the fast kernel (a
    debug render hands nothing over): `b` is the host fold of those paths bit for bit, and every pixel
    where `a` differs is the host fold after substituting the restatement's radiance for a smallest
    set of 1 to 4 samples; over all pixels no more substitutions than paths were listed."""
    hook = NOSIG if walk == "interpreter" else None
    w, h, spp = 250, 250, 64
    r = renderer(gpu, 5, hook, monkeypatch)
    d = gpu.render_desc(w, h, spp, numerics="fast")
    before = r.kernel_info()["handed_over"]
    a, ra = r.render(d)
    ki = r.kernel_info()
    listed = ki["handed_over"] - before
    assert ki["handover_lost"] == 0
    with monkeypatch.context() as mp:
        if hook:
            mp.setenv(hook, "1")
        mp.setenv("MRT_RETRACE", "0")
        r0 = gpu.Renderer(scene(gpu, 5), 0)
    b, rb = r0.render(d)
    assert r0.kernel_info()["handed_over"] == 0 and ra == rb
    dd = gpu.render_desc(w, h, spp, numerics="fast", flags=gpu._lib.RF_PATH_DEBUG)
    r0.render(dd)
    p_fast = gpu_paths(gpu, r0, dd)[0].reshape(h * w, spp, 3)
    r0.close()
    with np.errstate(invalid="ignore", over="ignore"):
        folded = host_fold(p_fast, spp)
    assert np.array_equal(bits(folded), bits(b.reshape(-1, 4)[:, :3])), "the host restatement of the fold"
    changed = np.nonzero((bits(a.reshape(-1, 4)[:, :3]) != bits(b.reshape(-1, 4)[:, :3])).any(axis=1))[0]
    od = orc.desc(w, h, spp, fold=1)
    sizes, unexplained = {}, []
    for pix in changed:
        fwd = np.stack([orc.path(scene(gpu, 5), od, pix % w, pix // w, s)[0] for s in range(spp)])
        got = explain_pixel(p_fast[pix], fwd, a.reshape(-1, 4)[pix, :3], spp)
        if got is None:
            unexplained.append(int(pix))
        else:
            sizes[len(got)] = sizes.get(len(got), 0) + 1
    print(f"hand-over [{walk}]: listed {listed}, changed pixels {len(changed)}, substitutions per pixel {dict(sorted(sizes.items()))}, "
          f"unexplained {unexplained[:10]}")
    assert not unexplained, unexplained[:10]
    assert sum(k * n for k, n in sizes.items()) <= listed
    assert 0 < len(changed)
