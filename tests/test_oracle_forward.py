"""The C restatement's forward fold (oracle.desc(fold=1)) against its pinned deepest-first fold.

fold=0 is the reference's recursion, pinned bit for bit by test_oracle_pinning.py.  fold=1 carries a
throughput T down the path (metal T = T*att; lambertian / isotropic T = (T*a)/pdf; end T*L_end) and is
the reference of the tolerance contract's path-exact kernels (test_tolerance_paths_gpu.py), so it
gets a check of its own here: the same geometry, draws and ray counts, and a product that differs
from the pinned one by rounding alone.

The bound is derived, not tuned.  Each fold rounds two operations per level (a*L then /pdf, or T*a
then /pdf; one for metal), each to 2^-24 relative, and every factor is non-negative, so nothing
cancels: two folds of a path of `rays` segments differ by at most 4 * rays * 2^-24 relative (first
order; measured margin about a factor 2).  Below 2^-100 a product may have passed through the
denormals in one order and not in the other, and the relative bound does not apply."""
import numpy as np
import pytest

CASES = [(0, 64, 64, 16), (2, 64, 64, 16), (5, 64, 64, 16), (6, 64, 64, 16), (8, 64, 64, 16), (9, 64, 64, 16), (5, 128, 128, 64)]
TINY = 2.0 ** -100
_scenes = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def both_folds(mrt, orc, sid, w, h, spp):
    if sid not in _scenes:
        _scenes[sid] = mrt.select_scene(sid, 1.0)
    sc = _scenes[sid]
    return [orc.render(sc, orc.desc(w, h, spp, threads=16, fold=f), paths=True) for f in (0, 1)]


@pytest.mark.parametrize("sid,w,h,spp", CASES)
def test_forward_fold_differs_from_the_pinned_fold_by_rounding_alone(mrt, orc, sid, w, h, spp):
    (_, rays0, p0, n0), (_, rays1, p1, n1) = both_folds(mrt, orc, sid, w, h, spp)
    assert rays0 == rays1 and rays0 == int(n0.sum(dtype=np.uint64))
    assert np.array_equal(n0, n1)
    one = n0 == 1
    assert one.any()
    assert np.array_equal(bits(p0[one]), bits(p1[one])), "a one-ray path is (1,1,1) * L_end: no level, no rounding"
    fin0, fin1 = np.isfinite(p0).all(axis=1), np.isfinite(p1).all(axis=1)
    assert np.array_equal(fin0, fin1), f"finite under one fold only: paths {np.nonzero(fin0 != fin1)[0][:5]}"
    a, b = p0.astype(np.float64), p1.astype(np.float64)
    mag = np.maximum(np.abs(a), np.abs(b))
    finite = (fin0 & fin1)[:, None] & np.ones((1, 3), dtype=bool)
    big = finite & (mag >= TINY)
    bound = 4.0 * n0[:, None].astype(np.float64) * 2.0 ** -24 * mag
    err = np.abs(a - b)
    worst = float((err[big] / bound[big]).max()) if big.any() else 0.0
    same = (bits(p0) == bits(p1)).all(axis=1)
    excluded = float((~finite | ((mag < TINY) & (mag > 0))).mean())  # non-finite or tiny non-zero channels (0 == 0 is compared below)
    print(f"scene {sid} {w}x{h}x{spp}: {len(n0)} paths, identical bits {same.mean():.4f}, largest error / bound {worst:.3f}, "
          f"tiny non-zero channels {int((finite & (mag < TINY) & (mag > 0)).sum())}, non-finite paths {int((~fin0).sum())}")
    assert (err[big] <= bound[big]).all(), worst
    assert np.array_equal((p0 == 0) & finite, (p1 == 0) & finite), "a channel is exactly 0 under one fold only"
    # not vacuous: nearly every channel is compared, and the option does something
    assert excluded <= 1e-4, excluded
    assert same.mean() < 0.95, same.mean()


def test_forward_fold_of_one_path_and_refusal(mrt, orc):
    """oracle_path honours fold (it equals the render's path); the reference's own order refuses it."""
    if 5 not in _scenes:
        _scenes[5] = mrt.select_scene(5, 1.0)
    sc = _scenes[5]
    d = orc.desc(16, 16, 16, threads=4, fold=1)
    _, _, prgb, prays = orc.render(sc, d, paths=True)
    _, _, prgb0, _ = orc.render(sc, orc.desc(16, 16, 16, threads=4), paths=True)
    differ = np.nonzero((bits(prgb) != bits(prgb0)).any(axis=1))[0]
    assert differ.size
    for i in list(differ[:8]) + [0, len(prays) - 1]:
        pix, s = divmod(int(i), 16)
        rgb, rays = orc.path(sc, d, pix % 16, pix // 16, s)
        assert rays == prays[i] and np.array_equal(bits(rgb), bits(prgb[i]))
    with pytest.raises(ValueError):
        orc.render_ref_order(sc, d)
    assert orc.lib().oracle_render_ref_order(None, d, 32, 0, 0, None) == 2 ** 64 - 1  # refused before anything is read
