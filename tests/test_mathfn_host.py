"""include/mrt_mathfn.h against a high-precision reference (host only).

The header claims that each float result "equals the correctly rounded value except for ~1e-8 of
arguments".  The reference build, the restatement and the kernels all share these functions, so the
bit-exact parities cannot see an error in them; this test can.  The ten functions are called through
oracle.mathfn (liboracle.so, test infrastructure) and compared with mpmath at 200 bits over their
documented domains:

* every result is one of the two floats that bracket the true value,
* the share of results that are not the nearest float is at most 1e-6 per function,
* the special values are IEEE's.

To keep 2^18 arguments per function quick, mpmath decides only where it has to.  numpy's double function
r of the same argument is within 2^-41 relative of the true value (glibc documents errors of an ulp or
two of double, 2^-52); where r is farther than that from every float and from every midpoint of two
adjacent floats, the true value rounds where r rounds, and the result must equal float32(r).  Every other
argument -- r within 2^-41 of a float or a midpoint, or a result that differs from float32(r) -- is
evaluated by mpmath.

The device side: the same header compiled for gfx950 is not the host's code (its double division, square
root, rint and conversions are instruction sequences of their own), and the render parities reach it only
at the arguments the scenes produce.  tests/test_mathfn_gpu.py evaluates the ten functions and their double
cores on the device through mrt_mathfn_device / mrt_mathfn_d_device, on the argument sets generated here
(trig_args, log_args, ... special_values) and on further edges, and requires the bits of this host code."""
import mpmath as mp
import numpy as np
import pytest

F32, F64 = np.float32, np.float64
N = 1 << 18
INF, NAN = F32(np.inf), F32(np.nan)
mp.mp.prec = 200

FN64 = {"sin": np.sin, "cos": np.cos, "tan": np.tan, "log": np.log, "log10": np.log10, "asin": np.arcsin, "exp": np.exp,
        "pow5": lambda x: x ** 5, "atan2": np.arctan2, "pow": np.power}
FNMP = {"sin": mp.sin, "cos": mp.cos, "tan": mp.tan, "log": mp.log, "log10": mp.log10, "asin": mp.asin, "exp": mp.exp,
        "pow5": lambda x: x ** 5, "atan2": mp.atan2, "pow": mp.power}


def bracket_mp(true):
    """(lo, hi, nearest) floats around an mpmath value (lo == hi when it is a float)."""
    with np.errstate(over="ignore"):  # (a value past FLT_MAX rounds to inf)
        c = F32(float(true))
    if np.isinf(c):
        c = F32(np.finfo(F32).max) * np.sign(c)
    cm = mp.mpf(float(c))
    lo, hi = (c, c) if cm == true else ((c, np.nextafter(c, INF)) if cm < true else (np.nextafter(c, -INF), c))
    if lo == hi:
        return lo, hi, lo
    if np.isinf(hi) or np.isinf(lo):
        # past FLT_MAX: nearest is inf from FLT_MAX + half an ulp (2^127 * (2 - 2^-24)) on
        edge = mp.mpf(2) ** 127 * (2 - mp.mpf(2) ** -24)
        return lo, hi, (hi if np.isinf(hi) and true >= edge else lo if np.isinf(lo) and -true >= edge else (lo if np.isinf(hi) else hi))
    dl, dh = true - mp.mpf(float(lo)), mp.mpf(float(hi)) - true
    return lo, hi, (lo if dl < dh else hi)


def check(orc, name, a, b=None):
    """Asserts the bracket property; returns (not nearest, arguments, decided by mpmath)."""
    a = np.ascontiguousarray(a, dtype=F32)
    got = orc.mathfn(name, a, b)
    args = (a.astype(F64),) if b is None else (a.astype(F64), np.ascontiguousarray(b, dtype=F32).astype(F64))
    with np.errstate(all="ignore"):
        r = FN64[name](*args)
        assert not np.isnan(r).any(), name  # (the domains below hold no invalid argument)
        near = r.astype(F32)
        n64 = near.astype(F64)
        lo = np.where(n64 <= r, near, np.nextafter(near, -INF)).astype(F64)
        hi = np.where(n64 >= r, near, np.nextafter(near, INF)).astype(F64)
        tol = np.abs(r) * 2.0 ** -41 + 1e-300
        fin = np.isfinite(lo) & np.isfinite(hi)
        mid = np.where(fin, 0.5 * lo + 0.5 * hi, np.inf)
        close = (np.abs(r - mid) <= tol) | (np.abs(r - lo) <= tol) | (np.abs(r - hi) <= tol)
    same = (got == near) | (np.isnan(got) & np.isnan(near))
    ask = np.nonzero(close | ~same)[0]
    not_nearest = 0
    for i in ask:
        true = FNMP[name](*(mp.mpf(float(x[i])) for x in args))
        l, h, nearest = bracket_mp(true)
        assert got[i] == l or got[i] == h, (name, [float(x[i]) for x in args], float(got[i]), float(l), float(h))
        not_nearest += int(got[i] != nearest)
    print(f"{name}: {len(a)} arguments, {len(ask)} decided by mpmath, {not_nearest} not the nearest float")
    return not_nearest, len(a), len(ask)


def assert_share(name, results):
    bad, n = sum(r[0] for r in results), sum(r[1] for r in results)
    assert bad <= 1e-6 * n, (name, bad, n)


def near_multiples_of_half_pi():
    k = np.arange(1, (1 << 12) + 1)
    x = np.array([float(mp.nstr(mp.mpf(int(i)) * mp.pi / 2, 20)) for i in k], dtype=F64).astype(F32)
    x = np.concatenate([x, np.nextafter(x, INF), np.nextafter(x, -INF)])
    return np.concatenate([x, -x])


def trig_args(seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(-2.0 ** 20, 2.0 ** 20, N // 2)
    g = np.ldexp(rng.uniform(0.5, 1.0, N // 2), rng.integers(-60, 21, N // 2)) * rng.choice([-1.0, 1.0], N // 2)
    x = np.concatenate([u, g]).astype(F32)
    return x[np.abs(x) < F32(2.0 ** 20)]


@pytest.mark.parametrize("name", ["sin", "cos", "tan"])
def test_trigonometric(orc, name):
    """|x| < 2^20: 2^18 seeded arguments (uniform and across the exponents) and the floats nearest
    k pi/2, k <= 2^12, with their neighbours (the hard cases of the reduction)."""
    assert_share(name, [check(orc, name, trig_args(11)), check(orc, name, near_multiples_of_half_pi())])


def log_args(seed):
    rng = np.random.default_rng(seed)
    e = rng.integers(-149, 128, N)  # all exponents, subnormals included
    x = np.ldexp(rng.uniform(1.0, 2.0, N), e).astype(F32)
    x = x[(x > 0) & np.isfinite(x)]
    one = F32(1.0)
    up, dn = [one], [one]
    for _ in range(1 << 12):
        up.append(np.nextafter(up[-1], INF))
        dn.append(np.nextafter(dn[-1], F32(0)))
    tiny = np.array([2.0 ** -149, 2.0 ** -148, 3 * 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, np.finfo(F32).max], dtype=F32)
    return x, np.concatenate([np.array(up[1:] + dn[1:], dtype=F32), tiny])


@pytest.mark.parametrize("name", ["log", "log10"])
def test_logarithms(orc, name):
    x, around_one = log_args(12)
    assert_share(name, [check(orc, name, x), check(orc, name, around_one)])


def asin_args(seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, N).astype(F32)
    top = [F32(1.0)]
    for _ in range(1 << 12):
        top.append(np.nextafter(top[-1], F32(0)))
    top = np.array(top[1:], dtype=F32)
    small = np.ldexp(rng.uniform(0.5, 1.0, 4096), rng.integers(-100, 0, 4096)).astype(F32)
    return x, np.concatenate([top, -top, small, -small])


def test_asin(orc):
    x, edges = asin_args(13)
    assert_share("asin", [check(orc, "asin", x), check(orc, "asin", edges)])


def exp_args(seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-104.0, 89.0, N).astype(F32)
    small = np.ldexp(rng.uniform(0.5, 1.0, 4096), rng.integers(-60, 0, 4096)).astype(F32)
    return x, np.concatenate([small, -small])


def test_exp(orc):
    x, small = exp_args(14)
    assert_share("exp", [check(orc, "exp", x), check(orc, "exp", small)])


def pow5_args(seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(0.0, 1.0, N // 2), np.ldexp(rng.uniform(0.5, 1.0, N // 2), rng.integers(-30, 26, N // 2))]).astype(F32)
    return x, -x[:4096]


def test_pow5(orc):
    x, neg = pow5_args(15)
    assert_share("pow5", [check(orc, "pow5", x), check(orc, "pow5", neg)])


def atan2_args(seed):
    """((y, x) across the exponents, (y, x) of random directions)."""
    rng = np.random.default_rng(seed)
    y = (np.ldexp(rng.uniform(0.5, 1.0, N), rng.integers(-40, 41, N)) * rng.choice([-1.0, 1.0], N)).astype(F32)
    x = (np.ldexp(rng.uniform(0.5, 1.0, N), rng.integers(-40, 41, N)) * rng.choice([-1.0, 1.0], N)).astype(F32)
    unit = rng.normal(size=(2, N // 4)).astype(F32)  # directions: sphere_uv's arguments
    return (y, x), (unit[0], unit[1])


def test_atan2(orc):
    wide, unit = atan2_args(16)
    assert_share("atan2", [check(orc, "atan2", *wide), check(orc, "atan2", *unit)])


def pow_args(seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, N).astype(F32)
    y = rng.uniform(0.0, 2.0, N).astype(F32)
    keep = (x > 0) & (y > 0)
    return x[keep], y[keep]


def test_pow_on_the_tone_map_s_domain(orc):
    assert_share("pow", [check(orc, "pow", *pow_args(17))])


def same(a, b):
    """Equal bits (so -0 is not +0), or NaN on both sides."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return bool((((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).all())


def special_values():
    """The special values as rows (function, arguments, wanted float; NaN = any NaN): IEEE's, and the
    atan2 quadrant / signed-zero / infinity table of C99 F.9.1.4."""
    z, nz = F32(0.0), F32(-0.0)
    pi = np.float64(np.pi)
    rows = []
    for name in ("sin", "tan", "asin"):
        rows += [(name, (z,), z), (name, (nz,), nz)]
    for name in ("sin", "cos", "tan"):
        rows += [(name, (NAN,), NAN)]
    rows += [("cos", (z,), F32(1)), ("cos", (nz,), F32(1))]
    rows += [("asin", (F32(1),), F32(pi / 2)), ("asin", (F32(-1),), F32(-pi / 2))]
    rows += [("asin", (F32(1.5),), NAN), ("asin", (NAN,), NAN), ("asin", (np.nextafter(F32(1), INF),), NAN)]
    for name in ("log", "log10"):
        rows += [(name, (z,), -INF), (name, (nz,), -INF), (name, (F32(1),), z)]
        rows += [(name, (F32(-1),), NAN), (name, (NAN,), NAN), (name, (INF,), INF)]
    rows += [("log10", (F32(1000),), F32(3)), ("log10", (F32(0.5) ** 0 * F32(1e10),), F32(10))]
    rows += [("exp", (z,), F32(1)), ("exp", (nz,), F32(1)), ("exp", (-INF,), z), ("exp", (INF,), INF)]
    rows += [("exp", (NAN,), NAN), ("exp", (F32(89),), INF), ("exp", (F32(-104),), z)]
    rows += [("pow5", (z,), z), ("pow5", (nz,), nz), ("pow5", (INF,), INF), ("pow5", (F32(2),), F32(32))]
    rows += [("pow5", (NAN,), NAN), ("pow5", (F32(-2),), F32(-32))]
    table = [(z, F32(1), z), (nz, F32(1), nz), (z, F32(-1), F32(pi)), (nz, F32(-1), F32(-pi)), (z, z, z), (nz, z, nz),
             (z, nz, F32(pi)), (nz, nz, F32(-pi)), (F32(1), z, F32(pi / 2)), (F32(-1), z, F32(-pi / 2)), (F32(1), nz, F32(pi / 2)),
             (F32(-1), nz, F32(-pi / 2)), (F32(1), INF, z), (F32(-1), INF, nz), (F32(1), -INF, F32(pi)), (F32(-1), -INF, F32(-pi)),
             (INF, F32(1), F32(pi / 2)), (-INF, F32(1), F32(-pi / 2)), (INF, INF, F32(pi / 4)), (-INF, INF, F32(-pi / 4)),
             (INF, -INF, F32(3 * pi / 4)), (-INF, -INF, F32(-3 * pi / 4)), (F32(1), F32(1), F32(pi / 4)), (F32(-1), F32(-1), F32(-3 * pi / 4))]
    rows += [("atan2", (y, x), want) for y, x, want in table]
    rows += [("atan2", (NAN, F32(1)), NAN), ("atan2", (F32(1), NAN), NAN)]
    # pow on the tone map's domain: x in [0, 1], y > 0
    rows += [("pow", (F32(0.3), z), F32(1)), ("pow", (F32(1), F32(1.7)), F32(1)), ("pow", (z, F32(0.5)), z)]
    rows += [("pow", (F32(0.25), F32(0.5)), F32(0.5)), ("pow", (F32(0.5), F32(2)), F32(0.25)), ("pow", (F32(0.5), F32(5)), F32(0.03125))]
    rows += [("pow", (NAN, F32(0.5)), NAN), ("pow", (F32(-0.5), F32(0.5)), NAN)]
    return rows


def test_special_values(orc):
    for name, args, want in special_values():
        got = orc.mathfn(name, *[[v] for v in args])[0]
        assert same(got, want), (name, [float(v) for v in args], float(got), float(want))
