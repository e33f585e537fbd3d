"""include/mrt_mathfn.h on the device, against its host evaluation, bit for bit.

The header is compiled into the reference build, the restatement, the CPU backend and every device unit,
so no parity sees an error in it; tests/test_mathfn_host.py pins the host evaluation to mpmath.  The device
build is other code: double division is v_rcp_f64 + v_div_fixup_f64, double sqrt a v_rsq_f64 refinement,
rint v_rndne_f64, the conversions expansions of their own, the coefficients and atan2's pi pass through
inline assembly.  Here the ten float functions and the four double cores run on the device through
mrt_mathfn_device / mrt_mathfn_d_device and must give the host's bits: -0 is not +0, subnormals are kept,
NaN matches NaN whatever the payload.  A float differs only where the double lands within an ulp of double
of a rounding boundary (~2^-29 of arguments); the doubles differ wherever a device operation is not
correctly rounded, which is what makes the double tests sensitive.

The reference is the host evaluation twice: oracle.mathfn[_d] (gcc) and mrt.mathfn[_d] (hipcc's host
pass).  The tests without the gpu mark need no device: the two compilers agree on every set, and the
edge sets this file adds to the host test's are held to mpmath's bracket and to values IEEE fixes.

No finite trigonometric argument past |x| < 2^20 appears: the contract ends there (the header says why).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_mathfn_host import (F32, F64, INF, N, NAN, asin_args, assert_share, atan2_args, check, exp_args, log_args, near_multiples_of_half_pi,
                              pow5_args, pow_args, special_values, trig_args)

gpu_only = pytest.mark.gpu
FLOAT_FNS = ("sin", "cos", "tan", "log", "log10", "asin", "exp", "pow5", "atan2", "pow")
DOUBLE_FNS = ("sincos", "log", "exp", "atan2")
SENTINEL32, SENTINEL64 = np.uint32(0xDEADBEEF), np.uint64(0xDEADBEEFCAFEF00D)


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def ubits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def first_difference(got, want):
    """None where got == want in every bit or both are NaN; else (index, got bits, want bits) of the first miss."""
    bad = np.nonzero((ubits(got) != ubits(want)) & ~(np.isnan(got) & np.isnan(want)))[0]
    return None if len(bad) == 0 else (int(bad[0]), hex(int(ubits(got)[bad[0]])), hex(int(ubits(want)[bad[0]])), len(bad))


def around(x, k, dtype=F32):
    """x and its k neighbours on each side."""
    up, dn = [dtype(x)], [dtype(x)]
    for _ in range(k):
        up.append(np.nextafter(up[-1], dtype(np.inf)))
        dn.append(np.nextafter(dn[-1], dtype(-np.inf)))
    return np.array(dn[:0:-1] + up, dtype=dtype)


def signed_exponents(rng, n, lo, hi):
    return np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(lo, hi + 1, n)) * rng.choice([-1.0, 1.0], n)


# ---------------------------------------------------------------- the argument sets
SUBNORMALS = np.array([2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -140, 2.0 ** -127, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126], dtype=F32)


@functools.lru_cache(maxsize=None)
def edge_sets():
    """Edges the host test lacks, all inside the documented domains: name -> (a, b or None)."""
    rng = np.random.default_rng(21)
    top = np.nextafter(F32(2.0 ** 20), F32(0))  # 2^20 - ulp
    sub = np.concatenate([SUBNORMALS, np.ldexp(rng.uniform(0.5, 1.0, 256), rng.integers(-148, -126, 256)).astype(F32)])
    trig = np.concatenate([around(top, 8)[:9], -around(top, 8)[:9], sub, -sub])
    # exp: around ln FLT_MAX, ln 2^-126 (first subnormal result) and ln 2^-150 (first zero), and through the subnormal results
    exp = np.concatenate([around(88.72284, 64), around(-87.33655, 64), around(-103.97208, 64), np.linspace(-104.0, -87.0, 4096).astype(F32)])
    # pow5 with subnormal results: |x|^5 in [2^-150, 2^-125]
    p5 = signed_exponents(rng, 4096, -29, -24).astype(F32)
    p5 = np.concatenate([p5, np.array([2.0 ** -29, 2.0 ** -25.2], dtype=F32)])  # (the exact tie (2^-30)^5 is in pinned_values)
    # pow: y = 5 (the pow5 shortcut) beside its neighbours; y up to 128 with x down to the smallest normal
    x5 = np.concatenate([rng.uniform(0.0, 1.0, 2048), np.ldexp(rng.uniform(0.5, 1.0, 2048), rng.integers(-30, 2, 2048))]).astype(F32)
    x5 = x5[x5 > 0]
    five = F32(5)
    xw = np.ldexp(rng.uniform(0.5, 1.0, 8192), rng.integers(-125, 2, 8192)).astype(F32)
    yw = np.concatenate([rng.uniform(0.0, 128.0, 4096), rng.choice([0.25, 1.0, 5.0, 32.0, 127.0, 128.0], 4096)]).astype(F32)
    keep = yw > 0
    pow_a = np.concatenate([x5, x5, x5, xw[keep], np.array([2.0 ** -126, 0.5, 0.5], dtype=F32)])
    pow_b = np.concatenate([np.full_like(x5, five), np.full_like(x5, np.nextafter(five, INF)), np.full_like(x5, np.nextafter(five, -INF)), yw[keep],
                            np.array([128.0, 128.0, 126.0], dtype=F32)])
    # atan2: |y / x| across 2^+-100, and y = +-x
    ex = rng.integers(-40, 21, 8192)
    xr = (np.ldexp(rng.uniform(0.5, 1.0, 8192), ex) * rng.choice([-1.0, 1.0], 8192)).astype(F32)
    yr = (np.ldexp(rng.uniform(0.5, 1.0, 8192), ex + rng.integers(-100, 101, 8192)) * rng.choice([-1.0, 1.0], 8192)).astype(F32)
    keep = (yr != 0) & np.isfinite(yr)
    xd = signed_exponents(rng, 2048, -120, 120).astype(F32)
    at_a = np.concatenate([yr[keep], xd, -xd])
    at_b = np.concatenate([xr[keep], xd, xd])
    return {"sin": (trig, None), "cos": (trig, None), "tan": (trig, None), "exp": (exp, None), "pow5": (p5, None), "pow": (pow_a, pow_b),
            "atan2": (at_a, at_b)}


def pinned_values():
    """Results IEEE (or exact arithmetic followed by one rounding) fixes, beyond special_values(): rows
    (function, arguments, wanted float)."""
    rows = []
    for x in np.concatenate([SUBNORMALS, -SUBNORMALS]):  # sin x = x - x^3/6, tan x = x + x^3/3: nearest float is x
        rows += [("sin", (x,), x), ("tan", (x,), x), ("asin", (x,), x), ("cos", (x,), F32(1))]
    rows += [("exp", (F32(88.73),), INF), ("exp", (F32(-103.98),), F32(0)), ("exp", (F32(-103.5),), F32(2.0 ** -149)),  # e^-103.5 = 0.80 * 2^-149
             ("exp", (F32(-104),), F32(0))]
    # x^5 of powers of two is exact: 2^-145 is a subnormal float, 2^-150 is the tie between 0 and 2^-149 (to even: 0)
    rows += [("pow5", (F32(2.0 ** -29),), F32(2.0 ** -145)), ("pow5", (F32(2.0 ** -30),), F32(0)), ("pow5", (F32(-2.0 ** -30),), F32(-0.0)),
             ("pow5", (F32(-2.0 ** -29),), F32(-2.0 ** -145)), ("pow", (F32(2.0 ** -29), F32(5)), F32(2.0 ** -145))]
    # powers of 1/2: the double before the rounding is within a few ulp of double of an exact float
    rows += [("pow", (F32(0.5), F32(128)), F32(2.0 ** -128)), ("pow", (F32(0.5), F32(126)), F32(2.0 ** -126)), ("pow", (F32(0.5), F32(127)), F32(2.0 ** -127)),
             ("pow", (F32(2.0 ** -126), F32(1)), F32(2.0 ** -126)), ("pow", (F32(2.0 ** -126), F32(128)), F32(0))]
    pi = np.float64(np.pi)
    for x in (F32(3.0), F32(2.0 ** -120), F32(2.0 ** 100), F32(1.7e-42)):  # y = +-x: the quotient is exactly 1
        rows += [("atan2", (x, x), F32(pi / 4)), ("atan2", (-x, x), F32(-pi / 4)), ("atan2", (x, -x), F32(3 * pi / 4)), ("atan2", (-x, -x), F32(-3 * pi / 4))]
    rows += [(name, (s,), NAN) for name in ("sin", "cos", "tan") for s in (INF, -INF)]
    return rows


@functools.lru_cache(maxsize=None)
def float_sets(name):
    """(a, b or None) for one function: the host test's sets, this file's edges, the special and pinned rows' arguments."""
    parts = []
    if name in ("sin", "cos", "tan"):
        parts += [(trig_args(11), None), (near_multiples_of_half_pi(), None)]
    elif name in ("log", "log10"):
        parts += [(s, None) for s in log_args(12)]
    elif name == "asin":
        parts += [(s, None) for s in asin_args(13)]
    elif name == "exp":
        parts += [(s, None) for s in exp_args(14)]
    elif name == "pow5":
        parts += [(s, None) for s in pow5_args(15)]
    elif name == "atan2":
        parts += list(atan2_args(16))
    else:
        parts += [pow_args(17)]
    if name in edge_sets():
        parts.append(edge_sets()[name])
    rows = [r for r in special_values() + pinned_values() if r[0] == name]
    parts.append((np.array([r[1][0] for r in rows], dtype=F32), np.array([r[1][-1] for r in rows], dtype=F32) if name in ("atan2", "pow") else None))
    a = np.concatenate([p[0] for p in parts]).astype(F32)
    b = np.concatenate([p[1] for p in parts]).astype(F32) if name in ("atan2", "pow") else None
    return a, b


def widen(rng, x):
    """Floats widened to double mantissas: the low 29 bits of the double's fraction drawn at random."""
    b = np.ascontiguousarray(x, dtype=F64).view(np.uint64) | rng.integers(0, 1 << 29, len(x), dtype=np.uint64)
    return b.view(F64)


@functools.lru_cache(maxsize=None)
def double_sets(name):
    """(a, b or None) for one double core: 2^18 seeded doubles over the range its float callers reach, the
    doubles no float reaches, and the special operands."""
    rng = np.random.default_rng(31 + DOUBLE_FNS.index(name))
    nan, inf = np.nan, np.inf
    if name == "sincos":
        x = np.concatenate([rng.uniform(-2.0 ** 20, 2.0 ** 20, N // 2), signed_exponents(rng, N // 2, -60, 20)])
        x = x[np.abs(x) < 2.0 ** 20]
        k = np.arange(1, (1 << 12) + 1) * (np.pi / 2)  # doubles next to multiples of pi/2
        k = np.concatenate([k, np.nextafter(k, inf), np.nextafter(k, -inf)])
        sub = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1040, 2.0 ** -1022, np.nextafter(2.0 ** 20, 0), -np.nextafter(2.0 ** 20, 0), nan, inf, -inf])
        return np.concatenate([x, k, -k, widen(rng, near_multiples_of_half_pi()), sub]), None
    if name == "log":
        x = np.ldexp(rng.uniform(1.0, 2.0, N), rng.integers(-149, 128, N))  # every float exponent
        one = np.concatenate([around(1.0, 4096, F64), 1.0 + np.arange(-4096, 4097) * 2.0 ** -24, widen(rng, log_args(12)[1])])
        subn = np.ldexp(rng.uniform(1.0, 2.0, 4096), rng.integers(-1074, -1022, 4096))  # the 2^54 branch
        root2 = around(1.4142135623730951, 64, F64)  # the m > sqrt 2 fold
        sp = np.array([0.0, -0.0, 5e-324, 2.2250738585072014e-308, np.nextafter(2.2250738585072014e-308, 0), 1.0, -1.0, -5e-324, nan, inf, -inf,
                       np.finfo(F64).max])
        return np.concatenate([x, one, subn, root2, 2.0 * root2, sp]), None
    if name == "exp":
        x = rng.uniform(-745.0, 709.0, N)
        px, py = pow_args(17)
        ea, eb = edge_sets()["pow"]
        import oracle
        prod = np.concatenate([py.astype(F64) * oracle.mathfn_d("log", px.astype(F64)), eb.astype(F64) * oracle.mathfn_d("log", ea.astype(F64))])
        subn = rng.uniform(-745.0, -708.0, 4096)  # results in the subnormal-double range
        small = signed_exponents(rng, 4096, -60, 0)
        sp = np.array([0.0, -0.0, 709.0, np.nextafter(709.0, inf), 709.5, 710.0, -745.0, np.nextafter(-745.0, -inf), -745.5, -746.0, 1e308, -1e308,
                       nan, inf, -inf, 5e-324, -5e-324])
        return np.concatenate([x, prod, subn, small, widen(rng, edge_sets()["exp"][0]), sp]), None
    (y, x), (u0, u1) = atan2_args(16)
    ea, eb = edge_sets()["atan2"]
    far_y, far_x = signed_exponents(rng, 8192, -1000, 1000), signed_exponents(rng, 8192, -1000, 1000)  # quotients that over- and underflow
    d = signed_exponents(rng, 2048, -1000, 1000)
    sub_y, sub_x = np.ldexp(rng.uniform(0.5, 1.0, 1024), rng.integers(-1073, -1021, 1024)), np.ldexp(rng.uniform(0.5, 1.0, 1024), rng.integers(-1073, -1021, 1024))
    t = [r[1] for r in special_values() if r[0] == "atan2"]
    a = np.concatenate([widen(rng, y), widen(rng, u0), widen(rng, ea), far_y, d, -d, sub_y, -sub_y, np.array([float(r[0]) for r in t])])
    b = np.concatenate([widen(rng, x), widen(rng, u1), widen(rng, eb), far_x, d, d, sub_x, sub_x, np.array([float(r[1]) for r in t])])
    return a, b


# ---------------------------------------------------------------- host only: two compilers, and the new edges' values
@pytest.mark.parametrize("name", FLOAT_FNS)
def test_two_compilers_agree_on_the_floats(mrt, orc, name):
    """mrt.mathfn (hipcc's host pass) == oracle.mathfn (gcc) on every float set, bit for bit."""
    a, b = float_sets(name)
    assert len(a) >= (1 << 17)
    assert first_difference(mrt.mathfn(name, a, b), orc.mathfn(name, a, b)) is None


@pytest.mark.parametrize("name", DOUBLE_FNS)
def test_two_compilers_agree_on_the_double_cores(mrt, orc, name):
    a, b = double_sets(name)
    assert len(a) >= (1 << 17)
    got, want = mrt.mathfn_d(name, a, b), orc.mathfn_d(name, a, b)
    for g, w in zip(got, want) if name == "sincos" else [(got, want)]:
        assert first_difference(g, w) is None


@pytest.mark.parametrize("name", sorted(edge_sets()))
def test_edges_bracket_the_true_value(orc, name):
    """The edge sets added here, held to what the host test holds its own sets to: each result is one of the
    two floats around mpmath's value, and at most 1e-6 of them are not the nearest."""
    assert_share(name, [check(orc, name, *edge_sets()[name])])


def test_pinned_values_on_the_host(mrt, orc):
    for name, args, want in pinned_values():
        for m in (mrt, orc):
            got = m.mathfn(name, *[np.array([v], dtype=F32) for v in args])[0]
            assert first_difference(np.array([got]), np.array([want], dtype=F32)) is None, (name, [float(v) for v in args], float(got), float(want))


def test_host_argument_errors(mrt):
    L = mrt.lib()
    a = np.zeros(4, dtype=F32)
    p = a.ctypes.data
    assert L.mrt_mathfn(10, 4, p, p, p) == 1 and L.mrt_mathfn(0, 4, None, None, p) == 1 and L.mrt_mathfn(0, 4, p, None, None) == 1
    assert L.mrt_mathfn(8, 4, p, None, p) == 1 and L.mrt_mathfn(0, 4, p, None, p) == 0 and L.mrt_mathfn(9, 0, p, p, p) == 0
    d = np.zeros(4, dtype=F64)
    q = d.ctypes.data
    assert L.mrt_mathfn_d(4, 4, q, q, q, q) == 1 and L.mrt_mathfn_d(0, 4, q, None, q, None) == 1 and L.mrt_mathfn_d(3, 4, q, None, q, None) == 1
    assert L.mrt_mathfn_d(1, 4, None, None, q, None) == 1 and L.mrt_mathfn_d(1, 4, q, None, q, None) == 0
    with pytest.raises(ValueError):
        mrt.mathfn("sinh", a)
    with pytest.raises(ValueError):
        mrt.mathfn("pow", a)


# ---------------------------------------------------------------- the device
def on_device(gpu, name, a, b=None, pad=64, stream=None):
    """mathfn_device over a (and b) into a sentinel-filled buffer of len(a) + pad floats: (results, tail)."""
    import torch
    n = len(a)
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(b, dtype=F32)).cuda() if b is not None else None
    out = torch.from_numpy(np.full(n + pad, SENTINEL32, dtype=np.uint32).view(F32)).cuda()
    st = stream if stream is not None else torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.mathfn_device(name, n, ta.data_ptr(), tb.data_ptr() if tb is not None else 0, out.data_ptr(), st.cuda_stream)
    st.synchronize()
    o = out.cpu().numpy()
    return o[:n], o[n:]


def on_device_d(gpu, name, a, b=None, pad=64):
    import torch
    n = len(a)
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=F64)).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(b, dtype=F64)).cuda() if b is not None else None
    outs = [torch.from_numpy(np.full(n + pad, SENTINEL64, dtype=np.uint64).view(F64)).cuda() for _ in range(2)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.mathfn_d_device(name, n, ta.data_ptr(), tb.data_ptr() if tb is not None else 0, outs[0].data_ptr(), outs[1].data_ptr(), st.cuda_stream)
    st.synchronize()
    o = [t.cpu().numpy() for t in outs]
    return [x[:n] for x in o], [x[n:] for x in o]


@gpu_only
@pytest.mark.parametrize("name", FLOAT_FNS)
def test_device_floats_equal_the_host_s(gpu, orc, name):
    """The host test's sets, the edges, the special and pinned arguments in one batch per function."""
    a, b = float_sets(name)
    got, tail = on_device(gpu, name, a, b)
    assert (ubits(tail) == SENTINEL32).all()
    assert first_difference(got, orc.mathfn(name, a, b)) is None
    assert first_difference(got, gpu.mathfn(name, a, b)) is None


@gpu_only
def test_device_special_and_pinned_values(gpu):
    """The whole special-value table (the atan2 zero / infinity quadrant table included) and the pinned edge
    values, one device batch per function, against the values themselves."""
    rows = special_values() + pinned_values()
    for name in FLOAT_FNS:
        mine = [r for r in rows if r[0] == name]
        a = np.array([r[1][0] for r in mine], dtype=F32)
        b = np.array([r[1][-1] for r in mine], dtype=F32) if name in ("atan2", "pow") else None
        want = np.array([r[2] for r in mine], dtype=F32)
        got, _ = on_device(gpu, name, a, b)
        miss = first_difference(got, want)
        assert miss is None, (name, miss, [float(v) for v in mine[miss[0]][1]])


@gpu_only
@pytest.mark.parametrize("name", DOUBLE_FNS)
def test_device_double_cores_equal_the_host_s(gpu, orc, name):
    a, b = double_sets(name)
    got, tails = on_device_d(gpu, name, a, b)
    want = orc.mathfn_d(name, a, b)
    want = list(want) if name == "sincos" else [want]
    mine = gpu.mathfn_d(name, a, b)
    mine = list(mine) if name == "sincos" else [mine]
    for k in range(len(want)):
        miss = first_difference(got[k], want[k])
        assert miss is None, (name, k, miss, float(a[miss[0]]), None if b is None else float(b[miss[0]]))
        assert first_difference(got[k], mine[k]) is None
    assert (ubits(tails[0]) == SENTINEL64).all() and (ubits(tails[1]) == SENTINEL64).all()
    assert name == "sincos" or (ubits(got[1]) == SENTINEL64).all()  # out2 is written by sincos only


@gpu_only
@pytest.mark.parametrize("n", [1, 63, 65, 1 << 18])
def test_exactly_n_results(gpu, orc, n):
    """One thread per element: n results, and the sentinel-filled tail of the buffers stays untouched."""
    for name in ("tan", "pow"):
        a, b = float_sets(name)
        a, b = a[:n], (b[:n] if b is not None else None)
        got, tail = on_device(gpu, name, a, b, pad=300)
        assert (ubits(tail) == SENTINEL32).all() and first_difference(got, orc.mathfn(name, a, b)) is None
    a, _ = double_sets("sincos")
    got, tails = on_device_d(gpu, "sincos", a[:n], pad=300)
    s, c = orc.mathfn_d("sincos", a[:n])
    assert (ubits(tails[0]) == SENTINEL64).all() and (ubits(tails[1]) == SENTINEL64).all()
    assert first_difference(got[0], s) is None and first_difference(got[1], c) is None


@gpu_only
def test_stream_order_between_two_enqueues(gpu, orc):
    """The call reads what the enqueue before it wrote and the enqueue after it reads what it wrote, on one
    stream with nothing synchronised in between."""
    import torch
    y, x = (s[:5000] for s in atan2_args(16)[0])
    ty, tx = torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()
    src, out, copy = torch.zeros_like(ty), torch.zeros_like(ty), torch.zeros_like(ty)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        src.copy_(ty)
        gpu.mathfn_device("atan2", len(y), src.data_ptr(), tx.data_ptr(), out.data_ptr(), st.cuda_stream)
        copy.copy_(out)
    st.synchronize()
    assert first_difference(copy.cpu().numpy(), orc.mathfn("atan2", y, x)) is None


@gpu_only
def test_graph_capture_replays_on_new_contents(gpu, orc):
    import torch
    xs = [exp_args(14)[0][:4097], edge_sets()["exp"][0][:4097]]
    a = torch.from_numpy(xs[0]).cuda()
    out = torch.zeros_like(a)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.mathfn_device("exp", len(xs[0]), a.data_ptr(), 0, out.data_ptr(), side.cuda_stream)  # once outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gpu.mathfn_device("exp", len(xs[0]), a.data_ptr(), 0, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for x in (xs[1], xs[0]):
        a.copy_(torch.from_numpy(x))
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert first_difference(out.cpu().numpy(), orc.mathfn("exp", x)) is None
    del graph


@gpu_only
def test_device_argument_errors(gpu):
    import torch
    L = gpu.lib()
    t = torch.zeros(8, dtype=torch.float64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    assert L.mrt_mathfn_device(10, 4, p, p, p, None) == 1 and L.mrt_mathfn_device(0, 4, None, None, p, None) == 1
    assert L.mrt_mathfn_device(0, 4, p, None, None, None) == 1 and L.mrt_mathfn_device(9, 4, p, None, p, None) == 1
    assert L.mrt_mathfn_device(9, 0, p, p, p, None) == 0
    assert L.mrt_mathfn_d_device(4, 4, p, p, p, p, None) == 1 and L.mrt_mathfn_d_device(0, 4, p, None, p, None, None) == 1
    assert L.mrt_mathfn_d_device(3, 4, p, None, p, None, None) == 1 and L.mrt_mathfn_d_device(2, 4, None, None, p, None, None) == 1
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 0).all()  # a refused call enqueues nothing
    with pytest.raises(gpu.MrtError):
        gpu.mathfn_device("sin", 4, 0, 0, t.data_ptr())
