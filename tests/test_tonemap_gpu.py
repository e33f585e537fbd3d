"""mrt_lum_max_device and mrt_tonemap_device against the host mrt_tonemap_argb, bit for bit, on synthetic
buffers (no render): the sizes at which mrt_lum_max_kernel's wave reduction, block count and grid-stride
loop change course, its two-call use into one *d_lwmax, luminances across every float exponent, and the
pixels include/mrt_tonemap.h's comments argue about (NaN, negative, infinite, all black), the last also
against bytes worked out by hand (tests/test_host.py tonemap_edge_frames).  The host form is pinned to the
reference's display loop by tests/golden/tonemap_*.npz."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_host import tonemap_edge_frames

pytestmark = pytest.mark.gpu
F32 = np.float32
STRIDE = 2048 * 256  # mrt_lum_max_kernel's largest grid: past it the grid-stride loop takes a second trip


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def luminance(frame):
    """mrt_luminance in float32, operation by operation."""
    return (frame[:, 0] * F32(0.212655) + frame[:, 1] * F32(0.715158)) + frame[:, 2] * F32(0.072187)


def host_max(frame):
    """The host's sequential std::max from 0: NaN and negative luminances never win."""
    with np.errstate(all="ignore"):
        l = luminance(frame)
    l = l[l > 0]
    return l.max() if len(l) else F32(0)


def host_argb(gpu, frame):
    return gpu.tonemap_argb(frame.reshape(1, -1, 4)).reshape(-1)


def lum_max(gpu, t_rgb, first, n, t_lwmax, stream):
    gpu._lib.check(gpu.lib().mrt_lum_max_device(C.c_void_p(t_rgb.data_ptr() + 16 * first), n, C.c_void_p(t_lwmax.data_ptr()), C.c_void_p(stream)),
                   "mrt_lum_max_device")


def tonemap(gpu, t_rgb, first, n, t_lwmax, t_argb, stream):
    gpu.tonemap_device(t_rgb.data_ptr() + 16 * first, n, t_lwmax.data_ptr(), t_argb.data_ptr() + 4 * first, stream, reduce=False)


def device_tonemap(gpu, frame, parts=None, lwmax0=0.0):
    """(L_wmax read back, argb) of lum_max over each part into one *d_lwmax, then the tone map of each part."""
    import torch
    n = len(frame)
    parts = parts or [(0, n)]
    rgb = torch.from_numpy(np.ascontiguousarray(frame, dtype=F32)).cuda()
    argb = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lw = torch.full((1,), float(lwmax0), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for first, m in parts:
        lum_max(gpu, rgb, first, m, lw, st.cuda_stream)
    for first, m in parts:
        tonemap(gpu, rgb, first, m, lw, argb, st.cuda_stream)
    st.synchronize()
    out = argb.cpu().numpy().view(np.uint32)
    assert (out[n:] == 0x5A5A5A5A).all()  # exactly n pixels written
    return lw.cpu().numpy()[0], out[:n]


@functools.lru_cache(maxsize=None)
def random_frame(n):
    rng = np.random.default_rng(n)
    f = np.zeros((n, 4), dtype=F32)
    f[:, :3] = rng.exponential(0.5, size=(n, 3)).astype(F32)
    f[:, 3] = 1.0
    return f


SIZES = [1, 63, 64, 65, 255, 257, STRIDE + 257]
PLACES = [(n, where) for n in SIZES for where in (("first", "last") if n <= 257 else ("first", "last", "tail"))]


@pytest.mark.parametrize("n,where", PLACES, ids=[f"{n}-{w}" for n, w in PLACES])
def test_sizes_and_where_the_maximum_sits(gpu, n, where):
    """The maximum in the first block, in the last element, and (n > 2048 * 256) in the part of the frame
    only the loop's second trip reads: *d_lwmax is the host's sequential maximum and the image the host's."""
    frame = random_frame(n).copy()
    at = {"first": min(7, n - 1), "last": n - 1, "tail": min(STRIDE + 5, n - 1)}[where]
    frame[at, :3] = (60.0, 70.0, 80.0)
    want = host_max(frame)
    assert want == luminance(frame[at:at + 1])[0] and (where != "tail" or at >= STRIDE)
    lw, argb = device_tonemap(gpu, frame)
    assert lw.view(np.uint32) == want.view(np.uint32), (float(lw), float(want))
    assert np.array_equal(argb, host_argb(gpu, frame))


def test_two_calls_accumulate_into_one_maximum(gpu):
    """Ranks combine by reducing their parts into one zeroed *d_lwmax: two uneven halves give the whole frame's
    result, whichever half holds the maximum; a larger value already there is kept."""
    n, cut = 1000, 437
    for at in (100, 900):
        frame = random_frame(n).copy()
        frame[at, :3] = (60.0, 70.0, 80.0)
        lw, argb = device_tonemap(gpu, frame, parts=[(0, cut), (cut, n - cut)])
        assert lw.view(np.uint32) == host_max(frame).view(np.uint32)
        assert np.array_equal(argb, host_argb(gpu, frame))
    # a preset above the frame's maximum: the host's result for the frame plus one pixel of that luminance
    extra = np.array([[500.0, 500.0, 500.0, 0.0]], dtype=F32)
    preset = luminance(extra)[0]
    frame = random_frame(n)
    assert preset > host_max(frame)
    lw, argb = device_tonemap(gpu, frame, lwmax0=preset)
    assert lw.view(np.uint32) == preset.view(np.uint32)
    assert np.array_equal(argb, host_argb(gpu, np.concatenate([frame, extra]))[:n])


def test_luminance_across_the_exponents(gpu):
    """Grey pixels 2^-149 ... 2^127 (subnormal luminances and products included), coloured ones across the
    same range, exact 0 and -0, in one frame of 4096 pixels."""
    rng = np.random.default_rng(5)
    n = 4096
    e = np.arange(-149, 128)
    frame = np.zeros((n, 4), dtype=F32)
    frame[:len(e), :3] = np.ldexp(1.0, e).astype(F32)[:, None]  # all channels equal
    k = n - len(e) - 8
    frame[len(e):len(e) + k, :3] = np.ldexp(rng.uniform(0.5, 1.0, (k, 3)), rng.integers(-149, 127, (k, 1))).astype(F32)
    frame[-8:-4, :3] = F32(-0.0)
    frame[-2, :3] = (0.0, -0.0, 0.0)
    want = host_max(frame)
    assert np.isfinite(want) and want >= F32(2.0 ** 126)
    lw, argb = device_tonemap(gpu, frame)
    assert lw.view(np.uint32) == want.view(np.uint32)
    assert np.array_equal(argb, host_argb(gpu, frame))


@pytest.mark.parametrize("case", tonemap_edge_frames(), ids=lambda c: c[0])
def test_edge_pixels(gpu, case):
    """NaN, negative and infinite channels, the all-black frame: the host's bits and the hand-derived bytes."""
    name, frame, checks = case
    lw, argb = device_tonemap(gpu, frame)
    assert lw.view(np.uint32) == host_max(frame).view(np.uint32), (name, float(lw))
    assert {"nan": np.isfinite(lw) and lw > 0, "negative": np.isfinite(lw) and lw > 0, "infinite": np.isposinf(lw),
            "black": lw.view(np.uint32) == 0}[name]
    for px, mask, value in checks:
        assert int(argb[px]) & mask == value, (name, px, hex(int(argb[px])))
    assert np.array_equal(argb, host_argb(gpu, frame))
