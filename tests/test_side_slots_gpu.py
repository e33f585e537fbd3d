"""MRT_RF_FOLD_ASYNC with side slots (mrt_context.h kSideSlots): the Cornell walk kernel, whose one-wave
groups fill every SIMD, is launched with fewer groups, and the launch's retrace and fold run in the freed wave
slots on the context's own stream while the caller's stream goes on to the next launch.  Per-path
streams make the result independent of which wave runs a path: every async render here equals the
blocking render of the same descriptor bit for bit, with equal ray totals and an equal handed_over
delta (mrt_kernel_info)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MRT_NPART = 8  # mrt_launch.h
SIDE = 768     # mrt_context.h kSideSlots


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    return mrt


_refs = {}


def blocking(gpu, sid, w, h, spp, nosig=False, **kw):
    """(image, rays, handed_over delta, grid) of the blocking render, computed once per descriptor."""
    key = (sid, w, h, spp, nosig, tuple(sorted(kw.items())))
    if key not in _refs:
        r = gpu.Renderer(gpu.select_scene(sid, w / h), 0)
        h0 = r.kernel_info()["handed_over"]
        img, rays = r.render(gpu.render_desc(w, h, spp, **kw))
        ki = r.kernel_info()
        r.close()
        img.setflags(write=False)
        _refs[key] = (img, rays, ki["handed_over"] - h0, ki["grid"], ki["kernel_features"])
    return _refs[key]


def enqueue(gpu, c, d, stream, rays_d):
    """One MRT_RF_FOLD_ASYNC render of d on `stream`, nothing synchronised: (d, pixel list, device image)."""
    import torch
    px = gpu.local_pixels(d)
    o = torch.zeros((len(px), 4), dtype=torch.float32, device=rays_d.device)
    c.render_device(d, o.data_ptr(), rays_d.data_ptr(), stream.cuda_stream)
    return d, px, o


def image(out):
    d, px, o = out
    im = np.zeros((d.width * d.height, 4), dtype=np.float32)
    im[px] = o.cpu().numpy()
    return im.reshape(d.height, d.width, 4)


def run_async(gpu, c, descs):
    """The descs as MRT_RF_FOLD_ASYNC renders back to back on context c, no host synchronisation
    between them: (images, ray total, handed_over delta, kernel_info after the last)."""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    rays_d = torch.zeros(1, dtype=torch.int64, device=dev)
    h0 = c.kernel_info()["handed_over"]
    outs = [enqueue(gpu, c, d, s, rays_d) for d in descs]
    c.join(s.cuda_stream)
    s.synchronize()
    ki = c.kernel_info()
    return [image(o) for o in outs], int(rays_d.item()), ki["handed_over"] - h0, ki


def same(a, b):
    return np.array_equal(a[..., :3].view(np.uint32), b[..., :3].view(np.uint32))


def adesc(gpu, w, h, spp, **kw):
    return gpu.render_desc(w, h, spp, flags=gpu._lib.RF_FOLD_ASYNC, **kw)


@pytest.mark.parametrize("chunk", [64, 0], ids=["three_launches", "one_launch"])
@pytest.mark.parametrize("numerics", ["fast", "exact"])
@pytest.mark.parametrize("mode", [0, 1])
def test_async_back_to_back(gpu, mode, numerics, chunk):
    """Scene 5 at 250x250x192 (a few hundred listed paths per render under the tolerance contract),
    three renders back to back on one context: in three launches each (both radiance parities and
    both lists in use) and in one."""
    w, h, spp = 250, 250, 192
    kw = dict(numerics=numerics, mode=mode, chunk_samples=chunk)
    ref, rays, listed, _, _ = blocking(gpu, 5, w, h, spp, **kw)
    assert (listed > 0) == (numerics == "fast")
    c = gpu.Renderer(gpu.select_scene(5, 1.0), 0)
    imgs, arays, alisted, _ = run_async(gpu, c, [adesc(gpu, w, h, spp, **kw)] * 3)
    c.close()
    assert arays == 3 * rays and alisted == 3 * listed
    assert all(same(im, ref) for im in imgs)


@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (8, 8, 4), (63, 1, 1), (64, 1, 1), (65, 1, 1), (129, 1, 1)])
def test_fewer_paths_than_waves(gpu, w, h, spp):
    """Launches with fewer paths than the reduced grid has waves (one path; an 8x8x4 image; 63, 64, 65
    and 129 paths through one-row images): most waves find their partition handed out at their static
    claim."""
    ref, rays, listed, _, _ = blocking(gpu, 5, w, h, spp, numerics="fast")
    c = gpu.Renderer(gpu.select_scene(5, w / h), 0)
    imgs, arays, alisted, _ = run_async(gpu, c, [adesc(gpu, w, h, spp, numerics="fast")] * 2)
    c.close()
    assert arays == 2 * rays and alisted == 2 * listed
    assert all(same(im, ref) for im in imgs)


def test_dynamic_claims_on_reduced_partitions(gpu):
    """A launch just above (grid - R) x 64 x MRT_BATCH paths: no static first claim (the host's
    static_first is false), every claim from the counters of partitions sized for the reduced grid --
    while the blocking render's full grid still deals its first claims statically."""
    w = h = 500
    c = gpu.Renderer(gpu.select_scene(5, 1.0), 0)
    _, _, _, ki = run_async(gpu, c, [adesc(gpu, 8, 8, 1, numerics="fast")])
    full = 32 * ki["n_cu"]
    assert ki["grid"] < full
    chunk = ki["grid"] * 64 * 256 // (w * h) + 1
    assert chunk * w * h < full * 64 * 256
    spp = int(np.ceil(np.sqrt(chunk))) ** 2  # two launches: `chunk` samples and the rest
    kw = dict(numerics="fast", chunk_samples=chunk)
    ref, rays, listed, _, _ = blocking(gpu, 5, w, h, spp, **kw)
    imgs, arays, alisted, _ = run_async(gpu, c, [adesc(gpu, w, h, spp, **kw)])
    c.close()
    assert arays == rays and alisted == listed and listed > 0
    assert same(imgs[0], ref)


VARIANTS = [  # (scene, MRT_NO_SIG, kernel variant, w, h, spp)
    (5, True, 10248, 128, 128, 64),    # the linear-program interpreter on the Cornell box
    (9, False, 141314, 128, 128, 64),  # room + mesh
    (9, True, 10274, 128, 128, 64),    # room + mesh through the interpreter
]


@pytest.mark.parametrize("sid,nosig,variant,w,h,spp", VARIANTS, ids=[str(v[2]) for v in VARIANTS])
def test_other_retrace_variants_keep_grid(gpu, monkeypatch, sid, nosig, variant, w, h, spp):
    """One async render (two launches) per scene whose kernel variant has a retrace kernel beside the
    Cornell walk's, each at a size where the blocking render lists at least one path (40, 36 and 36).
    These kernels keep their grids under MRT_RF_FOLD_ASYNC and their retrace its registers and its
    place on the render's stream; only the Cornell walk's launches leave side slots."""
    if nosig:
        monkeypatch.setenv("MRT_NO_SIG", "1")
    kw = dict(numerics="fast", chunk_samples=spp // 2)
    ref, rays, listed, grid, kf = blocking(gpu, sid, w, h, spp, nosig=nosig, **kw)
    print("variant", kf, "listed", listed)
    assert kf == variant and listed > 0
    c = gpu.Renderer(gpu.select_scene(sid, w / h), 0)
    imgs, arays, alisted, ki = run_async(gpu, c, [adesc(gpu, w, h, spp, **kw)])
    c.close()
    assert arays == rays and alisted == listed and ki["grid"] == grid
    assert same(imgs[0], ref)


def test_async_then_blocking_and_cast_in_flight(gpu):
    """An async render followed on the same context, with no host synchronisation in between, by ray
    queries on its stream (mrt_cast_rays_device), a blocking render and a second async render: the
    retrace and the fold of the async render's last launches are still on the context's stream when
    each of them is enqueued.  The blocking render reuses both radiance buffers and both lists, so it
    has to wait for both folds (and the retraces in front of them); the ray queries share nothing with
    them.  Everything is joined and compared at the end only."""
    import torch
    w, h, spp = 250, 250, 192
    kw = dict(numerics="fast", chunk_samples=64)
    ref, rays, listed, _, _ = blocking(gpu, 5, w, h, spp, **kw)
    q = np.zeros(257, dtype=gpu.RAY_DTYPE)
    q["o"] = (278.0, 278.0, -800.0)
    q["d"][:, 0] = np.linspace(-0.3, 0.3, len(q))
    q["d"][:, 1] = np.linspace(0.3, -0.3, len(q))
    q["d"][:, 2] = 1.0
    q["tmax"] = np.inf
    r0 = gpu.Renderer(gpu.select_scene(5, 1.0), 0)
    hits0 = r0.cast_rays(q)
    r0.close()
    assert np.isfinite(hits0["t"]).any()
    dev = torch.device("cuda", 0)
    c = gpu.Renderer(gpu.select_scene(5, 1.0), 0)
    d = adesc(gpu, w, h, spp, **kw)
    c.prepare(d)
    d_q = torch.from_numpy(q.view(np.uint8).copy()).to(dev)
    d_hits = [torch.zeros(len(q) * 32, dtype=torch.uint8, device=dev) for _ in range(2)]
    rays_d = torch.zeros(1, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    h0 = c.kernel_info()["handed_over"]
    first = enqueue(gpu, c, d, s, rays_d)
    c.cast_rays_device(d_q.data_ptr(), len(q), d_hits[0].data_ptr(), stream_ptr=s.cuda_stream)
    img, brays = c.render(gpu.render_desc(w, h, spp, **kw))  # (waits for its own end only)
    second = enqueue(gpu, c, d, s, rays_d)
    c.cast_rays_device(d_q.data_ptr(), len(q), d_hits[1].data_ptr(), stream_ptr=s.cuda_stream)
    c.join(s.cuda_stream)
    s.synchronize()
    alisted = c.kernel_info()["handed_over"] - h0
    c.close()
    assert int(rays_d.item()) == 2 * rays and brays == rays and alisted == 3 * listed
    assert same(image(first), ref) and same(img, ref) and same(image(second), ref)
    for dh in d_hits:
        assert dh.cpu().numpy().tobytes() == hits0.tobytes()


def test_async_shapes_alternating(gpu):
    """Async renders of two shapes alternating on one context, a, b, a, b, b, a enqueued back to back
    with no host synchronisation: each change of shape re-lays the workspace out while the retrace and
    the fold of the render before it are still on the context's stream, and has to wait for them
    (quiesce: ev_done is recorded on that stream behind both)."""
    a = (250, 250, 192, dict(numerics="fast", chunk_samples=64))
    b = (96, 96, 16, dict(numerics="fast", chunk_samples=0))  # (square like a: one scene, one camera)
    order = [a, b, a, b, b, a]
    refs = {id(x): blocking(gpu, 5, x[0], x[1], x[2], **x[3]) for x in (a, b)}
    c = gpu.Renderer(gpu.select_scene(5, 1.0), 0)
    imgs, arays, alisted, _ = run_async(gpu, c, [adesc(gpu, w, h, spp, **kw) for w, h, spp, kw in order])
    c.close()
    assert arays == sum(refs[id(x)][1] for x in order)
    assert alisted == sum(refs[id(x)][2] for x in order)
    for x, im in zip(order, imgs):
        assert same(im, refs[id(x)][0])


def test_grid_accounting(gpu):
    """kernel_info()["grid"]: under MRT_RF_FOLD_ASYNC the fast Cornell kernel (eight waves per SIMD, every
    slot taken) runs the full grid minus the side slots, a multiple of MRT_NPART; a blocking render on
    the same context reports the full grid again, and the exact contract's kernel keeps its grid under
    MRT_RF_FOLD_ASYNC."""
    c = gpu.Renderer(gpu.select_scene(5, 1.0), 0)
    _, _, _, ki = run_async(gpu, c, [adesc(gpu, 8, 8, 1, numerics="fast")])
    full = 32 * ki["n_cu"]
    side = min(SIDE, full // 2) // MRT_NPART * MRT_NPART
    assert ki["wg"] == 64 and side > 0 and side % MRT_NPART == 0
    assert ki["grid"] == full - side
    c.render(gpu.render_desc(8, 8, 1, numerics="fast"))
    assert c.kernel_info()["grid"] == full
    exact = c.render(gpu.render_desc(8, 8, 1, numerics="exact")) and c.kernel_info()["grid"]
    _, _, _, ki = run_async(gpu, c, [adesc(gpu, 8, 8, 1, numerics="exact")])
    assert ki["grid"] == exact
    # fewer than kSideMinBounces = 4 bounces: the full grid (the launch is too short for its fold)
    _, _, _, ki = run_async(gpu, c, [adesc(gpu, 8, 8, 1, numerics="fast", depth=3)])
    assert ki["grid"] == full
    _, _, _, ki = run_async(gpu, c, [adesc(gpu, 8, 8, 1, numerics="fast", depth=4)])
    assert ki["grid"] == full - side
    c.close()


@pytest.mark.parametrize("depth", [1, 3, 4])
def test_async_depth_limits_around_the_gate(gpu, depth):
    """Depth limits below and at kSideMinBounces, side slots off and on, alternating with the default
    depth on one context with nothing synchronised in between: a launch without side slots (retrace on
    the render's stream, fold in 256-thread groups) follows one with them and the other way round."""
    w, h, spp = 250, 250, 192
    lo = dict(numerics="fast", chunk_samples=64, depth=depth)
    hi = dict(numerics="fast", chunk_samples=64)
    rl, rh = blocking(gpu, 5, w, h, spp, **lo), blocking(gpu, 5, w, h, spp, **hi)
    c = gpu.Renderer(gpu.select_scene(5, 1.0), 0)
    imgs, arays, alisted, _ = run_async(gpu, c, [adesc(gpu, w, h, spp, **k) for k in (lo, hi, lo, hi)])
    c.close()
    assert arays == 2 * (rl[1] + rh[1]) and alisted == 2 * (rl[2] + rh[2])
    assert same(imgs[0], rl[0]) and same(imgs[1], rh[0]) and same(imgs[2], rl[0]) and same(imgs[3], rh[0])
