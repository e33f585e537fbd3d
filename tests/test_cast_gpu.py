"""Ray queries (include/mrt.h "ray queries") on the MI355X: mrt_cast_rays_device against the
reference's own closest hits, the CPU backend and the C restatement, bit for bit; ragged batch sizes;
stream order beside renders; one graph capture; the blocking form.  Batches of at most 2048 rays."""
import numpy as np
import pytest

from conftest import SCENE_SIZES
from test_aux_host import ref_scene
from test_cast_host import (BY_NAME, ENTRIES, NO_HIT, assert_equals_fixture, assert_equals_restatement, bits, cpu_full, entry_reference,
                            fixture, miss_words, tmax_cases, words)
from test_synthetic_scenes import GEN, NOBVHW, NOSIG, built

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def device_cast(r, rays, seed=0, stream=None, extra=1):
    """cast_rays_device of a RAY_DTYPE array on `stream` (default: a new side stream): the n records as
    HIT_DTYPE, the `extra` records behind them as bytes, and the ray buffer read back."""
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    d_hits = torch.full(((n + extra) * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = stream if stream is not None else torch.cuda.Stream()
    torch.cuda.synchronize()
    r.cast_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), seed=seed, stream_ptr=st.cuda_stream)
    st.synchronize()
    out = d_hits.cpu().numpy()
    from miniraytracer_amd import HIT_DTYPE
    return out[:n * 32].view(HIT_DTYPE), out[n * 32:], d_rays.cpu().numpy().view(rays.dtype)


_gpu = {}


def gpu_renderer(mrt, sid):
    if sid not in _gpu:
        _gpu[sid] = mrt.Renderer(fixture(mrt, sid)[0], 0)
    return _gpu[sid]


# ---------------------------------------------------------------- 1. the fixtures
@pytest.mark.parametrize("sid", sorted(SCENE_SIZES))
def test_device_cast_equals_reference_hits_and_cpu_backend(gpu, sid):
    _, rays, hit, tpn = fixture(gpu, sid)
    got, tail, back = device_cast(gpu_renderer(gpu, sid), rays)
    assert_equals_fixture(sid, got, hit, tpn)
    assert np.array_equal(words(got), words(cpu_full(gpu, sid)))
    assert (tail == SENTINEL).all()
    assert back.tobytes() == rays.tobytes()


# ---------------------------------------------------------------- 2. ragged sizes
@pytest.mark.parametrize("n", [1, 63, 65, 2047])
def test_exactly_n_records_are_written(gpu, n):
    _, rays, _, _ = fixture(gpu, 7)
    got, tail, _ = device_cast(gpu_renderer(gpu, 7), rays[:n], extra=65)
    assert np.array_equal(words(got), words(cpu_full(gpu, 7))[:n])
    assert (tail == SENTINEL).all()


def test_device_arguments(gpu):
    import torch
    r = gpu_renderer(gpu, 5)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    r.cast_rays_device(0, 0, 0)  # n == 0: nothing enqueued, null pointers are fine
    for rays_ptr, hits_ptr in ((0, p), (p, 0), (p + 4, p + 2048), (p, p + 2048 + 8)):
        with pytest.raises(gpu.MrtError):
            r.cast_rays_device(rays_ptr, 4, hits_ptr)
    torch.cuda.synchronize()
    assert not buf.any()


# ---------------------------------------------------------------- 3. the synthetic catalogue
@pytest.mark.parametrize("e", [e for e in ENTRIES if e.gpu], ids=lambda e: e.name)
def test_catalogue_device_cast_equals_restatement(gpu, orc, e):
    s, rays, want, flag = entry_reference(gpu, orc, e)
    r = gpu.Renderer(s, 0)
    assert r.kernel_info()["kernel_features"] == e.kernel, (hex(r.kernel_info()["kernel_features"]), hex(e.kernel))
    got, tail, _ = device_cast(r, rays)
    r.close()
    assert_equals_restatement(s, got, want, flag)
    assert (tail == SENTINEL).all()


@pytest.mark.parametrize("name,hook", [("a_cornell_plus_sphere", GEN), ("b_cornell_lookalike", NOSIG), ("j_tree_list_leaves", NOBVHW)])
def test_catalogue_device_cast_under_upload_hooks(gpu, orc, monkeypatch, name, hook):
    """The same records from the kernel variant an upload hook selects instead."""
    e = BY_NAME[name]
    assert hook in e.hooks
    s, rays, want, flag = entry_reference(gpu, orc, e)
    with monkeypatch.context() as mp:
        mp.setenv(hook, "1")
        r = gpu.Renderer(s, 0)
    assert r.kernel_info()["kernel_features"] != e.kernel or hook == NOBVHW, hook
    got, _, _ = device_cast(r, rays)
    r.close()
    assert_equals_restatement(s, got, want, flag)


# ---------------------------------------------------------------- 4. tmax and split batches
@pytest.mark.parametrize("sid", [5, 7])
def test_device_tmax_rule(gpu, sid):
    _, rays, _, _ = fixture(gpu, sid)
    r = gpu_renderer(gpu, sid)
    for label, whole, at, want in tmax_cases(rays, cpu_full(gpu, sid)):
        got, _, _ = device_cast(r, whole)
        assert np.array_equal(words(got)[at], want), label


@pytest.mark.parametrize("sid", [6, 7])
def test_device_split_batch_equals_the_whole(gpu, sid):
    _, rays, _, _ = fixture(gpu, sid)
    full = words(cpu_full(gpu, sid))
    r = gpu_renderer(gpu, sid)
    for k in (1, 63, 64, 2047):
        got, _, _ = device_cast(r, rays[k:], seed=k)
        assert np.array_equal(words(got), full[k:]), k


# ---------------------------------------------------------------- 5. stream order with a render
@pytest.mark.parametrize("numerics", ["exact", "fast"])
def test_cast_between_two_renders_on_one_stream(gpu, numerics):
    """render, cast, render on one stream: both images and ray totals are a lone render's, the
    records a lone cast's."""
    import torch
    _, rays, _, _ = fixture(gpu, 5)
    r = gpu.Renderer(ref_scene(gpu, 5), 0)
    d = gpu.render_desc(48, 48, 16, numerics=numerics)
    n_local = len(gpu.local_pixels(d))
    r.prepare(d)
    st = torch.cuda.Stream()

    def buffers():
        return torch.full((n_local, 4), -1.0, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

    img0, rays0 = buffers()
    torch.cuda.synchronize()
    r.render_device(d, img0.data_ptr(), rays0.data_ptr(), st.cuda_stream)
    r.join(st.cuda_stream)
    st.synchronize()
    lone, _, _ = device_cast(r, rays)
    (img1, rays1), (img2, rays2) = buffers(), buffers()
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.full((len(rays) * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.render_device(d, img1.data_ptr(), rays1.data_ptr(), st.cuda_stream)
    r.cast_rays_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), stream_ptr=st.cuda_stream)
    r.render_device(d, img2.data_ptr(), rays2.data_ptr(), st.cuda_stream)
    r.join(st.cuda_stream)
    st.synchronize()
    want = bits(img0.cpu().numpy())
    assert int(rays0.item()) > 0 and (want != bits(np.full(1, -1.0, np.float32))[0]).any()
    for img, nr in ((img1, rays1), (img2, rays2)):
        assert np.array_equal(bits(img.cpu().numpy()), want) and int(nr.item()) == int(rays0.item())
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint32).reshape(-1, 8), words(lone))
    assert np.array_equal(words(lone), words(cpu_full(gpu, 5)))
    r.close()


# ---------------------------------------------------------------- 6. graph capture
def test_captured_cast_replays_on_the_buffer_s_contents(gpu):
    """One cast_rays_device captured on a side stream; each replay casts what the ray buffer then holds."""
    import torch
    _, rays, _, _ = fixture(gpu, 7)
    r = gpu_renderer(gpu, 7)
    n = 1000
    first, second = rays[:n], rays[n:2 * n]
    host = [words(r.cast_rays(q, seed=5)) for q in (first, second)]
    d_rays = torch.from_numpy(first.view(np.uint8).copy()).cuda()
    d_hits = torch.full((n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    r.cast_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), seed=5, stream_ptr=side.cuda_stream)  # once outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        r.cast_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), seed=5, stream_ptr=torch.cuda.current_stream().cuda_stream)
    for q, want in ((second, host[1]), (first, host[0])):
        d_rays.copy_(torch.from_numpy(q.view(np.uint8).copy()))
        d_hits.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_hits.cpu().numpy().view(np.uint32).reshape(-1, 8), want)
    assert not np.array_equal(host[0], host[1])
    del graph


# ---------------------------------------------------------------- 7. the blocking form
@pytest.mark.parametrize("sid", [5, 7])
def test_blocking_cast_on_a_gpu_scene_equals_the_device_form(gpu, sid):
    _, rays, _, _ = fixture(gpu, sid)
    r = gpu_renderer(gpu, sid)
    got, _, _ = device_cast(r, rays, seed=3)
    assert np.array_equal(words(r.cast_rays(rays, seed=3)), words(got))
    assert np.array_equal(words(r.cast_rays(rays[:65], seed=3)), words(got)[:65])  # a smaller batch reuses the staging records
    assert (words(got)[:, 7] == NO_HIT).any() and np.array_equal(words(got)[words(got)[:, 7] == NO_HIT], miss_words(int((words(got)[:, 7] == NO_HIT).sum())))
