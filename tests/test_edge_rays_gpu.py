"""The exact contract's range guards on the MI355X (DESIGN.md "Numerics", the guard inventory):
mrt_cast_rays_device on the edge-operand rays of tests/edge_rays.py against the CPU backend's cast of
the same batch with the same seed, bit for bit (a NaN equals a NaN).  test_edge_rays_host.py pins that
cast to the C restatement and to the reference's own hits, so nothing here loops over oracle.hit.

On the device recip_nr is v_rcp_f32 + a Newton step and sqrt_core is v_sqrt_f32 + a neighbour test, exact
only inside operand ranges; outside them every site takes an IEEE form behind a wave ballot and a
per-lane select.  So every batch is cast in three wave compositions (edge_rays.arrangements): whole
64-ray groups of one class, one edge ray among 63 ordinary ones at lane 0 / 31 / 32 / 63, and a seeded
shuffle; and at lengths 1, 63, 65.  Batches of at most 4096 rays.

The non-finite class (NaN / inf operands, a zero direction) has the file's last test."""
import numpy as np
import pytest

import edge_rays as er
from test_cast_gpu import SENTINEL, device_cast
from test_cast_host import BY_NAME, EXTRA, NO_HIT, PER_VARIANT, miss_words, words
from test_edge_rays_host import FIXTURE_SCENES, batch, degenerate_normals, mesh_rays, slowdiv_case, view_of
from test_synthetic_scenes import GEN, NOBVHW, NOSIG, V_GENERIC

pytestmark = pytest.mark.gpu
GPU_KEYS = [f"scene_{sid}" for sid in FIXTURE_SCENES] + [n for n in PER_VARIANT + EXTRA if BY_NAME[n].gpu]
HOOKED = [("a_cornell_plus_sphere", GEN), ("b_cornell_lookalike", NOSIG), ("j_tree_list_leaves", NOBVHW), ("c_room_mesh_lookalike", NOSIG)]


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def differing(got, want):
    """Rows whose records differ: any word, except float words that are NaN on both sides."""
    a, b = words(got), words(want)
    fa, fb = a[:, :7].view(np.float32), b[:, :7].view(np.float32)
    return ~(((a[:, :7] == b[:, :7]) | (np.isnan(fa) & np.isnan(fb))).all(axis=1) & (a[:, 7] == b[:, 7]))


def assert_device_equals_cpu(what, r_gpu, r_cpu, rays, labels, seed=0):
    got, tail, back = device_cast(r_gpu, rays, seed=seed)
    want = r_cpu.cast_rays(rays, seed=seed)
    bad = differing(got, want)
    per_class = {str(c): (int(bad[labels == c].sum()), int((labels == c).sum())) for c in sorted(set(labels))}
    hits = int((words(want)[:, 7] != NO_HIT).sum())
    print(f"{what}: {len(rays)} rays, {hits} hit on the CPU backend, {int(bad.sum())} differ; differing / rays per class {per_class}")
    assert not bad.any(), (what, per_class, [int(i) for i in np.nonzero(bad)[0][:8]])
    assert (tail == SENTINEL).all() and back.tobytes() == rays.tobytes()
    miss = words(got)[:, 7] == NO_HIT
    assert np.array_equal(words(got)[miss], miss_words(int(miss.sum())))
    return got


def cast_all_arrangements(what, r_gpu, r_cpu, rays, labels):
    """The three wave compositions and the ragged lengths; seeds follow the index within each batch,
    and the CPU backend casts the same arrangement."""
    for name, idx in er.arrangements(labels, 17).items():
        if len(idx):
            assert len(idx) <= er.LIMIT
            assert_device_equals_cpu(f"{what} [{name}]", r_gpu, r_cpu, rays[idx], labels[idx])
    order = np.argsort(labels, kind="stable")
    for n in (1, 63, 65):
        # from the first ray of an edge class: the short batch is all edge rays
        at = int(np.nonzero(labels[order] != "ordinary")[0][0])
        assert_device_equals_cpu(f"{what} [{n} rays]", r_gpu, r_cpu, rays[order][at:at + n], labels[order][at:at + n], seed=at)


# ---------------------------------------------------------------- 1. scenes and kernel variants
@pytest.mark.parametrize("key", GPU_KEYS)
def test_device_cast_of_edge_rays_equals_cpu_backend(gpu, key):
    sc, rays, labels = batch(gpu, key)
    r, c = gpu.Renderer(sc, 0), gpu.Renderer(sc, "cpu")
    if key in BY_NAME:
        assert r.kernel_info()["kernel_features"] == BY_NAME[key].kernel, hex(r.kernel_info()["kernel_features"])
    cast_all_arrangements(key, r, c, rays, labels)
    r.close()
    c.close()


@pytest.mark.parametrize("name,hook", HOOKED)
def test_device_cast_of_edge_rays_under_upload_hooks(gpu, monkeypatch, name, hook):
    """The same from the kernel variant an upload hook selects instead."""
    e = BY_NAME[name]
    assert hook in e.hooks
    sc, rays, labels = batch(gpu, name)
    with monkeypatch.context() as mp:
        mp.setenv(hook, "1")
        r = gpu.Renderer(sc, 0)
    c = gpu.Renderer(sc, "cpu")
    assert r.kernel_info()["kernel_features"] != e.kernel or hook == NOBVHW, hook
    cast_all_arrangements(f"{name} {hook}", r, c, rays, labels)
    r.close()
    c.close()


# ---------------------------------------------------------------- 2. rects on slow-division planes, degenerate normals
@pytest.mark.parametrize("hook", [None, GEN])
def test_device_rects_on_slowdiv_planes(gpu, orc, monkeypatch, hook):
    """MRT_F_SLOWDIV rects beside ordinary ones in one list, origins on and beside the planes and
    above 2^60: the lin walk's rect test (mrt_lin.h lin_prim_t) and the generic walk's (rect_hit)."""
    s, rays, labels, _, _ = slowdiv_case(gpu, orc)
    with monkeypatch.context() as mp:
        if hook:
            mp.setenv(hook, "1")
        r = gpu.Renderer(s, 0)
    kf = r.kernel_info()["kernel_features"]
    print(f"slowdiv rects [{hook}]: kernel {kf:#x}")
    assert (kf == V_GENERIC) == (hook == GEN)
    c = gpu.Renderer(s, "cpu")
    cast_all_arrangements(f"slowdiv rects {hook}", r, c, rays, labels)
    r.close()
    c.close()


def test_device_degenerate_mesh_normals(gpu):
    """mesh_leaf's normalize on vertex normals that sum to 0, ~1e-30 and ~1e25: its IEEE fallback."""
    s = degenerate_normals(gpu)
    rays = mesh_rays(gpu, s, 31)
    r, c = gpu.Renderer(s, 0), gpu.Renderer(s, "cpu")
    got = assert_device_equals_cpu("degenerate normals", r, c, rays, np.full(len(rays), "mesh"))
    n = got["n"][got["mat"] != NO_HIT]
    assert np.isnan(n).any(axis=1).sum() >= 32
    r.close()
    c.close()


# ---------------------------------------------------------------- 3. graph capture
def test_captured_cast_of_edge_rays_replays_bit_equal(gpu):
    """One captured replay of the class-sorted edge batch of scene 5 equals the uncaptured call."""
    import torch
    sc, rays, labels = batch(gpu, "scene_5")
    rays = rays[np.argsort(labels, kind="stable")]
    r = gpu.Renderer(sc, 0)
    plain, _, _ = device_cast(r, rays, seed=9)
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.full((n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        r.cast_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), seed=9, stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_hits.cpu().numpy() == SENTINEL).all()  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert d_hits.cpu().numpy().tobytes() == plain.tobytes()
    del graph
    r.close()


# ---------------------------------------------------------------- 4. the non-finite class (last)
@pytest.mark.parametrize("key", ["scene_5", "scene_7", "scene_8", "n_bvh_with_instance_leaf"])
def test_device_cast_of_non_finite_rays(gpu, key):
    """"No ray is rejected" (include/mrt.h): NaN / inf operands and a zero direction yield the CPU
    backend's records.  The cast path computes no index, loop bound or stack depth from a ray's floats:
    the walks push at most one entry per graph or tree level whatever the box tests answer, node and
    triangle indices come from the tables, and the direction mask reads sign bits only (read before
    this test's first run: cast_one, scene_hit / scene_hit_lin / scene_hit_sig, mesh_hit, bvhw_hit)."""
    sc, syn = view_of(gpu, key)
    rays, labels = er.nonfinite_rays(gpu, syn, 99)
    fill, fl = batch(gpu, key)[1:]
    keep = np.nonzero(fl == "ordinary")[0][:256]
    rays, labels = np.concatenate([rays, fill[keep]]), np.concatenate([labels, fl[keep]])
    assert len(rays) <= 512
    r, c = gpu.Renderer(sc, 0), gpu.Renderer(sc, "cpu")
    for name, idx in er.arrangements(labels, 5).items():
        if name != "lone":
            assert_device_equals_cpu(f"{key} non-finite [{name}]", r, c, rays[idx], labels[idx])
    r.close()
    c.close()
