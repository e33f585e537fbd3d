"""The tolerance contract's path kernel may reschedule a path's work -- run a scatter later at a wider
lane mask, test the light once per ray instead of twice -- but never change a path: every path has its
own stream, so its radiance and its ray count are a function of the path alone.

1. Same bits as the parent commit: tools/fast_path_digest.py's cases (scene 5 at sizes down to one
   path, depth limits 1 and 2, both modes; a glass-heavy scene in which every lane of a wave meets
   glass at once and paths bounce inside it; scene 5 with another rect than the light as the biased
   object, where the light pdf cannot reuse the walk's light test) against
   tests/golden/fastpaths_parent.json, the tool's output on the parent commit's build.
2. Schedule independence, no fixture: the per-path radiance and ray counts of one launch equal those
   of a pixel-list render of a third of the pixels and of the three shards of world 3 (other paths
   share the wave, other lanes hold the path); the same render in sample chunks gives the same image
   and ray total (MRT_RF_PATH_DEBUG keeps a render in one launch, so chunks compare the fold's output).
"""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("fast_path_digest", os.path.join(ROOT, "tools", "fast_path_digest.py"))
fpd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fpd)

with open(os.path.join(GOLDEN, "fastpaths_parent.json")) as _f:
    PARENT = json.load(_f)


def test_fixture_lists_every_case():
    assert sorted(PARENT) == sorted(c[0] for c in fpd.CASES)


@pytest.mark.parametrize("case", fpd.CASES, ids=[c[0] for c in fpd.CASES])
def test_same_bits_as_parent(mrt, case):
    got = fpd.digest_case(mrt, case)
    print(case[0], got)
    if case[1] in ("glass", "offlight"):  # still the Cornell fast walk's kernel
        assert got["kernel_features"] == fpd.V_CORNELL, hex(got["kernel_features"])
    assert got == PARENT[case[0]]


_full = {}


def full_render(mrt, sid):
    """(renderer, per-path radiance, per-path rays, ray total) of sid at 64x64x16, fast, one launch."""
    if sid not in _full:
        r = mrt.Renderer(fpd.scene_of(mrt, sid, 1.0), 0)
        rgb, rays, total, _ = fpd.render_paths(mrt, r, W, W, SPP)
        rgb.setflags(write=False)
        rays.setflags(write=False)
        _full[sid] = (r, rgb, rays, total)
    return _full[sid]


W, SPP = 64, 16
SCENES = [5, "glass"]


@pytest.mark.parametrize("sid", SCENES, ids=str)
def test_pixel_list_same_paths(mrt, sid):
    r, rgb, rays, _ = full_render(mrt, sid)
    px = np.sort(np.random.default_rng(7).choice(W * W, size=W * W // 3, replace=False)).astype(np.uint32)
    prgb, prays, total, got_px = fpd.render_paths(mrt, r, W, W, SPP, pixels=px)
    assert np.array_equal(np.sort(got_px), px)
    assert np.array_equal(prgb[px].view(np.uint32), rgb[px].view(np.uint32))
    assert np.array_equal(prays[px], rays[px])
    assert total == int(rays[px].sum())


@pytest.mark.parametrize("sid", SCENES, ids=str)
def test_world3_shards_same_paths(mrt, sid):
    r, rgb, rays, total = full_render(mrt, sid)
    owned = np.zeros(W * W, dtype=np.int32)
    shard_total = 0
    for rank in range(3):
        prgb, prays, t, px = fpd.render_paths(mrt, r, W, W, SPP, tile_size=16, rank=rank, world=3)
        owned[px] += 1
        shard_total += t
        assert np.array_equal(prgb[px].view(np.uint32), rgb[px].view(np.uint32)), rank
        assert np.array_equal(prays[px], rays[px]), rank
    assert (owned == 1).all()
    assert shard_total == total


@pytest.mark.parametrize("sid", SCENES, ids=str)
def test_sample_chunks_same_image(mrt, sid):
    r, _, _, total = full_render(mrt, sid)
    one, rays1 = r.render(mrt.render_desc(W, W, SPP, numerics="fast"))
    chunked, rays2 = r.render(mrt.render_desc(W, W, SPP, numerics="fast", chunk_samples=5))
    assert rays1 == rays2 == total
    assert np.array_equal(one.view(np.uint32), chunked.view(np.uint32))
