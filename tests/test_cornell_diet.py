"""The Cornell walk's loop skeleton trimmed: the refill's claim in 32 bits on the scalar unit
(mrt_launch.h pool_claim32) and the radiance buffer's address held for the launch instead of loaded
where a path ends.  A path's operations, their order, its stream positions and the address of its
three words stay what they were.

On the GPU, tools/cornell_diet_digest.py's cases against tests/golden/cornell_diet_parent.json,
recorded with that tool from the library of the commit before this test: a material of its own on every
wall and box face with the box's rotation negated, and the lambertian sphere (identity 13) at 64x64x16,
each also under depth limits 1 and 2 (a scatter followed at once by the path's end); another rect as the
biased object (the pdf's leaf path); 1, 63, 64, 65 and 129 paths; one-row images 1 to 65 pixels wide; two
renders in a row on one renderer; the glass-heavy scene (all 64 lanes in the glass branch); ragged path
counts around partition edges (8 k - 1, 8 k + 1, 8460), below 64 per partition and below one claim; two
launches with more paths than the waves' static claims cover (2099601 = 8 k + 1 paths, all of them tail
zone; 6759999 = 8 k - 1 paths, whose partitions hand out full claims first and small ones from the tail
zone's edge), where the partitions' counters serve claims; launches of 4 samples with s0 > 0; a pixel
list; and three of the cases through the interpreter's queue kernel.  Per path radiance bits, per path
ray counts (stored beside the radiance) and the ray total must be the parent's exactly.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


cdd = _tool("cornell_diet_digest")
fpd = cdd.fpd

with open(os.path.join(ROOT, "tests", "golden", "cornell_diet_parent.json")) as _f:
    PARENT = json.load(_f)

WAVES = 32 * 256  # one-wave groups of a 256-CU launch (tests/test_cornell_store.py pins 32 per CU)
BATCH, NPART = 256, 8  # mrt_launch.h MRT_BATCH, MRT_NPART


def _kernel(case):
    return cdd.V_INTERP if case[7] else fpd.V_CORNELL


def test_fixture_lists_every_case():
    assert sorted(PARENT) == sorted(c[0] for c in cdd.CASES)
    for c in cdd.CASES:
        e = PARENT[c[0]]
        # the fixture itself ran the kernels it is about
        assert e["kernel_features"] == _kernel(c), (c[0], hex(e["kernel_features"]))
        assert [r["depth"] for r in e["renders"]] == list(c[5])
        for r in e["renders"]:
            assert r["rays"] >= cdd.n_paths(c)  # at least the camera ray of every path
            assert ("image_sha256" in r) == bool(c[6])


def test_fixture_covers_the_issue_cases():
    names = set(PARENT)
    by = {c[0]: c for c in cdd.CASES}
    # part 2
    assert {"walls", "walls_d1", "walls_d2", "sphere", "sphere_d1", "sphere_d2", "offlight"} <= names
    assert by["sphere"][2:5] == (64, 64, 16) and by["walls_d1"][5] == (1,) and by["sphere_d2"][5] == (2,)
    # parts 3 and 4
    assert {f"paths_{n}" for n in (1, 63, 64, 65, 129)} <= names
    assert [cdd.n_paths(by[f"paths_{n}"]) for n in (1, 63, 64, 65, 129)] == [1, 63, 64, 65, 129]
    rows = [by[n] for n in names if n.startswith("rows_w")]
    assert all(c[3] == 1 for c in rows) and {1, 65} <= {c[2] for c in rows} and all(1 <= c[2] <= 65 for c in rows)
    assert by["pair"][5] == (32, 2) and "glass" in names
    # the pair's first render is the render a fresh renderer makes
    assert PARENT["pair"]["renders"][0] == PARENT["paths_65"]["renders"][0]
    # part 5
    assert cdd.n_paths(by["ragged_8191"]) % 8 == 7 and cdd.n_paths(by["ragged_8193"]) % 8 == 1
    assert cdd.n_paths(by["ragged_8460"]) % (NPART * BATCH) != 0
    assert cdd.n_paths(by["ragged_500"]) < 64 * NPART and cdd.n_paths(by["ragged_200"]) < BATCH
    # more paths than the static claims cover: the counters hand out claims ...
    assert cdd.n_paths(by["dyn_8k1"]) > WAVES * BATCH and cdd.n_paths(by["dyn_8k1"]) % 8 == 1
    # ... and a partition holds more than its static claims and its tail zone (2 claims per wave): full claims first
    assert cdd.n_paths(by["dyn_8km1"]) > 3 * WAVES * BATCH and cdd.n_paths(by["dyn_8km1"]) % 8 == 7
    assert by["chunked"][6] == 4 and by["chunked"][4] > 4 and len(by["pixel_list"][8]) == 5
    assert len([n for n in names if n.startswith("nosig_")]) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", cdd.CASES, ids=[c[0] for c in cdd.CASES])
def test_same_bits_as_parent(mrt, case):
    got = cdd.digest_case(mrt, case)
    print(case[0], got)
    assert got["kernel_features"] == _kernel(case), hex(got["kernel_features"])
    assert [r["rays"] for r in got["renders"]] == [r["rays"] for r in PARENT[case[0]]["renders"]]
    assert got == PARENT[case[0]]
