"""The Cornell walk stores a finished path's radiance where the path ends (its loop holds no store for
the next iteration), which frees the registers that stood between seven and eight waves per SIMD; and
a refill of its queue of path starts skips the work of a start that the kernel never reads.  A path's
operations, operands, stream positions and the address of its three words stay what they were.

On the GPU, tools/cornell_store_digest.py's cases against tests/golden/cornell_store_parent.json,
recorded with that tool from the library of the commit before this test: 1, 63, 64, 65 and 129 paths
under depth limits 1 and 32 (the launch's last paths end inside a partial refill; at depth 1 every path
ends on its first or second ray) with MRT_RF_PATH_DEBUG, so the ray count's store sits beside the
radiance store; two renders in a row on one renderer; one-row images 1, 5, 63, 64 and 65 pixels wide at
16 spp (sixteen, twelve and one sample rows inside one refill of 64 starts, a row end before, at and
after a wave's 64th start); a pixel list of 5 pixels; a render in launches of 4 samples; a launch whose
path count is no multiple of 8 partitions x 256; a camera with a lens and a shutter (the time draw
reaches the ray: the stream still steps over it); and three of the cases through the interpreter's
queue kernel.  Per path radiance bits, per path ray counts and the ray total must be the parent's
exactly.
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


cst = _tool("cornell_store_digest")
fpd = cst.fpd

with open(os.path.join(ROOT, "tests", "golden", "cornell_store_parent.json")) as _f:
    PARENT = json.load(_f)


def _kernel(case):
    return cst.V_INTERP if case[7] else fpd.V_CORNELL


def test_fixture_lists_every_case():
    assert sorted(PARENT) == sorted(c[0] for c in cst.CASES)
    for c in cst.CASES:
        e = PARENT[c[0]]
        # the fixture itself ran the kernels it is about
        assert e["kernel_features"] == _kernel(c), (c[0], hex(e["kernel_features"]))
        assert [r["depth"] for r in e["renders"]] == list(c[5])
        n_pix = len(c[8]) if c[8] else c[2] * c[3]
        for r in e["renders"]:
            assert r["rays"] >= n_pix * c[4]  # at least the camera ray of every path
            assert ("image_sha256" in r) == bool(c[6])


def test_fixture_covers_the_issue_cases():
    names = set(PARENT)
    assert {f"store_{n}_d{d}" for n in (1, 63, 64, 65, 129) for d in (1, 32)} <= names
    assert {f"rows_w{w}" for w in (1, 5, 63, 64, 65)} <= names
    assert {"store_pair", "pixel_list", "chunked", "ragged", "lens_shutter"} <= names
    assert len([n for n in names if n.startswith("nosig_")]) == 3
    by = {c[0]: c for c in cst.CASES}
    assert by["chunked"][6] == 4 and len(by["pixel_list"][8]) == 5
    assert (by["ragged"][2] * by["ragged"][3] * by["ragged"][4]) % (8 * 256) != 0
    # the pair's second render is the render a fresh renderer makes
    assert PARENT["store_pair"]["renders"] == [PARENT["store_65_d32"]["renders"][0], PARENT["store_65_d1"]["renders"][0]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", cst.CASES, ids=[c[0] for c in cst.CASES])
def test_same_bits_as_parent(mrt, case):
    got = cst.digest_case(mrt, case)
    print(case[0], got)
    assert got["kernel_features"] == _kernel(case), hex(got["kernel_features"])
    assert [r["rays"] for r in got["renders"]] == [r["rays"] for r in PARENT[case[0]]["renders"]]
    assert got == PARENT[case[0]]


@pytest.mark.gpu
def test_sixty_four_registers_and_eight_waves_per_simd(mrt):
    """The fast Cornell variant allocates at most 64 VGPRs, its LDS is the queue and the hit table as
    tests/test_cornell_starts.py pins it, and the launch plan runs 32 one-wave groups per CU."""
    r = mrt.Renderer(mrt.select_scene(5, 1.0), 0)
    r.render(mrt.render_desc(8, 8, 1, numerics="fast"))
    ki = r.kernel_info()
    r.close()
    print(ki)
    assert ki["kernel_features"] == fpd.V_CORNELL and ki["wg"] == 64
    assert ki["vgprs"] <= 64
    assert ki["lds_bytes"] == 13 * 64 * 4 + 14 * 12 * 4
    assert ki["n_cu"] > 0 and ki["grid"] == 32 * ki["n_cu"]
