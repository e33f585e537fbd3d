"""The Cornell walk's cosine scatter takes the basis axis of a table normal from a table of the hit's
identity (mrt_sig.h kHitAxisWords, mrt_shade.h onb_axis_v), computed once per wave with the per-lane
basis' own function; a path's operations, operands and stream order stay what they were.

On the GPU, tools/cornell_start_digest.py's cases against tests/golden/cornell_starts_parent.json,
recorded with that tool from the library of the commit before the axes table: the sphere made
lambertian (the one identity whose normal is the ray's own keeps the per-lane basis beside the walls'
table axes), a camera with a lens and a shutter (disk point, (u, v) and time draw reach the ray), 1,
63, 64, 65 and 129 paths (launches that end inside a refill of the queue of path starts), one render
in several launches, and the last three through the interpreter's queue kernel (MRT_NO_SIG=1).  Per
path radiance bits, per path ray counts and the ray total must be the parent's exactly.
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


csd = _tool("cornell_start_digest")
fpd = csd.fpd

with open(os.path.join(ROOT, "tests", "golden", "cornell_starts_parent.json")) as _f:
    PARENT = json.load(_f)


def test_fixture_lists_every_case():
    assert sorted(PARENT) == sorted(c[0] for c in csd.CASES)
    for c in csd.CASES:
        e = PARENT[c[0]]
        # the fixture itself ran the kernels it is about
        assert e["kernel_features"] == (csd.V_INTERP if c[6] else fpd.V_CORNELL), (c[0], hex(e["kernel_features"]))
        assert e["rays"] >= c[2] * c[3] * c[4]  # at least the camera ray of every path
        assert ("image_sha256" in e) == bool(c[5])


@pytest.mark.gpu
@pytest.mark.parametrize("case", csd.CASES, ids=[c[0] for c in csd.CASES])
def test_same_bits_as_parent(mrt, case):
    got = csd.digest_case(mrt, case)
    print(case[0], got)
    assert got["kernel_features"] == (csd.V_INTERP if case[6] else fpd.V_CORNELL), hex(got["kernel_features"])
    assert got["rays"] == PARENT[case[0]]["rays"]
    assert got == PARENT[case[0]]


@pytest.mark.gpu
def test_axes_take_no_lds_and_keep_the_occupancy(mrt):
    """The axes live in the spare words of the queue's claim row: the launch's LDS is the queue and
    the hit table as before, at most 72 VGPRs, 28 waves per CU."""
    r = mrt.Renderer(mrt.select_scene(5, 1.0), 0)
    r.render(mrt.render_desc(8, 8, 1, numerics="fast"))
    ki = r.kernel_info()
    r.close()
    print(ki)
    assert ki["kernel_features"] == fpd.V_CORNELL and ki["wg"] == 64
    assert ki["lds_bytes"] == 13 * 64 * 4 + 14 * 12 * 4
    assert ki["vgprs"] <= 72 and 28 * ki["lds_bytes"] <= 160 * 1024
