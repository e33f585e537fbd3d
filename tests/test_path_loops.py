"""The path kernel's loops other than the Cornell one, held per path under the tolerance contract: the
resumable room + mesh loop (scene 9 with fast arithmetic, scene 8 path-exact with leaf postponing) and
the plain loop (the bvh_node treelet kernels of scenes 0 and 7, Cornell smoke, the generic machine in
1024-thread groups, the mesh interpreter in one-wave groups).  A change that moves their code about --
the LDS layout, the claim protocol, the loops as functions of their own -- leaves every path's
operations, operands and stream positions what they were.

On the GPU, tools/path_loop_digest.py's cases against tests/golden/pathloops_parent.json, recorded with
that tool from the library of the commit before this test: scenes 0, 6, 7, 8 and 9 on 1, 65 and 2304
paths; scenes 9, 7 and 8 on 8460 paths (no multiple of 8 partitions x 256: dynamic claims and the tail
zone run); scene 5 through the generic machine and scene 9 through the mesh interpreter on 65 and 2304
paths; two renders in a row on one renderer (depth 32, then 2); and scene 5 without the debug flag, at
a size where the fast kernel hands at least four paths to the retrace kernel.  Per path radiance bits,
per path ray counts, the ray total, the kernel and its build must be the parent's exactly.
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


pld = _tool("path_loop_digest")

with open(os.path.join(ROOT, "tests", "golden", "pathloops_parent.json")) as _f:
    PARENT = json.load(_f)

FT_LIN = 1 << 11  # kernel feature bit: linear hit program (miniraytracer_amd/_lib.py)
BUILDS = ("exact", "fast", "fastz", "pex")  # miniraytracer_amd/_lib.py BUILDS
SIG_ROOM_MESH_SCENES = (8, 9)  # their kernels carry a program signature in kernel_features' third byte


def test_fixture_lists_every_case():
    assert sorted(PARENT) == sorted([c[0] for c in pld.CASES] + ["retrace"])
    for c in pld.CASES:
        e = PARENT[c[0]]
        assert [r["depth"] for r in e["renders"]] == list(c[5])
        for r in e["renders"]:
            assert r["rays"] >= c[2] * c[3] * c[4]  # at least the camera ray of every path
        kf, build = e["kernel_features"], BUILDS[e["build"]]
        sig = (kf >> 16) & 0xFF
        # the fixture itself ran the kernels it is about
        if c[6] == "MRT_FORCE_GENERIC":
            assert not kf & FT_LIN and sig == 0, (c[0], hex(kf))
        elif c[6] == "MRT_NO_SIG":
            assert kf & FT_LIN and sig == 0, (c[0], hex(kf))
        elif c[1] in SIG_ROOM_MESH_SCENES:
            assert sig != 0 and build == ("pex" if c[1] == 8 else "fastz"), (c[0], hex(kf), build)
        else:
            assert kf & FT_LIN and sig == 0, (c[0], hex(kf))
            assert build == {0: "fastz", 6: "pex", 7: "pex"}[c[1]], (c[0], build)


def test_fixture_covers_the_issue_cases():
    by = {c[0]: c for c in pld.CASES}
    for s in (0, 6, 7, 8, 9):
        assert {f"s{s}_1x1x1", f"s{s}_13x5x1", f"s{s}_24x24x4"} <= set(by)
    for s in (9, 7, 8):
        c = by[f"s{s}_ragged"]
        assert c[2] * c[3] * c[4] == 8460 and 8460 % (8 * 256) != 0
    assert {"generic_s5_13x5x1", "generic_s5_24x24x4", "nosig_s9_13x5x1", "nosig_s9_24x24x4"} <= set(by)
    assert by["s9_pair"][5] == (32, 2)
    # the pair's first render is the render a fresh renderer makes
    assert PARENT["s9_pair"]["renders"][0] == PARENT["s9_13x5x1"]["renders"][0]
    assert PARENT["s9_pair"]["renders"][1] != PARENT["s9_pair"]["renders"][0]
    rt = PARENT["retrace"]
    assert tuple(rt["size"]) in pld.RETRACE_SIZES and rt["handed_over"] >= pld.RETRACE_MIN
    assert BUILDS[rt["build"]] == "fastz"


@pytest.mark.gpu
@pytest.mark.parametrize("case", pld.CASES, ids=[c[0] for c in pld.CASES])
def test_same_bits_as_parent(mrt, case):
    got = pld.digest_case(mrt, case)
    print(case[0], got)
    want = PARENT[case[0]]
    assert (got["kernel_features"], got["build"]) == (want["kernel_features"], want["build"])
    assert [r["rays"] for r in got["renders"]] == [r["rays"] for r in want["renders"]]
    assert got == want


@pytest.mark.gpu
def test_retrace_same_bits_as_parent(mrt):
    want = PARENT["retrace"]
    got = pld.digest_retrace(mrt, tuple(want["size"]))
    print(got)
    assert got["handed_over"] == want["handed_over"]
    assert got["rays"] == want["rays"]
    assert got == want
