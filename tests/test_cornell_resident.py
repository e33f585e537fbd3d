"""What the Cornell kernel reads of the scene on every iteration -- the room, the box, the sphere, the
light's rect, the depth limit -- is constant for a launch; work that turns those words into state of
the launch (or moves where they are read) must leave every path's operations, operands and stream
order as they are, for every launch and not only the first of a renderer.

On the GPU, tools/cornell_resident_digest.py's cases against tests/golden/cornell_resident_parent.json,
recorded with that tool from the library of the commit before this test: scene 5 at 24x24x4 under
depth limits 1, 2, 5 and 32; two renders in a row on ONE renderer, depth 32 then 2 and 2 then 32 (a
value kept from the launch before); launches of 63, 65 and 129 paths (one partial refill of the queue
of path starts, two refills, a launch across a claim boundary); one render in several launches (a
launch whose first sample is not 0); a material per wall with the box's rotation negated; the sphere
lambertian; the glass-heavy scene; another rect than the light as the biased object (light_once off:
the biased-leaf path); mode 1; and the catalogue's two Cornell lookalikes.  Every room of the Cornell
shape has five faces (the sixth bit of its mask is clear, in scene 5 as in b_cornell_lookalike), so the
mask is tested by every case; the catalogue's room that lacks one of THOSE,
b_cornell_lookalike_open_room, does not have the shape (the upload finds no room) and runs the
interpreter's kernel: it is here so that it keeps doing so with the same bits.  Per path radiance bits,
per path ray counts and the ray total must be the parent's exactly.
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


crd = _tool("cornell_resident_digest")

with open(os.path.join(ROOT, "tests", "golden", "cornell_resident_parent.json")) as _f:
    PARENT = json.load(_f)


def test_fixture_lists_every_case():
    assert sorted(PARENT) == sorted(c[0] for c in crd.CASES)
    for c in crd.CASES:
        e = PARENT[c[0]]
        # the fixture itself ran the kernels it is about
        assert e["kernel_features"] == c[7], (c[0], hex(e["kernel_features"]))
        assert [(r["depth"], r["mode"]) for r in e["renders"]] == list(c[5])
        for r in e["renders"]:
            assert r["rays"] >= c[2] * c[3] * c[4]  # at least the camera ray of every path
            assert ("image_sha256" in r) == bool(c[6])


def test_fixture_pairs_are_the_single_renders():
    """The parent's second render on a renderer is the render a fresh renderer makes: the pair cases
    compare with a record that itself holds no stale state."""
    one = {d: PARENT[f"s5_depth_{d}"]["renders"][0] for d in (2, 32)}
    assert PARENT["pair_32_2"]["renders"] == [one[32], one[2]]
    assert PARENT["pair_2_32"]["renders"] == [one[2], one[32]]
    # mode 1 changes the fold of the samples, not the paths
    assert PARENT["s5_mode1"]["renders"][0]["rays"] == one[32]["rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", crd.CASES, ids=[c[0] for c in crd.CASES])
def test_same_bits_as_parent(mrt, case):
    got = crd.digest_case(mrt, case)
    print(case[0], got)
    assert got["kernel_features"] == case[7], hex(got["kernel_features"])
    assert [r["rays"] for r in got["renders"]] == [r["rays"] for r in PARENT[case[0]]["renders"]]
    assert got == PARENT[case[0]]
