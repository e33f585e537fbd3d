"""The Cornell walk's light constants: the rect's extents and area computed once per wave and read from
its LDS (mrt_sig.h cornell_light_quad) instead of made from the scene words in every iteration, the light
pdf's cosine as |d.y * ns|, and a diffuse scatter's forward fold without the "no pdf" side where the
light's area is not negative.  A path's operations, their values and order and its stream positions stay
what they were.

Without a GPU: the quad as the host evaluates the kernel's function (mrt_debug_cornell_light_quad) on each
test light's words against xz_pdf_of_hit's expressions (f[1] - f[0]) * (f[3] - f[2]) in numpy float32,
each difference and the product a rounded float32 of its own.

On the GPU, tools/cornell_light_digest.py's cases against tests/golden/cornell_light_parent.json, recorded
with that tool from the library of the commit before this test: scene 5 at 64x64x16; depth limits 1 and 2;
1, 63, 64 and 65 paths; lights with unequal extents (40 x 210), moved towards a corner, one unit wide and
on bounds whose differences round; another rect as the biased object (the pdf's leaf path, which uses
nothing of the quad); two renderers with different lights rendered a, b, a on one device (the quad is a
launch's and a wave's, not cached); the glass-heavy scene; and one case through the interpreter's queue
kernel.  Per path radiance bits, per path ray counts and the ray total must be the parent's exactly.
"""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


cld = _tool("cornell_light_digest")
fpd = cld.fpd

with open(os.path.join(ROOT, "tests", "golden", "cornell_light_parent.json")) as _f:
    PARENT = json.load(_f)


def _kernels(case):
    return [cld.V_INTERP if case[6] else fpd.V_CORNELL] * len(case[1])


def test_fixture_lists_every_case():
    assert sorted(PARENT) == sorted(c[0] for c in cld.CASES)
    for c in cld.CASES:
        e = PARENT[c[0]]
        # the fixture itself ran the kernels it is about
        assert e["kernel_features"] == _kernels(c), (c[0], e["kernel_features"])
        assert [(r["renderer"], r["depth"]) for r in e["renders"]] == [tuple(x) for x in c[5]]
        for r in e["renders"]:
            assert r["rays"] >= cld.n_paths(c)  # at least the camera ray of every path


def test_fixture_covers_the_cases():
    by = {c[0]: c for c in cld.CASES}
    assert by["s5"][2:5] == (64, 64, 16) and by["s5"][5] == ((0, 32),)
    assert by["s5_d1"][2:6] == (16, 16, 4, ((0, 1),)) and by["s5_d2"][2:6] == (16, 16, 4, ((0, 2),))
    assert [cld.n_paths(by[f"paths_{n}"]) for n in (1, 63, 64, 65)] == [1, 63, 64, 65]
    assert {"light_uneven", "light_corner", "light_unit", "light_inexact", "offlight", "glass"} <= set(by)
    # a, b, a: two renderers, the first rendered again after the second -- with the parent's own bits
    assert by["alt"][1] == ("light_uneven", "light_inexact") and [k for k, _ in by["alt"][5]] == [0, 1, 0]
    a0, b, a1 = PARENT["alt"]["renders"]
    assert {k: v for k, v in a0.items()} == {k: v for k, v in a1.items()} and a0["radiance_sha256"] != b["radiance_sha256"]
    # ... and each is the render a renderer of its own makes
    strip = lambda r: {k: v for k, v in r.items() if k != "renderer"}  # noqa: E731
    assert strip(a0) == strip(PARENT["light_uneven"]["renders"][0]) and strip(b) == strip(PARENT["light_inexact"]["renders"][0])
    assert sum(1 for c in cld.CASES if c[6]) == 1
    # the lights differ from the stock one where the issue asks
    L = {n: cld.light_words(n) for n in cld.LIGHTS}
    ext = {n: (w[1] - w[0], w[3] - w[2]) for n, w in L.items()}
    assert ext["uneven"] == (40.0, 210.0) and ext["unit"][0] == 1.0
    assert ext["corner"] == ext["stock"] and not np.array_equal(L["corner"], L["stock"])
    w = L["inexact"].astype(np.float64)  # the float32 differences round
    assert np.float64(ext["inexact"][0]) != w[1] - w[0] and np.float64(ext["inexact"][1]) != w[3] - w[2]


def _quad(mrt, scene):
    fn = mrt.lib().mrt_debug_cornell_light_quad
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    quad, bounds = np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float32)
    assert fn(C.byref(scene.view), quad.ctypes.data, bounds.ctypes.data) == 0
    return quad, bounds


@pytest.mark.parametrize("name", sorted(cld.LIGHTS))
def test_quad_is_the_pdf_s_expressions(mrt, name):
    quad, bounds = _quad(mrt, cld.light_scene(mrt, name))
    f = cld.light_words(name)
    assert np.array_equal(bounds.view(np.uint32), f.view(np.uint32))  # the program's op 3 holds the test light's words
    ex, ez = np.float32(f[1] - f[0]), np.float32(f[3] - f[2])  # xz_pdf_of_hit / leaf_pdf_generate: each rounded
    area = np.float32(ex * ez)
    assert ex.dtype == np.float32 and area.dtype == np.float32
    want = np.asarray([ex, ez, area, 0.0], dtype=np.float32)
    assert np.array_equal(quad.view(np.uint32), want.view(np.uint32)), (quad, want)
    assert area > 0


def test_quad_of_the_offlight_scene_is_the_lights(mrt):
    # the biased object is another rect there; the quad stays op 3's (the walk's light), and the pdf's leaf path ignores it
    quad, bounds = _quad(mrt, fpd.offlight_scene(mrt))
    assert np.array_equal(bounds, cld.light_words("stock")) and quad[2] == np.float32(130.0 * 105.0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cld.CASES, ids=[c[0] for c in cld.CASES])
def test_same_bits_as_parent(mrt, case):
    got = cld.digest_case(mrt, case)
    print(case[0], got)
    assert got["kernel_features"] == _kernels(case), got["kernel_features"]
    assert [r["rays"] for r in got["renders"]] == [r["rays"] for r in PARENT[case[0]]["renders"]]
    assert got == PARENT[case[0]]
