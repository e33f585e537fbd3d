"""The Cornell walk's hit table (mrt_sig.h cornell_fast_hit, mrt_tables.hip cornell_hit_fill): the
walk carries the closest hit's identity and reads the record's constants -- normal, plane, code,
material -- from a table of the uploaded scene.

1. Without a GPU: the table as built on the host (mrt_debug_cornell_hits), entry by entry against the
   view it was built from -- scene 5, tools/fast_path_digest.py's glass and offlight scenes, and
   tools/cornell_table_digest.py's walls scene (a material of its own on every wall and on the box,
   the box's rotation negated): every room face has its own wall's plane and material, a box face the
   min / max plane by its normal's sign and the normal rotated back, each material's words are the
   material table's.
2. On the GPU: the walls scene's per-path radiance and ray digests equal
   tests/golden/cornell_table_parent.json, recorded with tools/cornell_table_digest.py from the build
   of the commit before the table (scene 5's own cases, tests/test_parked_scatter.py, cannot see a
   wrong index: its floor, ceiling and back wall share one material, its box has one).
"""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import synth_scenes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


ctd = _tool("cornell_table_digest")
fpd = ctd.fpd

with open(os.path.join(ROOT, "tests", "golden", "cornell_table_parent.json")) as _f:
    PARENT = json.load(_f)

HIT_ROOM, HIT_LIGHT, HIT_BOX, HIT_SPHERE, HIT_COUNT, HIT_WORDS = 0, 6, 7, 13, 14, 16
WALLS, LIGHT, SPHERE = (1, 2, 4, 5, 6), 3, 16  # scene 5's view (tests/test_synthetic_scenes.py)
AXIS = {ss.K_YZ: 0, ss.K_XZ: 1, ss.K_XY: 2}


def hit_table(mrt, s):
    fn = mrt.lib().mrt_debug_cornell_hits
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    fn.restype = C.c_int
    words = np.zeros(HIT_COUNT * HIT_WORDS, dtype=np.uint32)
    n = np.zeros(1, dtype=np.uint32)
    assert fn(C.byref(s.view), words.ctypes.data, len(words), n.ctypes.data) == 0
    return words[:int(n[0])].reshape(-1, HIT_WORDS)


def bits(*x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def mat_words(s, mat):
    """The material table's record of `mat` (mrt_tables.hip material_table) as the entry's words 5-11."""
    m = s.materials[mat]
    flags, col = 0, np.zeros(4, dtype=np.float32)
    if m["tex"] < len(s.textures) and s.textures[m["tex"]]["kind"] == ss.T_COLOR:
        flags, col = 1, s.textures[m["tex"]]["f"].copy()
    if m["kind"] == ss.M_DIELECTRIC:
        one, ref = np.float32(1.0), np.float32(m["p"])
        r0 = (one - ref) / (one + ref)
        col[0], col[1] = one / ref, r0 * r0
    return np.concatenate([np.asarray([m["kind"]], dtype=np.uint32), bits(m["p"]), np.asarray([flags], dtype=np.uint32), col.view(np.uint32)])


def one_hot(a, sign):
    n = np.zeros(3, dtype=np.float32)
    n[a] = sign
    return n


def check_entry(tab, ident, n, k, code, words, what):
    e = tab[ident]
    if n is not None:
        assert np.array_equal(e[0:3], np.asarray(n, dtype=np.float32).view(np.uint32)), (what, "normal", e[0:3].view(np.float32), n)
    if k is not None:
        assert e[3] == bits(k)[0], (what, "plane", e[3:4].view(np.float32), k)
    assert e[4] == code, (what, "code", e[4], code)
    assert np.array_equal(e[5:12], words), (what, "material", e[5:12], words)
    assert not e[12:].any(), what


SCENES = {
    "s5": lambda mrt: ss.Synth(mrt.select_scene(5, 1.0)),
    "glass": lambda mrt: fpd.glass_scene(mrt),
    "offlight": lambda mrt: fpd.offlight_scene(mrt),
    "walls": lambda mrt: ctd.walls_scene(mrt),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_table_entries_match_the_view(mrt, name):
    s = SCENES[name](mrt)
    tab = hit_table(mrt, s)
    assert tab.shape == (HIT_COUNT, HIT_WORDS)
    # the room: each wall at face 2 * axis + side (side 1: the normal points down the axis, the max plane)
    seen = set()
    for w in WALLS:
        nd = s.nodes[w]
        a, sign = AXIS[int(nd["kind"]) & 0xFF], float(nd["f"][5])
        face = 2 * a + (0 if sign > 0 else 1)
        seen.add(face)
        check_entry(tab, HIT_ROOM + face, one_hot(a, sign), nd["f"][4], 1 + a, mat_words(s, int(nd["mat"])), ("wall", w))
    assert len(seen) == 5
    (missing,) = set(range(6)) - seen
    assert tab[HIT_ROOM + missing][4] == 1 + missing // 2
    # the light (op 3)
    nd = s.nodes[LIGHT]
    check_entry(tab, HIT_LIGHT, one_hot(1, nd["f"][5]), nd["f"][4], 2, mat_words(s, int(nd["mat"])), "light")
    # the box: box.h's six rects under rotate_y; a face's identity by its axis and its outward normal's sign
    (rot,) = s.find(ss.K_ROTY)
    sn, cs = np.float32(s.nodes[rot]["f"][6]), np.float32(s.nodes[rot]["f"][7])
    faces = s.list_items(int(s.nodes[rot]["a"]))
    ids = set()
    for f in faces:
        nd = s.nodes[f]
        a, sign = AXIS[int(nd["kind"]) & 0xFF], np.float32(nd["f"][5])
        lx, ly, lz = one_hot(a, sign)
        n = [cs * lx + sn * lz, ly, cs * lz - sn * lx]  # unrotate_rec's normal (scene_object.cpp:85-93)
        ident = HIT_BOX + 2 * a + (1 if sign < 0 else 0)
        ids.add(ident)
        check_entry(tab, ident, n, nd["f"][4], 4 + a, mat_words(s, int(nd["mat"])), ("box face", f))
    assert ids == set(range(HIT_BOX, HIT_SPHERE))
    # the sphere: its material only (the normal is the ray's own)
    check_entry(tab, HIT_SPHERE, None, None, 7, mat_words(s, int(s.nodes[SPHERE]["mat"])), "sphere")


def test_walls_scene_tells_entries_apart(mrt):
    """What the walls scene is for: no two identities with a material share one, the sine is negative,
    and the rotated normals of opposite box faces differ in sign."""
    s = ctd.walls_scene(mrt)
    tab = hit_table(mrt, s)
    walls = [2 * AXIS[int(s.nodes[w]["kind"]) & 0xFF] + (0 if s.nodes[w]["f"][5] > 0 else 1) for w in WALLS]
    colours = {tuple(tab[HIT_ROOM + i][8:11]) for i in walls} | {tuple(tab[HIT_BOX][8:11])}
    assert len(colours) == 6
    (rot,) = s.find(ss.K_ROTY)
    assert s.nodes[rot]["f"][6] < 0
    for a in range(3):
        up, down = tab[HIT_BOX + 2 * a][0:3].view(np.float32), tab[HIT_BOX + 2 * a + 1][0:3].view(np.float32)
        assert np.array_equal(up, -down) and np.abs(up).max() > 0.9


def test_no_table_without_the_shape(mrt):
    sc = mrt.select_scene(9, 1.0)  # room + mesh: another walk
    assert hit_table(mrt, sc).size == 0
    sc.close()


def test_fixture_lists_every_case():
    assert sorted(PARENT) == sorted(c[0] for c in ctd.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ctd.CASES, ids=[c[0] for c in ctd.CASES])
def test_walls_same_bits_as_parent(mrt, case):
    got = ctd.digest_case(mrt, case)
    print(case[0], got)
    assert got["kernel_features"] == fpd.V_CORNELL, hex(got["kernel_features"])
    assert got == PARENT[case[0]]


@pytest.mark.gpu
def test_table_in_the_cornell_walks_lds(mrt):
    """The Cornell walk's launch (tolerance contract) has the wave's copy of the table in its LDS --
    12 words of each of the 14 entries beside the wave's queue of path starts -- and still fits seven
    waves per SIMD: at most 72 VGPRs, 28 slices in a CU's 160 KiB."""
    r = mrt.Renderer(mrt.select_scene(5, 1.0), 0)
    r.render(mrt.render_desc(8, 8, 1, numerics="fast"))
    ki = r.kernel_info()
    r.close()
    print(ki)
    queue = 13 * 64 * 4  # mrt_kernels.hip PathQ
    assert ki["kernel_features"] == fpd.V_CORNELL and ki["wg"] == 64
    assert ki["lds_bytes"] == queue + HIT_COUNT * 12 * 4
    assert ki["vgprs"] <= 72 and 28 * ki["lds_bytes"] <= 160 * 1024
