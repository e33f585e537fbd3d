"""The render path on scene graphs the ten reference scenes never build.

Every GPU parity test elsewhere renders select_scene(0..9), the graphs the kernels were specialised
for; mrt_scene_upload takes any mrt_scene_view.  The catalogue below builds views by hand
(tests/synth_scenes.py) and checks, per entry:

host leg (no GPU)  the CPU backend equals the C restatement bit for bit (image, ray total); the
                   entry's addition is live (the restatement's image or ray total differs from the
                   same graph without it); `features` is the entry's literal; the structure of the
                   tolerance contract's rewritten program.
GPU leg            the kernel picked is the entry's literal; the exact contract equals the
                   restatement per path (radiance bits, ray counts), also under the test hooks that
                   force the other walks; the tolerance contract holds the bars
                   test_fast_numerics_close_to_exact_other_scenes uses, and where it runs the path-exact
                   build it equals the restatement's forward fold (oracle.desc(fold=1)) per path, again
                   under the hooks whose walk runs that build.

The feature / kernel literals are worked out by hand from scene_features (mrt_tables.hip) and
pick_variant (mrt_upload.hip, mrt_launch.h kVariants): index 0-2 the shape-specialised walks, 3-7 the narrower
interpreters, 8 the catch-all interpreter 0x3FFF, 9 the generic machine 0x37FF.
"""
import ctypes as C

import numpy as np
import pytest

import synth_scenes as ss
from synth_scenes import (FT_BIASED, FT_BSPHERE, FT_BVH, FT_BVHW, FT_INST, FT_ISO, FT_LIN, FT_MESH, FT_METAL, FT_MOVING, FT_SKY,
                          FT_TEX, FT_UV, FT_VOLUME, FT_VSUB, Synth)

SIG_CORNELL, SIG_ROOM_MESH = 1 << 16, 2 << 16
V_CORNELL = FT_LIN | FT_INST | FT_BIASED | SIG_CORNELL      # 0
V_ROOM_MESH = FT_LIN | FT_MESH | FT_BIASED | SIG_ROOM_MESH  # 1
V_ROOM_MESH_METAL = V_ROOM_MESH | FT_METAL                  # 2
V_LIN_INST = FT_LIN | FT_INST | FT_BIASED                   # 3
V_LIN_MESH = FT_LIN | FT_MESH | FT_METAL | FT_BIASED        # 4
V_SKY = 0x1DB0                                              # 5: LIN BVHW TEX METAL MOVING SKY UV
V_SMOKE = 0x684C                                            # 6: LIN INST VOLUME VSUB ISO BIASED
V_BOOK2 = 0x3CFC                                            # 7: LIN BVHW VOLUME INST TEX METAL ISO MOVING UV BIASED
V_ANY_LIN, V_GENERIC = 0x3FFF, 0x37FF                       # 8, 9

_ref = {}


def ref_scene(mrt, sid):
    if sid not in _ref:
        _ref[sid] = mrt.select_scene(sid, 1.0)
    return _ref[sid]


# scene 5 (dump of its view): root list 0 = [yz 1, yz 2, light 3, xz 4, xz 5, xy 6, translate 7, glass sphere 16],
# biased list 17 = [3]; materials 0 red, 1 white, 2 green, 3 light, 4 glass
C_ROOT, C_LIGHT, C_INST, C_SPHERE, C_BIASED = 0, 3, 7, 16, 17
C_WHITE, C_LIGHTMAT, C_GLASS = 1, 3, 4
# scene 9: root list 0 = [walls and light 1..6, mesh 7], biased list 8 = [3]
R_MESH, R_BIASED = 7, 8


def cornell(mrt):
    return Synth(ref_scene(mrt, 5))


def add_to_root(s, items):
    s.set_list(s.root, s.list_items(s.root) + list(items))
    return s


# ---------------------------------------------------------------- builders: (graph, the graph without its addition)
def b_cornell_plus_sphere(mrt):
    base = cornell(mrt)
    s = base.copy()
    add_to_root(s, [s.sphere((420, 70, 140), 70, s.lambertian(0.2, 0.3, 0.7))])
    return s, base


def lookalike(mrt, closed=True, with_box=True, scale=1.0, planes=0.0, glass=False):
    """SIG_CORNELL's op / kind / skip sequence on other numbers: a room of 100 units, a box of another
    shape under a negative angle, a lambertian sphere elsewhere, the light moved and resized.
    scale: every coordinate and the camera times it (a power of two); planes: the plane of the floor and
    of the left wall (0: ordinary; off zero and below 2^-77 they are MRT_F_SLOWDIV rects); glass: a
    dielectric sphere in place of the lambertian one."""
    s = Synth(ref_scene(mrt, 5)).clear()
    s.scale_camera(100.0 / 555.0 * scale)
    red, white, green = s.lambertian(0.6, 0.1, 0.1), s.lambertian(0.7, 0.7, 0.6), s.lambertian(0.1, 0.5, 0.2)
    light = s.material(ss.M_LIGHT, s.color(11, 12, 13), 1.0)

    def c(*v):
        return [x * scale for x in v]

    L = 100.0 * scale
    lamp = s.rect(ss.K_XZ, *c(30, 62, 41, 73, 99.5), light, -1.0)
    walls = [s.rect(ss.K_YZ, 0, L, 0, L, L, green, -1.0), s.rect(ss.K_YZ, 0, L, 0, L, planes, red, 1.0), lamp,
             s.rect(ss.K_XZ, 0, L, 0, L, L, white, -1.0), s.rect(ss.K_XZ, 0, L, 0, L, planes, white, 1.0),
             s.rect(ss.K_XY, 0, L, 0, L, L if closed else 90.0 * scale, white, -1.0)]
    box = s.translate(s.rotate_y(s.box((0, 0, 0), c(28, 55, 31), white), -18.0, box=c(-40, 0, -40, 60, 56, 60)), c(52, 0, 47))
    ball = s.sphere(c(27, 15, 30), 15 * scale, s.material(ss.M_DIELECTRIC, ss.NONE, 1.5) if glass else s.lambertian(0.3, 0.3, 0.8))
    s.root = s.list(walls + ([box] if with_box else []) + [ball], box=c(-1, -1, -1, 101, 101, 101))
    s.biased = s.list([lamp], box=c(30, 99, 41, 62, 100, 73))
    return s


def b_lookalike(mrt):
    return lookalike(mrt), lookalike(mrt, with_box=False)


def b_lookalike_open(mrt):
    return lookalike(mrt, closed=False), lookalike(mrt, closed=False, with_box=False)


def collapse_mesh(s, rng, max_tris=100):
    """Reshape a pod_bvh: subtrees of at most max_tris contiguous triangles become leaves, every
    remaining inner node gets a fresh order byte."""
    mn = s.mesh_nodes.copy()

    def rec(i):
        cnt = int(mn[i]["count_order"]) & 0xFFFFFF
        if cnt:
            return int(mn[i]["left_or_first"]), cnt
        l = int(mn[i]["left_or_first"])
        a, b = rec(l), rec(l + 1)
        if a and b and (a[0] + a[1] == b[0] or b[0] + b[1] == a[0]) and a[1] + b[1] <= max_tris:
            mn[i]["left_or_first"], mn[i]["count_order"] = min(a[0], b[0]), a[1] + b[1]
            return min(a[0], b[0]), a[1] + b[1]
        mn[i]["count_order"] = int(rng.integers(0, 256)) << 24
        return None

    for m in s.find(ss.K_MESH):
        rec(int(s.nodes[m]["a"]))
    leaves = mn["count_order"] & 0xFFFFFF
    assert leaves.max() > 25  # (the project's own builder stops at 25)
    s.set_mesh(mn)
    return s


def b_mesh_reshaped(mrt):
    base = Synth(ref_scene(mrt, 9))
    return collapse_mesh(base.copy(), np.random.default_rng(901)), base


def b_mesh_degenerate(mrt):
    base, _ = b_mesh_reshaped(mrt)
    s = base.copy()
    # the two largest triangles lose their area (u = 0): tri_hit's determinant is 0 there
    area = np.linalg.norm(np.cross(s.tri_geo[:, 4:7], s.tri_geo[:, 8:11]), axis=1)
    s.tri_geo[np.argsort(area)[-2:], 4:8] = 0.0
    s._view = None
    return s, base


def degenerate_normals(mrt):
    """The room + mesh lookalike whose vertex normals sum to 0, to ~1e-30 and to ~1e25 on a quarter of
    the triangles each: mesh_leaf's normalize takes its IEEE fallback (|n|^2 out of [2^-52, 2^52))."""
    s = room_mesh_lookalike(mrt, False)
    n = s.tri_nrm.copy()
    k = np.arange(len(n))
    n[k % 4 == 0] = 0.0
    n[k % 4 == 1] *= np.float32(1e-30)
    n[k % 4 == 2] *= np.float32(1e25)
    s.set_mesh(s.mesh_nodes, s.tri_geo, n)
    return s


def scaled_spheres(s, k):
    """A graph of spheres, lists and bvh_nodes (and its camera) scaled by k about the origin."""
    s = s.copy()
    k = np.float32(k)
    kind = s.nodes["kind"] & 0xFF
    f = s.nodes["f"]
    assert set(int(x) for x in kind) <= {ss.K_SPHERE, ss.K_LIST, ss.K_BVH}
    sp = kind == ss.K_SPHERE
    f[sp, 0:6] *= k
    f[sp, 8] *= k
    f[~sp, 0:6] *= k
    s.scale_camera(k)
    s._view = None
    return s


def b_tree_scaled(mrt):
    s, _ = b_tree_list_leaves(mrt)
    return scaled_spheres(s, 2.0 ** 50), s


def room_mesh_lookalike(mrt, metal):
    s, _ = b_mesh_reshaped(mrt)
    # the room resized to [-20, 600]^3 (the mesh and the light stay)
    lo, hi = -20.0, 600.0
    for w in (1, 2, 4, 5, 6):
        f = s.nodes[w]["f"]
        f[0], f[1], f[2], f[3] = lo, hi, lo, hi
        f[4] = hi if f[5] < 0 else lo
    s.nodes[s.root]["f"][:6] = (lo - 1, lo - 1, lo - 1, hi + 1, hi + 1, hi + 1)
    if metal:
        s.nodes[R_MESH]["mat"] = s.material(ss.M_METAL, s.color(0.8, 0.8, 0.9), 0.9)
    s._view = None
    return s


def b_room_mesh(mrt):
    s = room_mesh_lookalike(mrt, False)
    w = s.copy()
    w.set_list(w.root, [i for i in w.list_items(w.root) if i != R_MESH])
    return s, w


def b_room_mesh_metal(mrt):
    s = room_mesh_lookalike(mrt, True)
    return s, room_mesh_lookalike(mrt, False)


def b_room_mesh_plus_sphere(mrt):
    base = Synth(ref_scene(mrt, 9))
    s = base.copy()
    add_to_root(s, [s.sphere((430, 60, 120), 60, s.lambertian(0.2, 0.6, 0.6))])
    return s, base


def biased_with(mrt, extra_in_list=True, sky=0, second_light=False):
    base = cornell(mrt)
    s = base.copy()
    items = [C_LIGHT, C_SPHERE]
    if second_light:
        up = s.rect(ss.K_XZ, 60, 200, 330, 480, 12.0, C_LIGHTMAT, 1.0)
        add_to_root(s, [up])
        items.append(up)
    s.biased = s.list(items, box=(0, 0, 0, 555, 555, 555))
    s.sky = sky
    return s, base


def b_biased_sphere(mrt):
    return biased_with(mrt)


def b_biased_three_sky(mrt):
    return biased_with(mrt, sky=1, second_light=True)


def b_biased_bare_sphere(mrt):
    base = cornell(mrt)
    s = base.copy()
    s.biased = C_SPHERE
    return s, base


def b_biased_bare_xz(mrt):
    base = cornell(mrt)
    s = base.copy()
    s.biased = C_LIGHT
    return s, base


def b_biased_enclosing_sphere(mrt):
    base, _ = biased_with(mrt)
    s = base.copy()
    # the glass sphere around the tall box (165 x 330 x 165 at (265, 0, 295)): every light sample from
    # the box's faces starts inside it, where sphere::pdf_value takes sqrt(1 - r^2 / d^2) of d < r
    s.nodes[C_SPHERE]["f"][:3] = s.nodes[C_SPHERE]["f"][3:6] = (347, 165, 377)
    s.nodes[C_SPHERE]["f"][8] = 260
    s._view = None
    return s, base


def b_biased_emissive_sphere(mrt):
    base, _ = biased_with(mrt)
    s = base.copy()
    s.nodes[C_SPHERE]["mat"] = C_LIGHTMAT
    s._view = None
    return s, base


def b_nopdf_xy_in_list(mrt):
    base = cornell(mrt)
    base = add_to_root(base, [base.rect(ss.K_XY, 200, 350, 200, 350, 554.0, C_LIGHTMAT, -1.0)])
    s = base.copy()
    s.biased = s.list([s.list_items(s.root)[-1], C_LIGHT], box=(0, 0, 0, 555, 555, 555))
    return s, base


def b_nopdf_bare_xy(mrt):
    s, base = b_nopdf_xy_in_list(mrt)
    s.biased = s.list_items(s.root)[-1]
    s._view = None
    return s, base


def b_nopdf_mesh_in_list(mrt):
    base = Synth(ref_scene(mrt, 9))
    s = base.copy()
    s.biased = s.list([C_LIGHT, R_MESH], box=(0, 0, 0, 555, 555, 555))
    return s, base


def b_moving_sphere(mrt):
    base = cornell(mrt)
    s = base.copy()
    add_to_root(s, [s.sphere((420, 90, 140), 60, s.lambertian(0.7, 0.3, 0.1), center1=(420, 150, 140), t0=0.0, t1=1.0)])
    return s, base


def b_textures(mrt):
    base = cornell(mrt)
    s = base.copy()
    rng = np.random.default_rng(77)
    s.texels = rng.integers(0, 256, size=3 + 7 * 5 * 3, dtype=np.uint8)  # a 7 x 5 image at byte offset 3
    img = s.texture(ss.T_IMAGE, a=3, b=7, c=5)
    chk = s.texture(ss.T_CHECKER, a=s.color(0.2, 0.3, 0.1), b=img, f=(0.05,))
    per = s.texture(ss.T_PERLIN, f=(0.03,))
    s.nodes[4]["mat"] = s.material(ss.M_LAMBERTIAN, chk)   # ceiling: checker over an image
    s.nodes[5]["mat"] = s.material(ss.M_LAMBERTIAN, per)   # floor: Perlin
    s.nodes[6]["mat"] = s.material(ss.M_METAL, img, 0.8)   # back wall: metal with an image
    s.nodes[1]["mat"] = s.material(ss.M_METAL, s.color(0.7, 0.9, 0.7), 1.0)
    add_to_root(s, [s.sphere((420, 70, 140), 70, s.material(ss.M_LAMBERTIAN, img)),
                    s.sphere((120, 330, 400), 50, s.material(ss.M_LAMBERTIAN, per))])
    return s, base


def teapot_instance(mrt, rotate, sky):
    base = Synth(ref_scene(mrt, 9))
    s = base.copy()
    big = (-2000, -2000, -2000, 2000, 2000, 2000)
    inst = s.translate(s.rotate_y(R_MESH, 25.0, box=big), (150, 10, -90)) if rotate else s.translate(R_MESH, (-30, 40, 25))
    s.set_list(s.root, [inst if i == R_MESH else i for i in s.list_items(s.root)])
    s.sky = sky
    return s, base


def sphere_cloud(s, rng, n, lo, hi, r, mats):
    c = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    c = c[np.argsort(c[:, 0])]
    ids = [s.sphere(tuple(p), r, mats[i % len(mats)]) for i, p in enumerate(c)]
    return ids, [tuple(p - r) + tuple(p + r) for p in c]


def sky_mats(s):
    return [s.lambertian(0.6, 0.3, 0.2), s.lambertian(0.2, 0.5, 0.7), s.material(ss.M_METAL, s.color(0.8, 0.7, 0.6), 0.9),
            s.material(ss.M_DIELECTRIC, ss.NONE, 1.5)]


def sky_base(mrt):
    s = Synth(ref_scene(mrt, 0)).clear()
    s.sky = 1
    return s


def b_big_tree(mrt, n=3000):
    rng = np.random.default_rng(3000)
    s = sky_base(mrt)
    mats = sky_mats(s)
    ground = s.sphere((0, -1000, 0), 1000, mats[0])
    ids, boxes = sphere_cloud(s, rng, n, (-11, 0.2, -11), (11, 0.2, 11), 0.2, mats)
    s.root = s.bvh([ground] + ids, [(-1000, -2000, -1000, 1000, 0, 1000)] + boxes, orders=rng)
    w = sky_base(mrt)
    w.root = w.sphere((0, -1000, 0), 1000, sky_mats(w)[0])
    return s, w


def b_tree_list_leaves(mrt):
    rng = np.random.default_rng(55)
    s = sky_base(mrt)
    mats = sky_mats(s)
    ground = s.sphere((0, -1000, 0), 1000, mats[0])
    leaves, boxes = [ground], [(-1000, -2000, -1000, 1000, 0, 1000)]
    for k in range(60):
        x0 = -9 + 0.3 * k
        ids, bx = sphere_cloud(s, rng, 5, (x0, 0.25, -6), (x0 + 0.3, 0.25, 6), 0.25, mats)
        bx = np.asarray(bx)
        box = tuple(bx[:, :3].min(axis=0)) + tuple(bx[:, 3:].max(axis=0))
        leaves.append(s.list(ids, box=box))
        boxes.append(box)
    s.root = s.bvh(leaves, boxes, orders=rng)
    w = sky_base(mrt)
    w.root = w.sphere((0, -1000, 0), 1000, sky_mats(w)[0])
    return s, w


def chain(mrt, n):
    rng = np.random.default_rng(n)
    s = sky_base(mrt)
    mats = sky_mats(s)
    ground = s.sphere((0, -1000, 0), 1000, mats[0])
    ids, boxes = sphere_cloud(s, rng, n, (-8, 0.4, -5), (8, 0.4, 5), 0.4, mats)
    s.root = s.bvh(ids + [ground], boxes + [(-1000, -2000, -1000, 1000, 0, 1000)], split=lambda k: 1, orders=rng)
    w = sky_base(mrt)
    w.root = w.sphere((0, -1000, 0), 1000, sky_mats(w)[0])
    return s, w


def b_bvh_in_room(mrt, n):
    base = cornell(mrt)
    s = base.copy()
    rng = np.random.default_rng(700 + n)
    mats = [s.lambertian(0.6, 0.3, 0.2), s.lambertian(0.2, 0.5, 0.7)]
    if n <= 2:
        ids = [s.sphere((420, 60, 140), 60, mats[0]), s.sphere((120, 300, 380), 45, mats[1])][:n]
        boxes = [(360, 0, 80, 480, 120, 200), (75, 255, 335, 165, 345, 425)][:n]
    else:
        ids, boxes = sphere_cloud(s, rng, n, (30, 6, 30), (525, 6, 525), 6, mats)
    add_to_root(s, [s.bvh(ids, boxes, orders=rng)])
    return s, base


def b_volume_live(mrt):
    base, _ = biased_with(mrt)
    s = base.copy()
    # book2's pairing (scene.cpp:431-435): the fog shares the glass sphere's boundary, so a ray that
    # refracted into the glass is `inside` and the boundary sphere reports its far root
    add_to_root(s, [s.volume(C_SPHERE, 0.02, (0.2, 0.4, 0.9))])
    return s, base


def smoke_plus(mrt, metal):
    base = Synth(ref_scene(mrt, 6))
    s = base.copy()
    mat = s.material(ss.M_METAL, s.color(0.8, 0.8, 0.9), 0.9) if metal else s.lambertian(0.2, 0.3, 0.7)
    add_to_root(s, [s.sphere((420, 60, 110), 60, mat)])
    return s, base


def b_nested_translate(mrt):
    base = cornell(mrt)
    s = base.copy()
    add_to_root(s, [s.translate(s.translate(s.sphere((0, 0, 0), 70, s.lambertian(0.2, 0.3, 0.7)), (400, 30, 100)), (20, 40, 40))])
    return s, base


def b_bvh_instance_leaf(mrt):
    base = cornell(mrt)
    s = base.copy()
    m = s.lambertian(0.2, 0.3, 0.7)
    a = s.sphere((420, 60, 140), 60, m)
    b = s.translate(s.sphere((0, 0, 0), 45, m), (120, 300, 380))
    add_to_root(s, [s.bvh([a, b], [(360, 0, 80, 480, 120, 200), (75, 255, 335, 165, 345, 425)])])
    return s, base


def rooms(mrt, walls, nested=False, two=False):
    """Rooms of `walls` inward-facing rects (of floor, ceiling, back, left, right, front) around a
    lambertian sphere, lit by a ceiling light in the biased list."""
    s = Synth(ref_scene(mrt, 5)).clear()
    white, red = s.lambertian(0.7, 0.7, 0.7), s.lambertian(0.6, 0.1, 0.1)
    light = s.material(ss.M_LIGHT, s.color(15, 15, 15), 1.0)

    def room(x0):
        x1, L = x0 + 555.0, 555.0
        faces = [s.rect(ss.K_XZ, x0, x1, 0, L, 0, white, 1.0), s.rect(ss.K_XZ, x0, x1, 0, L, L, white, -1.0),
                 s.rect(ss.K_XY, x0, x1, 0, L, L, white, -1.0), s.rect(ss.K_YZ, 0, L, 0, L, x0, red, 1.0),
                 s.rect(ss.K_YZ, 0, L, 0, L, x1, red, -1.0), s.rect(ss.K_XY, x0, x1, 0, L, 0, white, 1.0)][:walls]
        return faces

    lamp = s.rect(ss.K_XZ, 213, 343, 227, 332, 554, light, -1.0)
    ball = s.sphere((300, 90, 250), 90, white)
    if two:
        items = [s.list(room(0.0) + [lamp]), s.list(room(600.0)), ball]
    elif nested:
        items = [s.list([s.list(room(0.0)), lamp]), ball]
    else:
        items = room(0.0) + [lamp, ball]
    s.root = s.list(items)
    s.biased = s.list([lamp])
    w = s.copy()
    w.set_list(w.root, [i for i in w.list_items(w.root) if i != ball])
    return s, w


# ---------------------------------------------------------------- the catalogue
class Entry:
    def __init__(self, name, build, features, kernel, fast, mode=0, depth=16, hooks=("MRT_FORCE_GENERIC",), rooms=None,
                 partial_tree=False, fast_leg=True, gpu=True):
        self.gpu = gpu
        self.name, self.build, self.features, self.kernel, self.fast = name, build, features, kernel, fast
        self.mode, self.depth, self.hooks, self.rooms, self.partial_tree, self.fast_leg = mode, depth, hooks, rooms, partial_tree, fast_leg

    def __repr__(self):
        return self.name


CORNELL = FT_LIN | FT_INST | FT_BIASED
ROOM_MESH = FT_LIN | FT_MESH | FT_BIASED
SKY_TREE = FT_LIN | FT_BVHW | FT_SKY | FT_METAL
GEN, NOSIG, NOBVHW = "MRT_FORCE_GENERIC", "MRT_NO_SIG", "MRT_NO_BVHW"
CATALOGUE = [
    Entry("a_cornell_plus_sphere", b_cornell_plus_sphere, CORNELL, V_LIN_INST, "fastz", rooms=1),
    Entry("b_cornell_lookalike", b_lookalike, CORNELL | SIG_CORNELL, V_CORNELL, "fastz", hooks=(GEN, NOSIG), rooms=1),
    Entry("b_cornell_lookalike_open_room", b_lookalike_open, CORNELL, V_LIN_INST, "fastz", rooms=0),
    Entry("c_room_mesh_lookalike", b_room_mesh, ROOM_MESH | SIG_ROOM_MESH, V_ROOM_MESH, "fastz", hooks=(GEN, NOSIG), rooms=1),
    Entry("c_room_mesh_lookalike_metal", b_room_mesh_metal, ROOM_MESH | FT_METAL | SIG_ROOM_MESH, V_ROOM_MESH_METAL, "pex",
          hooks=(GEN, NOSIG), rooms=1),
    Entry("c_room_mesh_plus_sphere", b_room_mesh_plus_sphere, ROOM_MESH, V_LIN_MESH, "fastz", rooms=1),
    Entry("d_biased_light_and_sphere", b_biased_sphere, CORNELL | SIG_CORNELL | FT_BSPHERE, V_ANY_LIN, "pex", rooms=1),
    Entry("d_biased_three_leaves_sky", b_biased_three_sky, CORNELL | FT_BSPHERE | FT_SKY, V_ANY_LIN, "pex", rooms=1),
    Entry("d_biased_bare_sphere", b_biased_bare_sphere, CORNELL | SIG_CORNELL | FT_BSPHERE, V_ANY_LIN, "pex", rooms=1),
    Entry("d_biased_bare_xz_rect", b_biased_bare_xz, CORNELL | SIG_CORNELL, V_CORNELL, "fastz", hooks=(GEN, NOSIG), rooms=1),
    Entry("e_biased_sphere_encloses_box", b_biased_enclosing_sphere, CORNELL | SIG_CORNELL | FT_BSPHERE, V_ANY_LIN, "pex", rooms=1),
    Entry("f_emissive_biased_sphere_mode1_depth1", b_biased_emissive_sphere, CORNELL | SIG_CORNELL | FT_BSPHERE, V_ANY_LIN, "pex",
          mode=1, depth=1, rooms=1),
    Entry("f_emissive_biased_sphere_mode1_depth3", b_biased_emissive_sphere, CORNELL | SIG_CORNELL | FT_BSPHERE, V_ANY_LIN, "pex",
          mode=1, depth=3, rooms=1),
    Entry("g_nopdf_xy_rect_in_biased_list", b_nopdf_xy_in_list, CORNELL | FT_BSPHERE, V_ANY_LIN, "pex", rooms=1),
    Entry("g_nopdf_bare_xy_rect", b_nopdf_bare_xy, CORNELL | FT_BSPHERE, V_ANY_LIN, "pex", rooms=1),
    Entry("g_nopdf_mesh_in_biased_list", b_nopdf_mesh_in_list, ROOM_MESH | SIG_ROOM_MESH | FT_BSPHERE, V_ANY_LIN, "pex", rooms=1),
    Entry("h_moving_sphere", b_moving_sphere, CORNELL | FT_MOVING, V_BOOK2, "pex", rooms=1),
    # (the uv-sampling ceiling is no wall candidate, so the light stands in for it and spans no face: no room)
    Entry("h_textures_metal_walls", b_textures, CORNELL | FT_TEX | FT_METAL | FT_UV, V_BOOK2, "pex", rooms=0),
    Entry("i_teapot_translate_rotate", lambda m: teapot_instance(m, True, 0), ROOM_MESH | FT_INST, V_ANY_LIN, "pex", rooms=1),
    Entry("i_teapot_translate_rotate_sky", lambda m: teapot_instance(m, True, 1), ROOM_MESH | FT_INST | FT_SKY, V_ANY_LIN, "pex", rooms=1),
    Entry("i_teapot_translate_sky", lambda m: teapot_instance(m, False, 1), ROOM_MESH | FT_INST | FT_SKY, V_ANY_LIN, "pex", rooms=1),
    Entry("j_tree_3000_spheres", b_big_tree, SKY_TREE, V_SKY, "fastz", hooks=(GEN, NOBVHW), rooms=0, partial_tree=True),
    Entry("j_tree_list_leaves", b_tree_list_leaves, SKY_TREE, V_SKY, "fastz", hooks=(GEN, NOBVHW), rooms=0),
    Entry("j_chain_depth_12", lambda m: chain(m, 12), SKY_TREE, V_SKY, "fastz", hooks=(GEN, NOBVHW), rooms=0),
    # The walks keep one LDS stack word per tree level and lane, and the kernels for these graphs run
    # 1024-thread groups (4 KiB per word): a chain of depth 40 or 70 needs more LDS than a group has,
    # and mrt_scene_upload refuses it on a GPU ("scene graph too deep for the LDS stacks").  The host
    # leg runs them (depth 70 is past the wide conversion: the generic bvh_node walk, FT_BVH).
    Entry("j_chain_depth_40", lambda m: chain(m, 40), SKY_TREE, V_SKY, "fastz", hooks=(GEN, NOBVHW), rooms=0, gpu=False),
    Entry("j_chain_depth_70", lambda m: chain(m, 70), FT_BVH | FT_SKY | FT_METAL, V_GENERIC, "pex", hooks=(), gpu=False),
    Entry("k_two_sphere_bvh_in_room", lambda m: b_bvh_in_room(m, 2), CORNELL | FT_BVHW, V_BOOK2, "pex", hooks=(GEN, NOBVHW), rooms=1),
    # (no MRT_NO_BVHW leg: the generic bvh_node walk of this tree beside an instance is too deep for the LDS stacks)
    Entry("k_big_tree_in_room", lambda m: b_bvh_in_room(m, 3000), CORNELL | FT_BVHW, V_BOOK2, "pex", hooks=(GEN,), rooms=1,
          partial_tree=True),
    Entry("k_one_object_bvh_in_room", lambda m: b_bvh_in_room(m, 1), CORNELL | FT_BVHW, V_BOOK2, "pex", hooks=(GEN, NOBVHW), rooms=1),
    Entry("l_live_volume_biased_sphere", b_volume_live, CORNELL | FT_VOLUME | FT_ISO | FT_BSPHERE, V_ANY_LIN, "pex",
          rooms=1),
    # (a linear program no FT_LIN variant covers: pick_variant falls through to the generic machine by itself)
    Entry("l_smoke_plus_metal_sphere", lambda m: smoke_plus(m, True), V_SMOKE | FT_METAL, V_GENERIC, "pex", hooks=(), rooms=1),
    Entry("l_smoke_plus_lambertian_sphere", lambda m: smoke_plus(m, False), V_SMOKE, V_SMOKE, "pex", rooms=1),
    Entry("m_mesh_reshaped", b_mesh_reshaped, ROOM_MESH | SIG_ROOM_MESH, V_ROOM_MESH, "fastz", hooks=(GEN, NOSIG), rooms=1),
    Entry("m_mesh_zero_area_triangles", b_mesh_degenerate, ROOM_MESH | SIG_ROOM_MESH, V_ROOM_MESH, "fastz", hooks=(GEN, NOSIG), rooms=1),
    Entry("n_translate_translate_sphere", b_nested_translate, FT_INST | FT_BIASED, V_GENERIC, "pex", hooks=()),
    Entry("n_bvh_with_instance_leaf", b_bvh_instance_leaf, FT_BVH | FT_INST | FT_BIASED, V_GENERIC, "pex", hooks=()),
    Entry("r_room_3_walls", lambda m: rooms(m, 3), FT_LIN | FT_BIASED, V_LIN_INST, "fastz", rooms=1),
    Entry("r_room_4_walls", lambda m: rooms(m, 4), FT_LIN | FT_BIASED, V_LIN_INST, "fastz", rooms=1),
    Entry("r_room_6_walls", lambda m: rooms(m, 6), FT_LIN | FT_BIASED, V_LIN_INST, "fastz", rooms=1),
    Entry("r_room_2_walls_is_no_room", lambda m: rooms(m, 2), FT_LIN | FT_BIASED, V_LIN_INST, "fastz", rooms=0),
    Entry("r_room_in_nested_list", lambda m: rooms(m, 5, nested=True), FT_LIN | FT_BIASED, V_LIN_INST, "fastz", rooms=1),
    Entry("r_two_rooms", lambda m: rooms(m, 5, two=True), FT_LIN | FT_BIASED, V_LIN_INST, "fastz", rooms=2),
    # Operands outside the exact contract's short-core ranges in the path kernels (DESIGN.md "Numerics", the
    # guard inventory): origins above and below 2^60 in one wave, MRT_F_SLOWDIV rect planes (planes off zero
    # drop SIG_CORNELL), boxes of a bvh_node tree at 2^50, mesh normals normalize cannot take its short path
    # on.  `without`: the unscaled / ordinary-plane graph.
    Entry("s_scaled_2p54", lambda m: (lookalike(m, scale=2.0 ** 54, glass=True), lookalike(m, glass=True)), CORNELL, V_LIN_INST, "fastz",
          rooms=0),  # (MRT_F_SLOWDIV walls are no room candidates)
    Entry("s_scaled_2p53_open_room", lambda m: (lookalike(m, closed=False, scale=2.0 ** 53, glass=True), lookalike(m, closed=False, glass=True)),
          CORNELL, V_LIN_INST, "fastz", rooms=0),
    # (planes at 1e-30 render the ordinary-plane image bit for bit at the host leg's size, so that graph cannot
    # be the `without`: the graph without its box is, as for b_cornell_lookalike)
    Entry("s_slowdiv_planes", lambda m: (lookalike(m, planes=1e-30), lookalike(m, planes=1e-30, with_box=False)), CORNELL, V_LIN_INST,
          "fastz", rooms=1),
    Entry("s_slowdiv_planes_small", lambda m: (lookalike(m, scale=0.125, planes=2.0 ** -80), lookalike(m)), CORNELL, V_LIN_INST, "fastz",
          rooms=1),
    Entry("s_tree_scaled", b_tree_scaled, SKY_TREE, V_SKY, "fastz", hooks=(GEN, NOBVHW), rooms=0),
    # fast_leg=False: the tolerance contract normalises by v_rsq_f32, which answers these normals (sums of 0,
    # ~1e-30, ~1e25: |n|^2 is 0 or inf in float) differently from the reference's a / sqrt(|a|^2) -- a zero or
    # NaN normal where the reference has inf or NaN -- and the paths part: measured at 128 x 128 x 64, rays
    # 3023808 against 3881302 (-22%, bound 1%), mean diff -1.379e-01 (bound 2e-3), rmse 1.159e+01 (bound
    # 0.05), image finite.  Outside the tolerance contract's operand range (DESIGN.md "Numerics contracts").
    Entry("s_mesh_scaled_and_degenerate_normals", lambda m: (degenerate_normals(m), room_mesh_lookalike(m, False)),
          ROOM_MESH | SIG_ROOM_MESH, V_ROOM_MESH, "fastz", hooks=(GEN, NOSIG), rooms=1, fast_leg=False),
]
IDS = [e.name for e in CATALOGUE]

_built = {}


def built(mrt, e):
    if e.name not in _built:
        _built[e.name] = e.build(mrt)
    return _built[e.name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host_parity(mrt, orc, e, s, w=48, h=48, spp=16):
    """CPU backend == restatement, bit for bit; returns the restatement's (image, rays)."""
    oimg, orays, _, _ = orc.render(s, orc.desc(w, h, spp, depth=e.depth, mode=e.mode, threads=16))
    r = mrt.Renderer(s, "cpu")
    cimg, crays = r.render(mrt.render_desc(w, h, spp, depth=e.depth, mode=e.mode, threads=16))
    feats = r.kernel_info()["features"]
    r.close()
    print(f"{e.name}: {w}x{h}x{spp} depth {e.depth} mode {e.mode}: CPU backend rays {crays}, restatement rays {orays}, "
          f"features {feats:#x}")
    assert crays == orays, (crays, orays)
    assert np.array_equal(bits(cimg), bits(oimg))
    return oimg, orays, feats


def lin_program(mrt, s, rewritten):
    fn = mrt.lib().mrt_debug_lin_program
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    fn.restype = C.c_int
    cap = 1 << 16
    codes, skips, n = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    assert fn(C.byref(s.view), int(rewritten), codes.ctypes.data, skips.ctypes.data, cap, n.ctypes.data) == 0
    return codes[:int(n[0])], skips[:int(n[0])]


# ---------------------------------------------------------------- host leg
@pytest.mark.parametrize("e", CATALOGUE, ids=IDS)
def test_host_backend_equals_restatement(mrt, orc, e):
    s, without = built(mrt, e)
    oimg, orays, feats = host_parity(mrt, orc, e, s)
    assert feats == e.features, (hex(feats), hex(e.features))
    wimg, wrays, _, _ = orc.render(without, orc.desc(48, 48, 16, depth=e.depth, mode=e.mode, threads=16))
    assert wrays != orays or not np.array_equal(bits(wimg), bits(oimg)), "the entry's addition changes nothing: it tests nothing"


@pytest.mark.parametrize("e", [e for e in CATALOGUE if e.features & FT_LIN], ids=lambda e: e.name)
def test_rewritten_program_structure(mrt, e):
    """mrt_sig.h lin_rewrite_fast on the catalogue's graphs: every LIST / INST skip lands on its END op,
    every MRT_F_VSUB volume's skip just past its sub-program, exactly one MRT_F_LAST, one LOP_ROOM +
    LOP_ROOMDATA pair per room the entry names."""
    LIST, LIST_END, INST, INST_END, VOLUME, ROOM, ROOMDATA, END = 3, 4, 5, 6, 8, 10, 11, 0
    s, _ = built(mrt, e)
    for rewritten in (False, True):
        c, k = lin_program(mrt, s, rewritten)
        op, fl = c & 0xFF, (c >> 16) & 0xFF
        assert len(op) >= 2 and op[-1] == END
        for i in range(len(op)):
            if op[i] in (LIST, INST):
                assert i < k[i] < len(op) and op[k[i]] == (LIST_END if op[i] == LIST else INST_END), (rewritten, i, op[i], k[i])
            if op[i] == INST_END:
                assert k[i] < i and op[k[i]] == INST and k[k[i]] == i, (rewritten, i, k[i])
            if op[i] == VOLUME and fl[i] & 0x80:
                # the boundary sub-program: one LIST or INST whose END op is the last op before the skip
                assert i + 1 < k[i] <= len(op) - 1 and op[i + 1] in (LIST, INST) and k[i + 1] == k[i] - 1, (rewritten, i, k[i])
        if rewritten:
            assert int((fl & 0x40 != 0).sum()) == 1
            at = [i for i in range(len(op)) if op[i] == ROOM]
            assert len(at) == e.rooms and all(op[i + 1] == ROOMDATA for i in at), (at, e.rooms)
            assert int((op == ROOMDATA).sum()) == e.rooms
        else:
            assert ROOM not in op and not (fl & 0x40).any()
    if e.features & FT_VSUB:
        assert any(o == VOLUME and f & 0x80 for o, f in zip(op, fl))


# ---------------------------------------------------------------- GPU leg
@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def gpu_paths(mrt, r, d):
    ns = d.sqrt_samples ** 2
    px = mrt.local_pixels(d)
    prgb, prays = r.paths(len(px) * ns)
    full_rgb = np.zeros((d.width * d.height, ns, 3), dtype=np.float32)
    full_rays = np.zeros((d.width * d.height, ns), dtype=np.uint32)
    full_rgb[px] = prgb.reshape(ns, len(px), 3).transpose(1, 0, 2)
    full_rays[px] = prays.reshape(ns, len(px)).T
    return full_rgb.reshape(-1, 3), full_rays.reshape(-1)


SIZES = sorted(((w * w * spp, w, spp) for w in (64, 96, 128) for spp in (16, 64)))


def launch_size(ki):
    """The smallest size that gives every lane of the launch several paths (so lanes regenerate
    paths and every wave claims work), capped at 128 x 128 x 64."""
    need = 4 * ki["grid"] * ki["wg"]
    for paths, w, spp in SIZES:
        if paths >= need:
            return w, spp
    return 128, 64


def assert_exact(mrt, r, e, w, spp, ref, what, numerics="exact"):
    oimg, orays, prgb, prays = ref
    d = mrt.render_desc(w, w, spp, depth=e.depth, mode=e.mode, numerics=numerics, flags=mrt._lib.RF_PATH_DEBUG)
    img, rays = r.render(d)
    grgb, grays = gpu_paths(mrt, r, d)
    print(f"{e.name} [{what}]: {w}x{w}x{spp}: GPU rays {rays}, restatement rays {orays}")
    assert rays == orays, (what, rays, orays)
    assert np.array_equal(grays, prays), what
    # A NaN equals a NaN: invalid operations (0 / 0, sqrt of a negative) give x86's default NaN
    # 0xFFC00000 on the host and the GPU's 0x7FC00000, and the sign of a NaN is no value -- the fold
    # replaces every non-finite sample (main.cpp:162-164), which the image and ray equalities pin.
    same = (bits(grgb) == bits(prgb)) | (np.isnan(grgb) & np.isnan(prgb))
    bad = np.nonzero(~same.all(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} paths differ, first {bad[:5]}: GPU {[hex(x) for x in bits(grgb)[bad[:5]].ravel()]} "
                           f"restatement {[hex(x) for x in bits(prgb)[bad[:5]].ravel()]}; of them NaN on both sides "
                           f"{int((np.isnan(grgb[bad]).any(axis=1) & np.isnan(prgb[bad]).any(axis=1)).sum())}")
    assert np.array_equal(bits(img), bits(oimg)), what
    return rays


@pytest.mark.gpu
@pytest.mark.parametrize("e", [e for e in CATALOGUE if e.gpu], ids=lambda e: e.name)
def test_gpu_equals_restatement(gpu, orc, e, monkeypatch):
    mrt = gpu
    s, _ = built(mrt, e)
    host_parity(mrt, orc, e, s)  # a graph the two host implementations disagree on must not reach the GPU
    r = mrt.Renderer(s, 0)
    ki = r.kernel_info()
    print(f"{e.name}: features {ki['features']:#x} kernel {ki['kernel_features']:#x} grid {ki['grid']} wg {ki['wg']} "
          f"tree_nodes {ki['tree_nodes']} (exact build)")
    assert ki["features"] == e.features, (hex(ki["features"]), hex(e.features))
    assert ki["kernel_features"] == e.kernel, (hex(ki["kernel_features"]), hex(e.kernel))
    inner = int(((s.nodes["kind"] & 0xFF) == ss.K_BVH).sum())
    if e.partial_tree:
        assert 0 < ki["tree_nodes"] < inner, (ki["tree_nodes"], inner)
    w, spp = launch_size(ki)
    ref = orc.render(s, orc.desc(w, w, spp, depth=e.depth, mode=e.mode, threads=16), paths=True)
    exact_rays = assert_exact(mrt, r, e, w, spp, ref, "exact")
    for hook in e.hooks:
        with monkeypatch.context() as mp:
            mp.setenv(hook, "1")
            rh = mrt.Renderer(s, 0)
        assert rh.kernel_info()["kernel_features"] != e.kernel or hook == NOBVHW, hook
        assert_exact(mrt, rh, e, w, spp, ref, hook)
        rh.close()
    if e.fast_leg:
        ref64 = ref if spp == 64 else orc.render(s, orc.desc(w, w, 64, depth=e.depth, mode=e.mode, threads=16))
        fimg, frays = r.render(mrt.render_desc(w, w, 64, depth=e.depth, mode=e.mode, numerics="fast"))
        kf = r.kernel_info()
        d = fimg[..., :3].astype(np.float64) - ref64[0][..., :3]
        rmse = float(np.sqrt((d ** 2).mean()))
        print(f"{e.name} [fast]: build {mrt._lib.BUILDS[kf['build']]} tree_nodes {kf['tree_nodes']} rays {frays} vs {ref64[1]} "
              f"mean diff {d.mean():.3e} rmse {rmse:.3e} handover_lost {kf['handover_lost']}")
        assert mrt._lib.BUILDS[kf["build"]] == e.fast
        assert np.isfinite(fimg).all() and kf["handover_lost"] == 0
        if e.partial_tree:
            assert 0 < kf["tree_nodes"] < inner, (kf["tree_nodes"], inner)
        assert abs(frays / ref64[1] - 1) < 1e-2
        assert abs(d.mean()) < 2e-3
        assert rmse < 0.05
        if e.fast == "pex":  # the path-exact build: "the paths are the same" 
            assert frays == ref64[1]
            # ... and each one's radiance is the forward fold of the same levels: per path, per pixel and
            # in the ray total the build equals the restatement's forward fold bit for bit, through
            # every walk of the entry's hooks that runs it
            fwd = orc.render(s, orc.desc(w, w, 64, depth=e.depth, mode=e.mode, threads=16, fold=1), paths=True)
            assert_exact(mrt, r, e, w, 64, fwd, "pex", numerics="fast")
            assert mrt._lib.BUILDS[r.kernel_info()["build"]] == "pex"
            for hook in e.hooks:
                with monkeypatch.context() as mp:
                    mp.setenv(hook, "1")
                    rh = mrt.Renderer(s, 0)
                rh.render(mrt.render_desc(16, 16, 1, depth=e.depth, mode=e.mode, numerics="fast"))
                build = mrt._lib.BUILDS[rh.kernel_info()["build"]]
                print(f"{e.name} [fast, {hook}]: build {build}")
                if build == "pex":
                    assert_exact(mrt, rh, e, w, 64, fwd, f"pex {hook}", numerics="fast")
                rh.close()
    r.close()
