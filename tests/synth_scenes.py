"""Scene views built by hand for tests: graphs the ten reference scenes never produce.

A Synth holds the arrays of an mrt_scene_view (include/mrt_scene.h) as numpy arrays / lists that
tests edit freely; `.view` freezes them into an MrtSceneView and keeps the arrays alive.  A Synth
goes wherever a Scene goes: mrt.Renderer(s, dev), oracle.render(s, ...), mrt_debug_lin_program.

Both the product and the restatement consume the same view, so boxes may be loose and instance
sines need not be correctly rounded: a parity test only needs both sides to read the same numbers.
"""
import ctypes as C

import numpy as np

NODE = np.dtype([("kind", "<u4"), ("a", "<u4"), ("b", "<u4"), ("mat", "<u4"), ("f", "<f4", (12,))])
MATERIAL = np.dtype([("kind", "<u4"), ("tex", "<u4"), ("p", "<f4"), ("pad", "<f4")])
TEXTURE = np.dtype([("kind", "<u4"), ("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("f", "<f4", (4,))])
MESH_NODE = np.dtype([("bmin", "<f4", (3,)), ("left_or_first", "<u4"), ("bmax", "<f4", (3,)), ("count_order", "<u4")])
assert NODE.itemsize == 64 and MATERIAL.itemsize == 16 and TEXTURE.itemsize == 32 and MESH_NODE.itemsize == 32

NONE = 0xFFFFFFFF
K_LIST, K_BVH, K_MESH, K_TRANSLATE, K_ROTY, K_SPHERE, K_XY, K_XZ, K_YZ, K_VOLUME = range(1, 11)
F_HASBOX, F_MOVING = 1, 2
M_LAMBERTIAN, M_ISOTROPIC, M_METAL, M_DIELECTRIC, M_LIGHT = range(1, 6)
T_COLOR, T_CHECKER, T_PERLIN, T_IMAGE = range(1, 5)

# kernel feature bits (miniraytracer_amd/csrc/mrt_trace.h)
FT_BVH, FT_MESH, FT_VOLUME, FT_INST, FT_TEX, FT_METAL, FT_ISO, FT_MOVING, FT_SKY, FT_BSPHERE, FT_UV, FT_LIN, FT_BVHW, FT_BIASED, \
    FT_VSUB = (1 << i for i in range(15))
FT_ALL = 0x37FF


def _arr(ptr, n, dtype):
    """Copy n records of a view's array."""
    dtype = np.dtype(dtype)
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_uint8 * (int(n) * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


class Synth:
    def __init__(self, scene=None):
        """Copy of `scene`'s view (a Scene from select_scene; camera, Perlin tables and texels come
        along).  clear() then drops the graph and keeps those."""
        from miniraytracer_amd._lib import MrtCamera
        self.scene_id = 0
        self.camera = MrtCamera()
        self.root, self.biased, self.sky = 0, NONE, 0
        self.nodes = np.zeros(0, dtype=NODE)
        self.children = np.zeros(0, dtype=np.uint32)
        self.mesh_nodes = np.zeros(0, dtype=MESH_NODE)
        self.tri_geo = np.zeros((0, 12), dtype=np.float32)
        self.tri_nrm = np.zeros((0, 12), dtype=np.float32)
        self.materials = np.zeros(0, dtype=MATERIAL)
        self.textures = np.zeros(0, dtype=TEXTURE)
        self.perlin_ranvec = np.zeros((256, 4), dtype=np.float32)
        self.perlin_perm = np.zeros(768, dtype=np.int32)
        self.texels = np.zeros(0, dtype=np.uint8)
        self._view = None
        if scene is not None:
            v = scene.view
            self.scene_id, self.root, self.biased, self.sky = v.scene_id, v.root, v.biased, v.sky
            C.memmove(C.byref(self.camera), C.byref(v.camera), C.sizeof(MrtCamera))
            self.nodes = _arr(v.nodes, v.n_nodes, NODE)
            self.children = _arr(v.children, v.n_children, np.uint32)
            self.mesh_nodes = _arr(v.mesh_nodes, v.n_mesh_nodes, MESH_NODE)
            self.tri_geo = _arr(v.tri_geo, v.n_tris * 12, np.float32).reshape(-1, 12)
            self.tri_nrm = _arr(v.tri_nrm, v.n_tris * 12, np.float32).reshape(-1, 12)
            self.materials = _arr(v.materials, v.n_materials, MATERIAL)
            self.textures = _arr(v.textures, v.n_textures, TEXTURE)
            self.perlin_ranvec = _arr(v.perlin_ranvec, 1024, np.float32).reshape(256, 4)
            self.perlin_perm = _arr(v.perlin_perm, 768, np.int32)
            self.texels = _arr(v.texels, v.n_texels, np.uint8)

    def clear(self):
        """Drop the graph (nodes, children, meshes, materials, textures); keep camera, Perlin, texels."""
        self.nodes = np.zeros(0, dtype=NODE)
        self.children = np.zeros(0, dtype=np.uint32)
        self.mesh_nodes = np.zeros(0, dtype=MESH_NODE)
        self.tri_geo = np.zeros((0, 12), dtype=np.float32)
        self.tri_nrm = np.zeros((0, 12), dtype=np.float32)
        self.materials = np.zeros(0, dtype=MATERIAL)
        self.textures = np.zeros(0, dtype=TEXTURE)
        self.root, self.biased, self._view = 0, NONE, None
        return self

    def copy(self):
        import copy
        s = copy.copy(self)
        for k in ("nodes", "children", "mesh_nodes", "tri_geo", "tri_nrm", "materials", "textures", "texels"):
            setattr(s, k, getattr(self, k).copy())
        s.camera = type(self.camera).from_buffer_copy(self.camera)
        s._view = None
        return s

    # ---- records
    def _push(self, name, rec):
        self._view = None
        a = getattr(self, name)
        setattr(self, name, np.concatenate([a, rec.reshape(1)]))
        return len(a)

    def node(self, kind, a=0, b=0, mat=NONE, f=(), flags=0, order=0):
        n = np.zeros((), dtype=NODE)
        n["kind"] = kind | (order << 8) | (flags << 16)
        n["a"], n["b"], n["mat"] = a, b, mat
        n["f"][:len(f)] = np.asarray(f, dtype=np.float32)
        return self._push("nodes", n)

    def texture(self, kind, a=0, b=0, c=0, f=()):
        t = np.zeros((), dtype=TEXTURE)
        t["kind"], t["a"], t["b"], t["c"] = kind, a, b, c
        t["f"][:len(f)] = np.asarray(f, dtype=np.float32)
        return self._push("textures", t)

    def color(self, r, g, b):
        return self.texture(T_COLOR, f=(r, g, b))

    def material(self, kind, tex=NONE, p=0.0):
        m = np.zeros((), dtype=MATERIAL)
        m["kind"], m["tex"], m["p"] = kind, tex, p
        return self._push("materials", m)

    def lambertian(self, r, g, b):
        return self.material(M_LAMBERTIAN, self.color(r, g, b))

    # ---- objects
    def sphere(self, center, radius, mat, center1=None, t0=0.0, t1=1.0):
        c1 = center if center1 is None else center1
        return self.node(K_SPHERE, mat=mat, f=list(center) + list(c1) + [t0, t1, radius],
                         flags=F_MOVING if center1 is not None else 0)

    def rect(self, kind, a0, a1, b0, b1, k, mat, sign=1.0):
        return self.node(kind, mat=mat, f=(a0, a1, b0, b1, k, sign))

    def run(self, items):
        """Append a children run; returns its first slot."""
        self._view = None
        first = len(self.children)
        self.children = np.concatenate([self.children, np.asarray(items, dtype=np.uint32)])
        return first

    def list(self, items, box=None):
        return self.node(K_LIST, a=self.run(items), b=len(items), f=box if box is not None else (),
                         flags=F_HASBOX if box is not None else 0)

    def set_list(self, node, items, box=None):
        """Re-point an object_list at a new children run."""
        self.nodes[node]["a"], self.nodes[node]["b"] = self.run(items), len(items)
        if box is not None:
            self.nodes[node]["f"][:6] = np.asarray(box, dtype=np.float32)

    def list_items(self, node):
        n = self.nodes[node]
        return [int(x) for x in self.children[int(n["a"]):int(n["a"]) + int(n["b"])]]

    def box(self, p0, p1, mat):
        """box.h:12-20: the object_list of six rects, in its order, with its box."""
        x0, y0, z0 = p0
        x1, y1, z1 = p1
        items = [self.rect(K_XY, x0, x1, y0, y1, z1, mat, 1.0), self.rect(K_XY, x0, x1, y0, y1, z0, mat, -1.0),
                 self.rect(K_XZ, x0, x1, z0, z1, y1, mat, 1.0), self.rect(K_XZ, x0, x1, z0, z1, y0, mat, -1.0),
                 self.rect(K_YZ, y0, y1, z0, z1, x1, mat, 1.0), self.rect(K_YZ, y0, y1, z0, z1, x0, mat, -1.0)]
        return self.list(items, box=(x0, y0, z0, x1, y1, z1))

    def translate(self, child, offset):
        return self.node(K_TRANSLATE, a=child, f=offset)

    def rotate_y(self, child, degrees, box=None):
        rad = np.float32(degrees) * np.float32(np.pi / 180.0)
        f = list(box if box is not None else [0] * 6) + [np.float32(np.sin(rad)), np.float32(np.cos(rad))]
        return self.node(K_ROTY, a=child, f=f, flags=F_HASBOX if box is not None else 0)

    def volume(self, boundary, density, rgb):
        return self.node(K_VOLUME, a=boundary, mat=self.material(M_ISOTROPIC, self.color(*rgb)), f=(density,))

    def bvh(self, items, boxes, split=lambda n: n // 2, orders=None):
        """bvh_node tree over `items` in the given order; boxes[i] = (min xyz, max xyz) of items[i].
        split(n) -> how many of n items go left (1 <= . < n); one item gives bvh_node(x, x), the
        reference's one-object case.  orders: a Generator drawing each node's order byte (default 0)."""
        boxes = np.asarray(boxes, dtype=np.float32).reshape(len(items), 6)

        def build(lo, hi):
            if hi - lo == 1:
                return items[lo], boxes[lo]
            k = lo + max(1, min(hi - lo - 1, int(split(hi - lo))))
            (l, lb), (r, rb) = build(lo, k), build(k, hi)
            bx = np.concatenate([np.minimum(lb[:3], rb[:3]), np.maximum(lb[3:], rb[3:])])
            order = int(orders.integers(0, 256)) if orders is not None else 0
            return self.node(K_BVH, a=l, b=r, f=bx, order=order), bx

        if len(items) == 1:
            return self.node(K_BVH, a=items[0], b=items[0], f=boxes[0],
                             order=int(orders.integers(0, 256)) if orders is not None else 0)
        # the recursion is as deep as the tree: chains of ~70 stay well inside Python's limit
        return build(0, len(items))[0]

    def set_mesh(self, mesh_nodes, tri_geo=None, tri_nrm=None):
        self._view = None
        self.mesh_nodes = np.ascontiguousarray(mesh_nodes, dtype=MESH_NODE)
        if tri_geo is not None:
            self.tri_geo = np.ascontiguousarray(tri_geo, dtype=np.float32).reshape(-1, 12)
            self.tri_nrm = np.ascontiguousarray(tri_nrm, dtype=np.float32).reshape(-1, 12)

    def scale_camera(self, s):
        """The same view of a scene scaled by s about the origin (positions and the focus-plane
        extents scale; the unit axes u, v, w stay)."""
        self._view = None
        for name in ("origin", "llcorner", "horz", "vert"):
            a = getattr(self.camera, name)
            for i in range(4):
                a[i] = float(np.float32(a[i]) * np.float32(s))
        self.camera.lens_radius = float(np.float32(self.camera.lens_radius) * np.float32(s))

    def find(self, kind, **where):
        """Indices of the nodes of a kind (optionally with mat=...)."""
        m = (self.nodes["kind"] & 0xFF) == kind
        for k, val in where.items():
            m &= self.nodes[k] == val
        return [int(i) for i in np.nonzero(m)[0]]

    # ---- the frozen view
    @property
    def view(self):
        if self._view is None:
            from miniraytracer_amd._lib import MrtSceneView
            keep = {k: np.ascontiguousarray(getattr(self, k)) for k in
                    ("nodes", "children", "mesh_nodes", "tri_geo", "tri_nrm", "materials", "textures", "perlin_ranvec",
                     "perlin_perm", "texels")}
            v = MrtSceneView()
            v.scene_id, v.root, v.biased, v.sky = self.scene_id, int(self.root), int(self.biased), int(self.sky)
            v.camera = self.camera
            for k, a in keep.items():
                setattr(v, k, a.ctypes.data)
            v.n_nodes, v.n_children, v.n_mesh_nodes = len(keep["nodes"]), len(keep["children"]), len(keep["mesh_nodes"])
            v.n_tris, v.n_materials, v.n_textures = len(keep["tri_geo"]), len(keep["materials"]), len(keep["textures"])
            v.n_texels = len(keep["texels"])
            self._keep = keep
            self._view = v
        return self._view

    def close(self):
        pass
