"""Edge-operand rays for the exact contract's range guards (DESIGN.md "Numerics", the guard inventory).

The exact contract's device code takes short cores (recip_nr, div_core, sqrt_core) inside operand
ranges and IEEE forms behind a wave ballot outside them (mrt_device.h ray_nice / ray_inv / normalize /
aabb_hit_b, mrt_lin.h lin_prim_t).  edge_rays() builds, deterministically from a view and a seed, caller
rays on both sides of each range, one class label per ray:

axis       the six axis directions and directions with one component +0.0 / -0.0, at lengths 1, 2^-60, 2^25
thin       one direction component at 2^-25 ... a subnormal after normalisation, both signs
norm       |d|^2 at 2^-52, 2^52 (and their float neighbours), 2^-100, 2^100, overflow; one component
           nonzero and below 2^-100
origin     one origin component at +-0, +-2^-77 (and neighbours), a subnormal, +-2^60 (and the float
           above), +-2^100
plane      origins on a rect's plane and one ulp to either side
box        origins on a bvh_node / mesh / list box plane with an axis direction lying in that plane
           (0 * inf = NaN slab values)
instance   origins at a translate's offset and one ulp from it, directions whose rotate_y image has a
           component below 2^-26
ordinary   test_cast_host.entry_rays, the filler of mixed waves
nonfinite  (nonfinite_rays, kept apart) NaN / +-inf in one component, a zero direction, 3e38 directions

ray_flags() restates normalize's and ray_nice's range tests in numpy, on the float bits.
"""
import numpy as np

import synth_scenes as ss

F32 = np.float32
FIXTURE_LIMIT, LIMIT = 2048, 4096
FINITE_CLASSES = ("axis", "thin", "norm", "origin", "plane", "box", "instance", "ordinary")
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- the guards, restated
def _mag2(x):
    """mrt_device.h mag2: |x| as an unsigned key (the sign shifted out)."""
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.int64) << 1) & M32


def _key(e):
    return (e + 127) << 24


def _mag_in(x, lo, hi):
    return ((_mag2(x) - _key(lo)) & M32) < (_key(hi) - _key(lo))


def unit(d):
    """Vec3::normalize in float32, the host form: (d / sqrt((x*x + y*y) + z*z), |d|^2)."""
    d = np.ascontiguousarray(d, dtype=F32)
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return d / np.sqrt(dd)[:, None], dd


def ray_flags(o, d):
    """dict of bool arrays for rays (o, d): norm_ok (normalize's short path: |d|^2 in [2^-52, 2^52),
    every component 0 or >= 2^-100), dir_ok (every normalised component in [2^-26, 2)), o_small (a
    nonzero origin component below 2^-77), o_large (one above 2^60), nice (ray_nice)."""
    o = np.ascontiguousarray(o, dtype=F32)
    dn, dd = unit(d)
    norm_ok = _mag_in(dd, -52, 52) & ((((_mag2(d) - 1) & M32).min(axis=1)) >= _key(-100) - 1)
    dir_ok = _mag_in(dn, -26, 1).all(axis=1)
    o_small = (((_mag2(o) - 1) & M32).min(axis=1)) < _key(-77) - 1
    o_large = _mag2(o).max(axis=1) > _key(60)  # (a NaN's key is above every finite one)
    return dict(norm_ok=norm_ok, dir_ok=dir_ok, o_small=o_small, o_large=o_large, nice=dir_ok & ~o_small & ~o_large)


# the sides of the guards a cast ray decides by itself: (name, mask from ray_flags)
GUARD_SIDES = (("normalize: short path", lambda f: f["norm_ok"]), ("normalize: IEEE fallback", lambda f: ~f["norm_ok"]),
               ("ray_nice: nice", lambda f: f["nice"]), ("ray_nice: direction out of range", lambda f: ~f["dir_ok"]),
               ("ray_nice: origin below 2^-77", lambda f: f["o_small"]), ("ray_nice: origin above 2^60", lambda f: f["o_large"]))


# ---------------------------------------------------------------- the view's numbers
RECT_AXES = {ss.K_XY: (0, 1, 2), ss.K_XZ: (0, 2, 1), ss.K_YZ: (1, 2, 0)}


def _anchors(s):
    """Centres of the view's primitives (spheres, rects, mesh root boxes), in their own frames."""
    nodes = np.asarray(s.nodes)
    kind = nodes["kind"] & 0xFF
    out = [n["f"][0:3].astype(np.float64) for n in nodes[kind == ss.K_SPHERE]]
    for k, (a, b, c) in RECT_AXES.items():
        for n in nodes[kind == k]:
            p = np.zeros(3)
            p[a], p[b], p[c] = 0.5 * (n["f"][0] + n["f"][1]), 0.5 * (n["f"][2] + n["f"][3]), n["f"][4]
            out.append(p)
    for n in nodes[kind == ss.K_MESH]:
        m = s.mesh_nodes[int(n["a"])]
        out.append(0.5 * (m["bmin"].astype(np.float64) + m["bmax"]))
    return np.asarray(out)


def _boxes(s):
    """(min xyz, max xyz) rows of every box a walk tests: bvh_node, boxed lists and rotate_y, mesh nodes."""
    nodes = np.asarray(s.nodes)
    kind, flags = nodes["kind"] & 0xFF, nodes["kind"] >> 16
    rows = [n["f"][:6] for n in nodes[(kind == ss.K_BVH) | (((kind == ss.K_LIST) | (kind == ss.K_ROTY)) & ((flags & ss.F_HASBOX) != 0))]]
    rows += [np.concatenate([m["bmin"], m["bmax"]]) for m in np.asarray(s.mesh_nodes)]
    rows = np.asarray(rows, dtype=F32).reshape(-1, 6)
    return rows[np.isfinite(rows).all(axis=1) & (np.abs(rows) < 1e30).all(axis=1)]


class _Gen:
    def __init__(self, mrt, s, seed):
        from test_cast_host import scene_bounds
        self.mrt, self.s, self.rng = mrt, s, np.random.default_rng(seed)
        self.lo, self.hi = scene_bounds(s)
        self.anchors = _anchors(s)
        self.cam = np.array(s.camera.origin[:3], dtype=np.float64)
        if not np.isfinite(self.cam).all():
            self.cam = 0.5 * (self.lo + self.hi)
        self.o, self.d, self.label = [], [], []

    def targets(self, n):
        a = self.anchors[self.rng.integers(0, len(self.anchors), n)]
        return a + self.rng.normal(0.0, 1.0, (n, 3)) * 0.02 * np.minimum(self.hi - self.lo, 1000.0)

    def origins(self, n):
        """Points between the camera and the scene's primitives: inside the bounds' hull with the
        camera, mostly in free space."""
        u = self.rng.uniform(0.05, 0.8, (n, 1))
        return (self.cam + u * (self.targets(n) - self.cam)).astype(F32)

    def aimed(self, o):
        d = self.targets(len(o)) - o.astype(np.float64)
        d /= np.linalg.norm(d, axis=1)[:, None]
        # no component near the thin range by accident
        d = np.where(np.abs(d) < 1e-3, 1e-3, d)
        return d.astype(F32)

    def add(self, label, o, d):
        o, d = np.asarray(o, dtype=F32).reshape(-1, 3), np.asarray(d, dtype=F32).reshape(-1, 3)
        assert len(o) == len(d)
        self.o.append(o)
        self.d.append(d)
        self.label += [label] * len(o)

    # ---- classes
    def axis(self, k):
        o = self.origins(k)
        lengths = (F32(1.0), F32(2.0 ** -60), F32(2.0 ** 25))
        zeros = ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0))
        for i in range(k):
            for j in range(6):
                d = np.zeros(3, dtype=F32)
                ax = j % 3
                z = zeros[(i + j) % 4]
                d[(ax + 1) % 3], d[(ax + 2) % 3] = z
                d[ax] = (1.0 if j < 3 else -1.0) * lengths[(i + j) % 3]
                self.add("axis", o[i], d)
        # one component exactly +0 / -0, the other two aimed
        o = self.origins(k)
        d = self.aimed(np.repeat(o, 6, axis=0)).reshape(k, 6, 3)
        for j in range(6):
            d[:, j, j % 3] = 0.0 if j < 3 else -0.0
        d *= np.asarray(lengths, dtype=F32)[(np.arange(k)[:, None] + np.arange(6)[None, :]) % 3][:, :, None]
        self.add("axis", np.repeat(o, 6, axis=0), d.reshape(-1, 3))

    def thin(self, k):
        """One component whose normalised value is v: 2^-25, the float below 2^-26, 2^-26, 2^-27,
        2^-40, 2^-100, a subnormal; both signs, each axis."""
        below = np.nextafter(F32(2.0 ** -26), F32(0))
        vals = (F32(2.0 ** -25), below, F32(2.0 ** -26), F32(2.0 ** -27), F32(2.0 ** -40), F32(2.0 ** -100), F32(2.0 ** -140))
        for v in vals:
            for sign in (1.0, -1.0):
                for ax in range(3):
                    o = self.origins(k)
                    d = self.aimed(o)
                    d[:, ax] = 0.0
                    ln = np.sqrt(unit(d)[1])
                    for i in range(k):
                        # the float c with RN(c / |d|) == v, searched among the neighbours of RN(v * |d|)
                        c = F32(v * ln[i])
                        cand = [c]
                        for _ in range(6):
                            cand = [np.nextafter(cand[0], F32(0))] + cand + [np.nextafter(cand[-1], F32(np.inf))]
                        q = np.array([unit(np.array([[x if a == ax else d[i, a] for a in range(3)]], dtype=F32))[0][0, ax] for x in cand])
                        d[i, ax] = sign * cand[int(np.argmin(np.abs(q.astype(np.float64) - float(v))))]
                    self.add("thin", o, d)

    def norm(self, k):
        """|d|^2 at the edges of normalize's short path."""
        def scale_to(dd_target):
            return np.sqrt(float(dd_target))

        edges = []
        for e in (-52, 52):
            x = F32(2.0 ** e)
            edges += [np.nextafter(x, F32(0)), x, np.nextafter(x, F32(np.inf))]
        edges += [F32(2.0 ** -100), F32(2.0 ** 100)]
        for t in edges:
            o = self.origins(k)
            d = self.aimed(o).astype(np.float64)
            d = (d / np.linalg.norm(d, axis=1)[:, None] * scale_to(t)).astype(F32)
            # walk the largest component by ulps until |d|^2 is the target (or as near as it gets)
            for i in range(k):
                ax = int(np.argmax(np.abs(d[i])))
                for _ in range(64):
                    dd = unit(d[i:i + 1])[1][0]
                    if dd == t:
                        break
                    d[i, ax] = np.nextafter(d[i, ax], np.copysign(F32(np.inf), d[i, ax]) if dd < t else F32(0))
            self.add("norm", o, d)
        for sc in (2.0 ** 64, 2.0 ** 70):  # |d|^2 overflows
            o = self.origins(k)
            self.add("norm", o, (self.aimed(o).astype(np.float64) * sc).astype(F32))
        for tiny in (2.0 ** -101, 2.0 ** -120, 2.0 ** -149):  # one component nonzero and below 2^-100, the others O(1)
            o = self.origins(k)
            d = self.aimed(o)
            d[np.arange(k), self.rng.integers(0, 3, k)] = F32(tiny) * np.where(self.rng.random(k) < 0.5, -1, 1).astype(F32)
            self.add("norm", o, d)

    def origin(self, k):
        up = F32(np.inf)
        small, big = F32(2.0 ** -77), F32(2.0 ** 60)
        vals = [F32(0.0), np.nextafter(small, F32(0)), small, np.nextafter(small, up), F32(2.0 ** -149), F32(2.0 ** -130),
                big, np.nextafter(big, up), F32(2.0 ** 100)]
        for v in vals:
            for sign in (1.0, -1.0):
                for ax in range(3):
                    o = self.origins(k)
                    o[:, ax] = sign * v
                    d = self.aimed(o)
                    if v >= big:
                        # from that far only the axis direction back to the scene keeps the other two
                        # coordinates: t = |o_ax| exactly, p = o on the other axes
                        d[:] = 0.0
                        d[:, ax] = -sign
                        d[1::2] = self.aimed(o)[1::2]
                    self.add("origin", o, d)

    def plane(self, k):
        nodes = np.asarray(self.s.nodes)
        kind = nodes["kind"] & 0xFF
        rects = [n for n in nodes if int(n["kind"]) & 0xFF in RECT_AXES]
        if not rects:
            return
        pick = self.rng.permutation(len(rects))[:k]
        for i in pick:
            n = rects[int(i)]
            a, b, c = RECT_AXES[int(n["kind"]) & 0xFF]
            kk = F32(n["f"][4])
            for off in (kk, np.nextafter(kk, F32(-np.inf)), np.nextafter(kk, F32(np.inf))):
                o = self.origins(4)
                o[:, c] = off
                o[:2, a] = F32(n["f"][0]) + self.rng.random(2).astype(F32) * (F32(n["f"][1]) - F32(n["f"][0]))
                o[:2, b] = F32(n["f"][2]) + self.rng.random(2).astype(F32) * (F32(n["f"][3]) - F32(n["f"][2]))
                d = self.aimed(o)
                d[0] = 0.0
                d[0, c] = 1.0 if i % 2 else -1.0   # perpendicular to the plane
                d[1, c] = 0.0                       # in the plane
                self.add("plane", o, d)
        del kind

    def box(self, k):
        boxes = _boxes(self.s)
        if not len(boxes):
            return
        for i in self.rng.integers(0, len(boxes), k):
            bx = boxes[int(i)]
            ax = int(self.rng.integers(0, 3))
            o = (bx[:3] + self.rng.random(3).astype(F32) * (bx[3:] - bx[:3])).astype(F32)
            o = np.minimum(np.maximum(o, bx[:3]), bx[3:])
            o[ax] = bx[ax + 3 * int(self.rng.integers(0, 2))]
            for other in ((ax + 1) % 3, (ax + 2) % 3):
                for sign in (1.0, -1.0):
                    d = np.zeros(3, dtype=F32)
                    d[other] = sign
                    self.add("box", o, d)

    def instance(self, k):
        nodes = np.asarray(self.s.nodes)
        kind = nodes["kind"] & 0xFF
        up, dn = F32(np.inf), F32(-np.inf)
        for n in nodes[kind == ss.K_TRANSLATE][:4]:
            off = n["f"][:3].astype(F32)
            rows = [off.copy(), np.nextafter(off, up), np.nextafter(off, dn)]
            for ax in range(3):
                for v in (off[ax], np.nextafter(off[ax], up), np.nextafter(off[ax], dn)):
                    o = self.origins(1)[0]
                    o[ax] = v
                    rows.append(o)
            rows = np.repeat(np.asarray(rows, dtype=F32), k, axis=0)
            self.add("instance", rows, self.aimed(rows))
        for n in nodes[kind == ss.K_ROTY][:4]:
            s, c = F32(n["f"][6]), F32(n["f"][7])
            # world directions whose image c*dx -+ s*dz or c*dz +- s*dx nearly cancels
            for dx, dz in ((s, c), (-s, c), (c, s), (c, -s), (-c, s), (s, -c)):
                o = self.origins(k)
                y = self.rng.uniform(-1.0, 1.0, k).astype(F32)
                d = np.stack([np.full(k, dx, dtype=F32), y, np.full(k, dz, dtype=F32)], axis=1)
                d[k // 2:, 1] = 0.0
                self.add("instance", o, d)


def edge_rays(mrt, s, seed, limit=LIMIT):
    """(RAY_DTYPE rays, class label per ray) for the view `s` (a Synth): every finite class, at most
    `limit` rays (FIXTURE_LIMIT for the reference fixtures, LIMIT otherwise), times and inside flags
    seeded, tmax = +inf."""
    from test_cast_host import entry_rays
    k = limit // 512  # 8 at 4096, 4 at 2048
    g = _Gen(mrt, s, seed)
    g.axis(8 * k)
    g.thin(k)
    g.norm(2 * k)
    g.origin(k)
    g.plane(2 * k)
    g.box(6 * k)
    g.instance(k)
    o, d, label = np.concatenate(g.o), np.concatenate(g.d), np.asarray(g.label)
    n = len(o)
    assert n <= limit - 256, (n, limit)
    rays = np.zeros(n, dtype=mrt.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = o, d, np.inf
    rays["time"] = g.rng.random(n).astype(F32)
    rays["inside"] = g.rng.integers(0, 4, n) == 0
    fill = entry_rays(mrt, s, seed + 1)
    fill = fill[g.rng.permutation(len(fill))[:limit - n]]
    return np.concatenate([rays, fill]), np.concatenate([label, np.full(len(fill), "ordinary")])


def nonfinite_rays(mrt, s, seed):
    """The non-finite class: NaN / +inf / -inf in one origin or one direction component, a zero
    direction, directions of 3e38 (|d|^2 overflows); about 200 rays."""
    g = _Gen(mrt, s, seed)
    for v in (np.nan, np.inf, -np.inf):
        for ax in range(3):
            o = g.origins(4)
            d = g.aimed(o)
            o[:, ax] = v
            g.add("nonfinite", o, d)
            o = g.origins(4)
            d = g.aimed(o)
            d[:, ax] = v
            g.add("nonfinite", o, d)
    o = g.origins(8)
    g.add("nonfinite", o, np.zeros((8, 3), dtype=F32) * np.array([1, -1, 1], dtype=F32))
    o = g.origins(16)
    g.add("nonfinite", o, np.sign(g.aimed(o)) * F32(3e38))
    o = g.origins(8)
    d = g.aimed(o)
    o[:4], d[:4] = np.nan, np.nan
    o[4:], d[4:] = np.inf, -np.inf
    g.add("nonfinite", o, d)
    o, d = np.concatenate(g.o), np.concatenate(g.d)
    rays = np.zeros(len(o), dtype=mrt.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = o, d, np.inf
    rays["time"] = g.rng.random(len(o)).astype(F32)
    return rays, np.full(len(o), "nonfinite")


# ---------------------------------------------------------------- wave arrangements
def arrangements(labels, seed):
    """Index arrays into a batch, one per wave composition: (a) sorted by class, whole 64-ray groups
    of one kind; (b) groups of 63 ordinary rays and one edge ray at lane 0, 31, 32 or 63, a few rays of
    each class; (c) a seeded shuffle."""
    labels = np.asarray(labels)
    rng = np.random.default_rng(seed)
    order = np.argsort(labels, kind="stable")
    ordinary = np.nonzero(labels == "ordinary")[0]
    lone = []
    if len(ordinary) >= 63:
        for c in sorted(set(labels) - {"ordinary"}):
            idx = np.nonzero(labels == c)[0]
            for j, i in enumerate(idx[rng.permutation(len(idx))[:8]]):
                grp = list(ordinary[rng.permutation(len(ordinary))[:63]])
                grp.insert((0, 31, 32, 63)[j % 4], int(i))
                lone += grp
    return dict(sorted=order, lone=np.asarray(lone, dtype=np.int64), shuffled=rng.permutation(len(labels)))
