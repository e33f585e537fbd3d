#!/usr/bin/env python3
"""Digests of the Cornell walk's per-path results on a scene in which every hit identity has its own
record: scene 5 with a distinct lambertian material on each of the five walls, a material of its own
on the box, and the box's rotation negated (sin < 0).  Scene 5 itself cannot tell a wrong hit-table
index from the right one (floor, ceiling and back wall share a material).  tools/fast_path_digest.py's
method: numerics="fast", MRT_RF_PATH_DEBUG, sha256 of the per-path radiance bits and ray counts.
tests/test_cornell_hit_table.py compares with the committed tests/golden/cornell_table_parent.json,
this tool's output on the commit BEFORE the hit table (never regenerated from the tree under test).
  python tools/cornell_table_digest.py [out.json]      (default: stdout)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fast_path_digest as fpd  # noqa: E402

# (name, width, height, spp, depth)
CASES = [
    ("walls_32x32x16", 32, 32, 16, 32),
    ("walls_16x16x4_depth2", 16, 16, 4, 2),
]
# scene 5's view: walls 1, 2 (yz), 4, 5 (xz), 6 (xy); the light 3; translate 7 over rotate_y over the box's list
WALLS = (1, 2, 4, 5, 6)
WALL_RGB = ((0.65, 0.05, 0.05), (0.12, 0.45, 0.15), (0.2, 0.3, 0.7), (0.7, 0.6, 0.2), (0.5, 0.2, 0.6))
BOX_RGB = (0.3, 0.7, 0.7)


def walls_scene(mrt, aspect=1.0):
    from synth_scenes import K_LIST, K_ROTY, Synth
    s = Synth(mrt.select_scene(5, aspect))
    for w, rgb in zip(WALLS, WALL_RGB):
        s.nodes[w]["mat"] = s.lambertian(*rgb)
    (rot,) = s.find(K_ROTY)
    box = int(s.nodes[rot]["a"])
    assert (int(s.nodes[box]["kind"]) & 0xFF) == K_LIST
    faces = s.list_items(box)
    assert len(faces) == 6
    m = s.lambertian(*BOX_RGB)
    for f in faces:
        s.nodes[f]["mat"] = m
    s.nodes[box]["mat"] = m
    s.nodes[rot]["f"][6] = -s.nodes[rot]["f"][6]  # rotate_y's sine
    assert s.nodes[rot]["f"][6] < 0
    s._view = None
    return s


def digest_case(mrt, case):
    name, w, h, spp, depth = case
    r = mrt.Renderer(walls_scene(mrt, w / h), 0)
    rgb, rays, total, _ = fpd.render_paths(mrt, r, w, h, spp, depth, 0)
    ki = r.kernel_info()
    r.close()
    assert int(rays.sum()) == total, (name, int(rays.sum()), total)
    return {"radiance_sha256": hashlib.sha256(np.ascontiguousarray(rgb).view(np.uint32).tobytes()).hexdigest(),
            "rays_sha256": hashlib.sha256(np.ascontiguousarray(rays).tobytes()).hexdigest(),
            "rays": int(total), "kernel_features": int(ki["kernel_features"])}


def main():
    import miniraytracer_amd as mrt
    out = {c[0]: digest_case(mrt, c) for c in CASES}
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
