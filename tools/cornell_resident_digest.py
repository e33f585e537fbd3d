#!/usr/bin/env python3
"""Digests of the Cornell kernels' per-path results on the cases that matter once the walk's scene
words (the room, the box, the sphere, the light's rect, the depth limit) are state of a LAUNCH instead
of being read where they are used: a value taken once per launch must be the right one for every depth
limit, must not survive into the next launch of the same renderer, and must be there for a wave that
never runs a full refill.

  s5_depth_N          scene 5 at 24x24x4 with max_bounces N = 1, 2, 5, 32
  pair_32_2, pair_2_32   two renders in a row on ONE renderer, max_bounces 32 then 2 and 2 then 32:
                      each render's digests, in order (a resident value gone stale between launches)
  paths_N             scene 5 with N = 63, 65, 129 paths at 1 spp: one partial refill, two refills, a
                      launch that crosses a claim boundary
  chunked             one render in several launches (chunk_samples): a launch's first sample is not 0;
                      the image's bits and the ray total (MRT_RF_PATH_DEBUG keeps a render in one launch)
  walls               a material per wall and on the box, the box's rotation negated
                      (tools/cornell_table_digest.py walls_scene)
  sphere_lambertian   the sphere lambertian (tools/cornell_start_digest.py lambsphere_scene)
  glass               the glass-heavy scene (tools/fast_path_digest.py glass_scene)
  offlight            another rect than op 3 as the biased object: DScene::light_once off
  lookalike           the catalogue's b_cornell_lookalike: the Cornell shape on other numbers (its room,
                      like scene 5's, has five faces: the mask's sixth bit is clear)
  lookalike_open      the catalogue's b_cornell_lookalike_open_room: its back wall is moved off the
                      room's box, so the upload finds no room and the interpreter's kernel runs it
  s5_mode1            scene 5, mode 1

tools/fast_path_digest.py's method: numerics="fast", MRT_RF_PATH_DEBUG, sha256 of the per-path
radiance bits and ray counts.  tests/test_cornell_resident.py compares with the committed
tests/golden/cornell_resident_parent.json, this tool's output with the PARENT commit's library (never
regenerated from the tree under test).
  python tools/cornell_resident_digest.py [out.json]      (default: stdout)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cornell_start_digest as csd  # noqa: E402
import cornell_table_digest as ctd  # noqa: E402
import fast_path_digest as fpd  # noqa: E402

V_LIN_INST = 0x2808  # FT_LIN | FT_INST | FT_BIASED, no shape id: the linear-program interpreter

# (name, scene, width, height, spp, renders as (depth, mode) in order, chunk_samples or 0, the kernel)
CASES = [(f"s5_depth_{d}", 5, 24, 24, 4, ((d, 0),), 0, fpd.V_CORNELL) for d in (1, 2, 5, 32)] + [
    ("pair_32_2", 5, 24, 24, 4, ((32, 0), (2, 0)), 0, fpd.V_CORNELL),
    ("pair_2_32", 5, 24, 24, 4, ((2, 0), (32, 0)), 0, fpd.V_CORNELL),
    ("paths_63", 5, 9, 7, 1, ((32, 0),), 0, fpd.V_CORNELL),
    ("paths_65", 5, 13, 5, 1, ((32, 0),), 0, fpd.V_CORNELL),
    ("paths_129", 5, 43, 3, 1, ((32, 0),), 0, fpd.V_CORNELL),
    ("chunked", 5, 24, 24, 16, ((32, 0),), 5, fpd.V_CORNELL),
    ("walls", "walls", 24, 24, 4, ((32, 0),), 0, fpd.V_CORNELL),
    ("sphere_lambertian", "lambsphere", 24, 24, 4, ((32, 0),), 0, fpd.V_CORNELL),
    ("glass", "glass", 16, 16, 4, ((32, 0),), 0, fpd.V_CORNELL),
    ("offlight", "offlight", 24, 24, 4, ((32, 0),), 0, fpd.V_CORNELL),
    ("lookalike", "lookalike", 24, 24, 4, ((32, 0),), 0, fpd.V_CORNELL),
    ("lookalike_open", "lookalike_open", 24, 24, 4, ((32, 0),), 0, V_LIN_INST),
    ("s5_mode1", 5, 24, 24, 4, ((32, 1),), 0, fpd.V_CORNELL),
]


def scene_of(mrt, sid, aspect):
    if sid == "walls":
        return ctd.walls_scene(mrt, aspect)
    if sid == "lambsphere":
        return csd.lambsphere_scene(mrt, aspect)
    if sid in ("lookalike", "lookalike_open"):
        import test_synthetic_scenes as tss
        assert aspect == 1.0  # (the catalogue builds its graphs on scene 5's square camera)
        return tss.lookalike(mrt, closed=sid == "lookalike")
    return fpd.scene_of(mrt, sid, aspect)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest_case(mrt, case):
    name, sid, w, h, spp, renders, chunk, _ = case
    r = mrt.Renderer(scene_of(mrt, sid, w / h), 0)
    out = {"renders": []}
    for depth, mode in renders:
        if chunk:
            img, total = r.render(mrt.render_desc(w, h, spp, depth=depth, mode=mode, numerics="fast", chunk_samples=chunk))
            e = {"image_sha256": _sha(np.ascontiguousarray(img).view(np.uint32))}
        else:
            rgb, rays, total, _ = fpd.render_paths(mrt, r, w, h, spp, depth, mode)
            assert int(rays.sum()) == total, (name, int(rays.sum()), total)
            e = {"radiance_sha256": _sha(np.ascontiguousarray(rgb).view(np.uint32)), "rays_sha256": _sha(rays)}
        e.update({"depth": depth, "mode": mode, "rays": int(total)})
        out["renders"].append(e)
    out["kernel_features"] = int(r.kernel_info()["kernel_features"])
    r.close()
    return out


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
