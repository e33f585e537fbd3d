// mrt_tables.hip -- the scene compiler: a caller's mrt_scene_view -> SceneTables (mrt_tables.h), the
// tables both backends run on (mrt_scene_upload copies them to HBM, mrt_cpu_scene_create keeps them).
//
// Host code only (--offload-host-only; no HIP call, no kernel): the graph checks every device stack
// is sized from, the wide BVH layouts, the linear hit program and its shape.  Its float arithmetic
// (the dielectric quotients, the box.h recognition) is under the exact contract's host flags: no
// contraction, no -mfma.  mrt_internal_scene_tables at the end is the list of its stages.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "mrt_tables.h"

using namespace mrtd;

// Wide nodes renumbered breadth-first over all roots together (level 0 of every tree, then level
// 1, ...), so the first K nodes of the array are the top levels of the scene's BVHs -- what a
// treelet of K nodes holds.  Only the labels change: every walk visits the same nodes.
// limit: only the first `limit` nodes breadth-first, the others after them in their own order
// (pod_bvh's depth-first layout keeps a subtree's nodes together in the cache).
template <typename W>
static void bfs_order(std::vector<W>& wide, std::vector<uint32_t*> roots, uint32_t leaf_bit, uint32_t limit = 0xFFFFFFFFu) {
    const uint32_t n = (uint32_t)wide.size();
    std::vector<uint32_t> nid(n, MRT_NONE), order;
    order.reserve(n);
    for (uint32_t* r : roots)
        if (!(*r & leaf_bit) && *r < n && nid[*r] == MRT_NONE && order.size() < limit) { nid[*r] = (uint32_t)order.size(); order.push_back(*r); }
    for (size_t q = 0; q < order.size() && order.size() < limit; q++) {
        const W& w = wide[order[q]];
        for (uint32_t c : {w.lref, w.rref})
            if (!(c & leaf_bit) && c < n && nid[c] == MRT_NONE && order.size() < limit) { nid[c] = (uint32_t)order.size(); order.push_back(c); }
    }
    for (uint32_t i = 0; i < n; i++)  // the rest (and unreachable nodes) in their own order
        if (nid[i] == MRT_NONE) { nid[i] = (uint32_t)order.size(); order.push_back(i); }
    auto remap = [&](uint32_t c) { return (c & leaf_bit) || c >= n ? c : nid[c]; };
    std::vector<W> out(n);
    for (uint32_t k = 0; k < n; k++) {
        out[k] = wide[order[k]];
        out[k].lref = remap(out[k].lref);
        out[k].rref = remap(out[k].rref);
    }
    wide.swap(out);
    for (uint32_t* r : roots) *r = remap(*r);
}

static bool is_prim_kind(uint32_t k) { return k == MRT_K_SPHERE || k == MRT_K_XY || k == MRT_K_XZ || k == MRT_K_YZ; }

// graph checks on the host: every device stack is sized from them, so none can overflow
static bool needs_uv_tex(const mrt_scene_view* v, uint32_t t, int guard = 0) {
    if (t == MRT_NONE || t >= v->n_textures || guard > 16) return false;
    const mrt_texture& T = v->textures[t];
    if (T.kind == MRT_T_IMAGE) return true;
    if (T.kind == MRT_T_CHECKER) return needs_uv_tex(v, T.a, guard + 1) || needs_uv_tex(v, T.b, guard + 1);
    return false;
}
struct GraphCheck {
    const std::vector<mrt_node>& nodes;
    const mrt_scene_view* v;
    int max_frames = 0, max_rays = 0, max_mesh = 0;
    int bvhw_depth = 0;  // deepest wide-node stack of the converted bvh_node subtrees
    bool ok = true;
    std::string why;
    int mesh_depth(uint32_t ni, int guard) {
        if (guard > 1000 || ni >= v->n_mesh_nodes) return 100000;
        const mrt_mesh_node& m = v->mesh_nodes[ni];
        if (m.count_order & 0xFFFFFFu) return 1;
        return 1 + std::max(mesh_depth(m.left_or_first, guard + 1), mesh_depth(m.left_or_first + 1, guard + 1));
    }
    void walk(uint32_t id, int frames, int rays, bool in_volume, int guard) {
        if (!ok) return;
        if (id >= nodes.size() || guard > 4096) { ok = false; why = "bad node index / cyclic scene graph"; return; }
        const mrt_node& n = nodes[id];
        uint32_t k = n.kind & 0xFF;
        if (is_prim_kind(k)) return;
        if (k == MRT_K_MESH) {
            max_mesh = std::max(max_mesh, mesh_depth(n.a, 0));
            return;
        }
        if (k == MRT_K_BVHW) {
            max_mesh = std::max(max_mesh, bvhw_depth);
            return;
        }
        frames++;
        max_frames = std::max(max_frames, frames);
        switch (k) {
        case MRT_K_LIST:
            for (uint32_t i = 0; i < n.b; i++) walk(v->children[n.a + i], frames, rays, in_volume, guard + 1);
            break;
        case MRT_K_BVH:
            walk(n.a, frames, rays, in_volume, guard + 1);
            walk(n.b, frames, rays, in_volume, guard + 1);
            break;
        case MRT_K_TRANSLATE: case MRT_K_ROTY: case MRT_K_TRROTY:
            max_rays = std::max(max_rays, rays + 1);
            walk(n.a, frames, rays + 1, in_volume, guard + 1);
            break;
        case MRT_K_VOLUME:
            if (in_volume) { ok = false; why = "nested constant_volume"; return; }
            walk(n.a, frames, rays, true, guard + 1);
            break;
        default: ok = false; why = "unknown node kind";
        }
    }
};

// Linear hit program (mrt_lin.h): object_list trees of primitives / meshes with at most one
// instance level.  Returns false (generic kernel) for bvh_node, constant_volume, nested instances.
struct LinCompiler {
    const std::vector<mrt_node>& nodes;
    const mrt_scene_view* v;
    std::vector<LinOp> prog;
    int max_lvl = 0;
    uint32_t inst_pc = MRT_NONE;  // op index of the enclosing instance while its subtree is emitted
    bool in_vsub = false;         // emitting a volume's boundary sub-program (primitives, lists, one instance level)
    bool vsub = false;            // the program has such a volume (FT_VSUB)
    // code = op | kind << 8 | flags << 16 | nesting level << 24 (the level the op is tested at)
    LinOp op_of(uint32_t code, uint32_t id, int lvl) {
        const mrt_node& n = nodes[id];
        LinOp o{};
        o.code = code | ((n.kind & 0xFFu) << 8) | (n.kind & 0xFF0000u) | ((uint32_t)lvl << 24);
        o.node = id;
        o.skip = 0;
        o.mat = n.mat;
        for (int i = 0; i < 12; i++) o.f[i] = n.f[i];
        return o;
    }
    // primitive-like ops (prim, mesh, bvh subtree, volume) also carry the enclosing instance's op
    // index in f[11] (which they do not use) for the resumable interpreter
    LinOp leaf_op(uint32_t code, uint32_t id, int lvl) {
        LinOp o = op_of(code, id, lvl);
        memcpy(&o.f[11], &inst_pc, 4);
        return o;
    }
    bool emit(uint32_t id, int inst_depth, int lvl, int guard) {
        if (id >= nodes.size() || guard > 256 || lvl > 30) return false;
        const mrt_node& n = nodes[id];
        const uint32_t k = n.kind & 0xFFu;
        max_lvl = std::max(max_lvl, lvl);
        switch (k) {
        case MRT_K_SPHERE: case MRT_K_XY: case MRT_K_XZ: case MRT_K_YZ:
            prog.push_back(leaf_op(LOP_PRIM, id, lvl));
            return true;
        case MRT_K_MESH:
            if (in_vsub) return false;
            prog.push_back(leaf_op(LOP_MESH, id, lvl));
            return true;
        case MRT_K_BVHW: {
            if (in_vsub) return false;
            LinOp o = leaf_op(LOP_BVHW, id, lvl);
            o.skip = n.a;  // the subtree's root ref (the op's f[0..5] are its box)
            prog.push_back(o);
            return true;
        }
        case MRT_K_VOLUME: {
            if (n.a >= nodes.size() || in_vsub) return false;
            const uint32_t bk = nodes[n.a].kind & 0xFFu;
            if (is_prim_kind(bk)) {  // a primitive boundary
                prog.push_back(leaf_op(LOP_VOLUME, id, lvl));
                prog.push_back(op_of(LOP_VBOUND, n.a, lvl));
                return true;
            }
            // any other boundary (box.h lists, instances of them: cornell_smoke, scene.cpp:364-369)
            // as a sub-program after the op, walked twice per query by the volume op (lin_sub_t) and
            // skipped by the main walk; outside instances only (its instance is then the only level)
            if (inst_depth > 0) return false;
            const size_t at = prog.size();
            LinOp vo = leaf_op(LOP_VOLUME, id, lvl);
            vo.code |= MRT_F_VSUB << 16;
            prog.push_back(vo);
            in_vsub = true;
            const bool ok = emit(n.a, inst_depth, 0, guard + 1);  // (levels of the sub-program from 0)
            in_vsub = false;
            if (!ok) return false;
            prog[at].skip = (uint32_t)prog.size();
            vsub = true;
            return true;
        }
        case MRT_K_LIST: {
            size_t at = prog.size();
            prog.push_back(op_of(LOP_LIST, id, lvl));
            for (uint32_t i = 0; i < n.b; i++)
                if (!emit(v->children[n.a + i], inst_depth, lvl + 1, guard + 1)) return false;
            prog[at].skip = (uint32_t)prog.size();
            prog.push_back(op_of(LOP_LIST_END, id, lvl));
            return true;
        }
        case MRT_K_TRANSLATE: case MRT_K_ROTY: case MRT_K_TRROTY: {
            if (inst_depth > 0) return false;
            size_t at = prog.size();
            prog.push_back(op_of(LOP_INST, id, lvl));
            const uint32_t outer_pc = inst_pc;
            if (!in_vsub) inst_pc = (uint32_t)at;
            const bool ok = emit(n.a, inst_depth + 1, lvl + 1, guard + 1);
            inst_pc = outer_pc;
            if (!ok) return false;
            prog[at].skip = (uint32_t)prog.size();
            LinOp e = op_of(LOP_INST_END, id, lvl);
            e.skip = (uint32_t)at;  // its instance op
            prog.push_back(e);
            return true;
        }
        default:
            return false;
        }
    }
};

static uint32_t scene_features(const mrt_scene_view* v, const std::vector<mrt_node>& nodes, const std::vector<uint8_t>& absorbed) {
    uint32_t f = 0;
    for (size_t i = 0; i < nodes.size(); i++) {
        const mrt_node& n = nodes[i];
        switch (n.kind & 0xFF) {
        case MRT_K_BVH: if (!absorbed[i]) f |= FT_BVH; break;
        case MRT_K_BVHW: f |= FT_BVHW; break;
        case MRT_K_MESH: f |= FT_MESH; break;
        case MRT_K_VOLUME: f |= FT_VOLUME; break;
        case MRT_K_TRANSLATE: case MRT_K_ROTY: case MRT_K_TRROTY: f |= FT_INST; break;
        case MRT_K_SPHERE: if ((n.kind >> 16) & MRT_F_MOVING) f |= FT_MOVING; break;
        }
        if ((n.kind >> 16) & MRT_F_NEEDUV) f |= FT_UV;
    }
    for (uint32_t i = 0; i < v->n_textures; i++)
        if (v->textures[i].kind != MRT_T_COLOR) f |= FT_TEX;
    for (uint32_t i = 0; i < v->n_materials; i++) {
        if (v->materials[i].kind == MRT_M_METAL) f |= FT_METAL;
        if (v->materials[i].kind == MRT_M_ISOTROPIC) f |= FT_ISO;
    }
    if (v->sky) f |= FT_SKY;
    if (v->biased != MRT_NONE) {
        f |= FT_BIASED;
        const mrt_node& b = nodes[v->biased];
        // any leaf but an xz_rect: spheres, and kinds without a pdf of their own (mrt_shade.h predraw_ok)
        if ((b.kind & 0xFF) != MRT_K_XZ && (b.kind & 0xFF) != MRT_K_LIST) f |= FT_BSPHERE;
        if ((b.kind & 0xFF) == MRT_K_LIST)
            for (uint32_t i = 0; i < b.b; i++)
                if ((nodes[v->children[b.a + i]].kind & 0xFF) != MRT_K_XZ) f |= FT_BSPHERE;
    }
    return f;
}

// Every index a view's records hold, against the array it points into: the table builder below and
// both backends' walks dereference them unchecked.  Returns what is out of range ("" if nothing is);
// runs before anything else reads the arrays and before any HIP call.
static std::string view_range_error(const mrt_scene_view* v) {
    auto at = [](const char* what, uint32_t i) { return std::string(what) + " (record " + std::to_string(i) + ")"; };
    if ((v->n_nodes && !v->nodes) || (v->n_children && !v->children) || (v->n_mesh_nodes && !v->mesh_nodes) ||
        (v->n_tris && (!v->tri_geo || !v->tri_nrm)) || (v->n_materials && !v->materials) || (v->n_textures && !v->textures) ||
        (v->n_texels && !v->texels) || !v->perlin_ranvec || !v->perlin_perm)
        return "null array with a non-zero count";
    if (v->biased != MRT_NONE && v->biased >= v->n_nodes) return "bad biased node";
    for (uint32_t i = 0; i < v->n_nodes; i++) {
        const mrt_node& n = v->nodes[i];
        switch (n.kind & 0xFF) {
        case MRT_K_LIST:
            if ((uint64_t)n.a + n.b > v->n_children) return at("object_list children run beyond n_children", i);
            for (uint32_t c = 0; c < n.b; c++)
                if (v->children[n.a + c] >= v->n_nodes) return at("object_list child index beyond n_nodes", i);
            break;
        case MRT_K_BVH:
            if (n.a >= v->n_nodes || n.b >= v->n_nodes) return at("bvh_node child index beyond n_nodes", i);
            break;
        case MRT_K_MESH:
            if (n.a >= v->n_mesh_nodes) return at("mesh root beyond n_mesh_nodes", i);
            if (n.mat >= v->n_materials) return at("mesh material index beyond n_materials", i);
            break;
        case MRT_K_TRANSLATE: case MRT_K_ROTY:
            if (n.a >= v->n_nodes) return at("instance child index beyond n_nodes", i);
            break;
        case MRT_K_SPHERE: case MRT_K_XY: case MRT_K_XZ: case MRT_K_YZ:
            if (n.mat >= v->n_materials) return at("primitive material index beyond n_materials", i);
            break;
        case MRT_K_VOLUME:
            if (n.a >= v->n_nodes) return at("constant_volume boundary index beyond n_nodes", i);
            if (n.mat >= v->n_materials) return at("constant_volume material index beyond n_materials", i);
            break;
        default: break;  // (an unknown kind is refused where the graph reaches it: GraphCheck)
        }
    }
    for (uint32_t i = 0; i < v->n_mesh_nodes; i++) {
        const mrt_mesh_node& m = v->mesh_nodes[i];
        const uint32_t cnt = m.count_order & 0xFFFFFFu;
        if (cnt == 0 ? (uint64_t)m.left_or_first + 1 >= v->n_mesh_nodes : (uint64_t)m.left_or_first + cnt > v->n_tris)
            return at(cnt == 0 ? "mesh node children beyond n_mesh_nodes" : "mesh leaf triangles beyond n_tris", i);
    }
    for (uint32_t i = 0; i < v->n_materials; i++) {
        const mrt_material& m = v->materials[i];
        // (a dielectric has no texture: material.h:121)
        if (m.kind != MRT_M_DIELECTRIC && m.tex >= v->n_textures) return at("material texture index beyond n_textures", i);
    }
    for (uint32_t i = 0; i < v->n_textures; i++) {
        const mrt_texture& t = v->textures[i];
        if (t.kind == MRT_T_CHECKER && (t.a >= v->n_textures || t.b >= v->n_textures))
            return at("checker texture child index beyond n_textures", i);
        if (t.kind == MRT_T_IMAGE && (t.b == 0 || t.c == 0 || (uint64_t)t.b * t.c > (1ull << 40) ||
                                      (uint64_t)t.a + (uint64_t)t.b * t.c * 3u > v->n_texels))
            return at("image texture texels beyond n_texels", i);
    }
    return "";
}

// ---- The stages of mrt_internal_scene_tables, in the order it runs them.  Each takes what it reads
// and the tables it makes; `nodes` is the device node table in the making (a copy of the view's).
// a test hook of the builder, read on every call (the tests set them per test)
static bool hook_set(const char* name) {
    const char* e = getenv(name);
    return e && *e && *e != '0';
}

// node flags: NEEDUV on primitives whose material samples an image texture; SLOWDIV on rect planes
// outside {0} U [2^-77, 2^60], which keep the IEEE division in rect tests (mrt_device.h ray_nice)
static void flag_nodes(const mrt_scene_view* v, std::vector<mrt_node>& nodes) {
    for (mrt_node& n : nodes)
        if (is_prim_kind(n.kind & 0xFF) && n.mat < v->n_materials && needs_uv_tex(v, v->materials[n.mat].tex)) n.kind |= MRT_F_NEEDUV << 16;
    for (mrt_node& n : nodes) {
        const uint32_t k = n.kind & 0xFF;
        if (k != MRT_K_XY && k != MRT_K_XZ && k != MRT_K_YZ) continue;
        const float c = std::fabs(n.f[4]);
        if (!(c == 0.0f || (c >= 0x1p-77f && c <= 0x1p60f))) n.kind |= MRT_F_SLOWDIV << 16;
    }
}

// box.h:12-20 recognised: an object_list of exactly six outward-facing rects over one box
// (xy at max z / min z, xz at max y / min y, yz at max x / min x, bounds spanning the box, one
// material, no uv, no slow divisions).  Flag MRT_F_BOX6, planes in f[6..11] (min xyz, max xyz):
// the tolerance contract tests such a list as one slab test (mrt_sig.h box6_hit).
static void recognise_box_lists(const mrt_scene_view* v, std::vector<mrt_node>& nodes) {
    for (size_t i = 0; i < nodes.size(); i++) {
        mrt_node& n = nodes[i];
        if ((n.kind & 0xFF) != MRT_K_LIST || n.b != 6 || n.a + 6 > v->n_children) continue;
        const mrt_node* c[6];
        bool ok = true;
        for (int j = 0; j < 6 && ok; j++) {
            const uint32_t ci = v->children[n.a + j];
            ok = ci < nodes.size();
            if (ok) c[j] = &nodes[ci];
        }
        if (!ok) continue;
        static const uint32_t kinds[6] = {MRT_K_XY, MRT_K_XY, MRT_K_XZ, MRT_K_XZ, MRT_K_YZ, MRT_K_YZ};
        for (int j = 0; j < 6 && ok; j++)
            ok = (c[j]->kind & 0xFF) == kinds[j] && c[j]->f[5] == ((j & 1) ? -1.0f : 1.0f) && c[j]->mat == c[0]->mat &&
                 !((c[j]->kind >> 16) & (MRT_F_NEEDUV | MRT_F_SLOWDIV));
        if (!ok) continue;
        const float xmin = c[5]->f[4], xmax = c[4]->f[4], ymin = c[3]->f[4], ymax = c[2]->f[4], zmin = c[1]->f[4], zmax = c[0]->f[4];
        auto span = [&](const mrt_node* r, float a0, float a1, float b0, float b1) {
            return r->f[0] == a0 && r->f[1] == a1 && r->f[2] == b0 && r->f[3] == b1;
        };
        ok = xmin < xmax && ymin < ymax && zmin < zmax && span(c[0], xmin, xmax, ymin, ymax) && span(c[1], xmin, xmax, ymin, ymax) &&
             span(c[2], xmin, xmax, zmin, zmax) && span(c[3], xmin, xmax, zmin, zmax) && span(c[4], ymin, ymax, zmin, zmax) &&
             span(c[5], ymin, ymax, zmin, zmax);
        if (!ok) continue;
        n.kind |= MRT_F_BOX6 << 16;
        n.mat = c[0]->mat;  // (an object_list has no material of its own)
        n.f[6] = xmin; n.f[7] = ymin; n.f[8] = zmin;
        n.f[9] = xmax; n.f[10] = ymax; n.f[11] = zmax;
    }
}

// translate(rotate_y(x)) fused into one instance node (MRT_K_TRROTY)
static void fuse_translate_rotate(std::vector<mrt_node>& nodes) {
    for (mrt_node& n : nodes) {
        if ((n.kind & 0xFF) != MRT_K_TRANSLATE || n.a >= nodes.size()) continue;
        const mrt_node& c = nodes[n.a];
        if ((c.kind & 0xFF) != MRT_K_ROTY) continue;
        mrt_node f{};
        f.kind = MRT_K_TRROTY | (c.kind & (MRT_F_HASBOX << 16));
        f.a = c.a;
        f.b = MRT_NONE;
        f.mat = MRT_NONE;
        for (int i = 0; i < 8; i++) f.f[i] = c.f[i];  // bbox, sin, cos
        f.f[8] = n.f[0]; f.f[9] = n.f[1]; f.f[10] = n.f[2];
        n = f;
    }
}

// pod_bvh -> wide nodes (both child boxes inline); MESH nodes get b = root ref.  False: a mesh BVH
// outside the device encoding.
static bool mesh_wide(const mrt_scene_view* v, std::vector<mrt_node>& nodes, std::vector<MeshWide>& wide) {
    std::vector<uint32_t> wide_of(v->n_mesh_nodes, MRT_NONE);
    for (uint32_t i = 0; i < v->n_mesh_nodes; i++)
        if ((v->mesh_nodes[i].count_order & 0xFFFFFFu) == 0) {
            wide_of[i] = (uint32_t)wide.size();
            wide.push_back(MeshWide{});
        }
    bool ok = wide.size() < MESH_LEAF;
    auto ref_of = [&](uint32_t i) -> uint32_t {
        if (i >= v->n_mesh_nodes) { ok = false; return 0; }
        const mrt_mesh_node& m = v->mesh_nodes[i];
        const uint32_t cnt = m.count_order & 0xFFFFFFu;
        if (cnt == 0) return wide_of[i];
        if (cnt > 0x7Fu || m.left_or_first > 0xFFFFFFu) ok = false;
        if ((MESH_LEAF | (cnt << 24) | m.left_or_first) >= kMeshEmpty) ok = false;  // (the walk's marks)
        return MESH_LEAF | (cnt << 24) | m.left_or_first;
    };
    for (uint32_t i = 0; i < v->n_mesh_nodes && ok; i++) {
        if (wide_of[i] == MRT_NONE) continue;
        const mrt_mesh_node& m = v->mesh_nodes[i];
        const uint32_t l = m.left_or_first;
        if (l + 1 >= v->n_mesh_nodes) { ok = false; break; }
        MeshWide& W = wide[wide_of[i]];
        const mrt_mesh_node &L = v->mesh_nodes[l], &R = v->mesh_nodes[l + 1];
        for (int k = 0; k < 3; k++) {
            W.lmin[k] = L.bmin[k]; W.lmax[k] = L.bmax[k];
            W.rmin[k] = R.bmin[k]; W.rmax[k] = R.bmax[k];
        }
        W.lref = ref_of(l);
        W.rref = ref_of(l + 1);
        W.order = m.count_order >> 24;
    }
    for (mrt_node& n : nodes)
        if ((n.kind & 0xFF) == MRT_K_MESH) n.b = ref_of(n.a);
    if (!ok) return false;
    // the top 63 nodes first, breadth-first: the hot top levels share cache lines
    std::vector<uint32_t*> mroots;
    for (mrt_node& n : nodes)
        if ((n.kind & 0xFF) == MRT_K_MESH) mroots.push_back(&n.b);
    bfs_order(wide, mroots, MESH_LEAF, 63u);
    return true;
}

// bvh_node subtrees whose leaves are primitives / object_lists of primitives (and of boxes of
// primitives) -> wide nodes; the subtree root becomes an MRT_K_BVHW node (a = root ref)
struct BvhSubtrees {
    std::vector<BvhWide> bwide;     // breadth-first over all roots: treelet kernels cache the first nodes, the top levels
    std::vector<mrt_node> bprims;   // leaf primitive runs of the wide subtrees
    std::vector<uint8_t> absorbed;  // per node: a bvh_node now inside a wide subtree
    int depth = 0;                  // deepest wide-node stack (one word per level for the binary walk)
};
// False: a leaf outside the device encoding.  MRT_NO_BVHW (test hook) keeps the generic bvh_node walk.
static bool bvh_wide(const mrt_scene_view* v, std::vector<mrt_node>& nodes, BvhSubtrees& B) {
    std::vector<BvhWide>& bwide = B.bwide;
    std::vector<mrt_node>& bprims = B.bprims;
    B.absorbed.assign(nodes.size(), 0);
    const size_t nn = nodes.size();
    auto kind_of = [&](uint32_t i) { return nodes[i].kind & 0xFFu; };
    auto is_leaf_prim = [&](uint32_t i) { return is_prim_kind(kind_of(i)); };
    auto leaf_ok = [&](uint32_t i) {
        if (is_leaf_prim(i)) return true;
        if (kind_of(i) != MRT_K_LIST) return false;
        const mrt_node& l = nodes[i];
        for (uint32_t c = 0; c < l.b; c++) {
            const uint32_t ci = v->children[l.a + c];
            if (ci >= nn) return false;
            if (is_leaf_prim(ci)) continue;
            if (kind_of(ci) != MRT_K_LIST) return false;
            const mrt_node& g = nodes[ci];
            for (uint32_t j = 0; j < g.b; j++) {
                const uint32_t gi = v->children[g.a + j];
                if (gi >= nn || !is_leaf_prim(gi)) return false;
            }
        }
        return true;
    };
    std::vector<uint8_t> under_bvh(nn, 0);
    for (size_t i = 0; i < nn; i++)
        if (kind_of((uint32_t)i) == MRT_K_BVH) {
            if (nodes[i].a < nn) under_bvh[nodes[i].a] = 1;
            if (nodes[i].b < nn) under_bvh[nodes[i].b] = 1;
        }
    // does the subtree at i qualify (bvh_node inner nodes, qualifying leaves)?
    std::function<bool(uint32_t, int)> ok = [&](uint32_t i, int guard) -> bool {
        if (i >= nn || guard > 64) return false;
        if (kind_of(i) != MRT_K_BVH) return leaf_ok(i);
        return ok(nodes[i].a, guard + 1) && ok(nodes[i].b, guard + 1);
    };
    // a leaf's primitives as one contiguous run of node records (bprims): a primitive leaf is a
    // run of one; an object_list leaf is its children in order, a nested object_list as a LIST
    // record (its box, b = the count of its own children that follow) before its children.  The
    // walk then fetches a leaf's records at independent addresses instead of through the
    // children[] -> node chain (two dependent loads per primitive).
    bool leaves_ok = true;
    auto emit_leaf = [&](uint32_t i) -> uint32_t {
        const uint32_t first = (uint32_t)bprims.size();
        if (is_leaf_prim(i)) {
            bprims.push_back(nodes[i]);
        } else {
            const mrt_node& l = nodes[i];
            for (uint32_t c = 0; c < l.b; c++) {
                const uint32_t ci = v->children[l.a + c];
                if (is_leaf_prim(ci)) { bprims.push_back(nodes[ci]); continue; }
                const mrt_node& g = nodes[ci];
                bprims.push_back(g);
                for (uint32_t j = 0; j < g.b; j++) bprims.push_back(nodes[v->children[g.a + j]]);
            }
        }
        const uint32_t cnt = (uint32_t)bprims.size() - first;
        if (cnt > BVHW_MAX_RUN || first > BVHW_FIRST_MASK) leaves_ok = false;
        if ((BVHW_LEAF | (cnt << 24) | (first & BVHW_FIRST_MASK)) == kBvhwEmpty) leaves_ok = false;  // (the walk's empty-stack mark)
        return BVHW_LEAF | (cnt << 24) | (first & BVHW_FIRST_MASK);
    };
    std::function<uint32_t(uint32_t, int)> build = [&](uint32_t i, int depth) -> uint32_t {
        B.depth = std::max(B.depth, depth);
        if (kind_of(i) != MRT_K_BVH) return emit_leaf(i);
        B.absorbed[i] = 1;
        const uint32_t w = (uint32_t)bwide.size();
        bwide.push_back(BvhWide{});
        const mrt_node& b = nodes[i];
        const uint32_t lc = b.a, rc = b.b;
        const uint32_t lref = build(lc, depth + 1), rref = build(rc, depth + 1);
        BvhWide& W = bwide[w];
        W.lref = lref;
        W.rref = rref;
        W.order = (b.kind >> 8) & 0xFFu;
        W.flags = 0;
        const mrt_node &L = nodes[lc], &R = nodes[rc];
        auto has_box = [&](const mrt_node& c) {
            const uint32_t k = c.kind & 0xFFu;
            return k == MRT_K_BVH || (k == MRT_K_LIST && ((c.kind >> 16) & MRT_F_HASBOX));
        };
        if (has_box(L)) { W.flags |= 1u; for (int k = 0; k < 3; k++) { W.lmin[k] = L.f[k]; W.lmax[k] = L.f[3 + k]; } }
        if (has_box(R)) { W.flags |= 2u; for (int k = 0; k < 3; k++) { W.rmin[k] = R.f[k]; W.rmax[k] = R.f[3 + k]; } }
        return w;
    };
    if (!hook_set("MRT_NO_BVHW"))
        for (size_t i = 0; i < nn; i++)
            if (kind_of((uint32_t)i) == MRT_K_BVH && !under_bvh[i] && ok((uint32_t)i, 0) && bwide.size() < BVHW_LEAF / 2) {
                const uint32_t root = build((uint32_t)i, 1);
                mrt_node& r = nodes[i];
                r.kind = (r.kind & ~0xFFu) | MRT_K_BVHW;
                r.a = root;
            }
    if (!leaves_ok) return false;
    std::vector<uint32_t*> broots;
    for (mrt_node& n : nodes)
        if ((n.kind & 0xFF) == MRT_K_BVHW) broots.push_back(&n.a);
    bfs_order(bwide, broots, BVHW_LEAF);
    return true;
}

// the stack depths of the scene graph (GraphCheck) and the shape of scene.biased_objects; what is
// wrong with the graph ("" if nothing is)
static std::string check_graph(const mrt_scene_view* v, const std::vector<mrt_node>& nodes, int bvhw_depth, SceneTables* T) {
    GraphCheck gc{nodes, v};
    gc.bvhw_depth = bvhw_depth;
    gc.walk(v->root, 0, 0, false, 0);
    if (!gc.ok) return gc.why;
    if (v->biased != MRT_NONE) {
        if (v->biased >= nodes.size()) return "bad biased node";
        const mrt_node& b = nodes[v->biased];
        if ((b.kind & 0xFF) == MRT_K_LIST)
            for (uint32_t i = 0; i < b.b; i++)
                if ((nodes[v->children[b.a + i]].kind & 0xFF) == MRT_K_LIST) return "nested biased object_list";
    }
    T->max_frames = gc.max_frames;
    T->max_rays = gc.max_rays;
    T->max_mesh = gc.max_mesh;
    return "";
}

// the material table: mrt_material plus the inline constant colour and the dielectric quotients
static std::vector<DMat> material_table(const mrt_scene_view* v) {
    std::vector<DMat> dmats(v->n_materials);
    for (uint32_t i = 0; i < v->n_materials; i++) {
        const mrt_material& m = v->materials[i];
        DMat& d = dmats[i];
        d.kind = m.kind;
        d.tex = m.tex;
        d.p = m.p;
        d.flags = 0;
        if (m.tex < v->n_textures && v->textures[m.tex].kind == MRT_T_COLOR) {
            d.flags = DMAT_COLOR;
            for (int k = 0; k < 4; k++) d.col[k] = v->textures[m.tex].f[k];
        }
        if (m.kind == MRT_M_DIELECTRIC) {  // dielectric::scatter's per-material quotients (material.h:121-175)
            const float ref = m.p;
            d.col[0] = 1.0f / ref;
            float r0 = (1 - ref) / (1 + ref);
            d.col[1] = r0 * r0;
        }
    }
    return dmats;
}

// scene.biased_objects flattened: an object_list's children, or the object itself (bleaf, never
// empty: one zero record when the scene has none), with blist, nbleaf and blazy
static void biased_leaves(const mrt_scene_view* v, const std::vector<mrt_node>& nodes, SceneTables* T) {
    std::vector<mrt_node>& bleaf = T->bleaf;
    if (v->biased != MRT_NONE) {
        const mrt_node& b = nodes[v->biased];
        if ((b.kind & 0xFF) == MRT_K_LIST) {
            T->blist = 1;
            for (uint32_t i = 0; i < b.b; i++) bleaf.push_back(nodes[v->children[b.a + i]]);
        } else {
            bleaf.push_back(b);
        }
    }
    for (const mrt_node& l : bleaf)
        if ((l.kind & 0xFF) != MRT_K_XZ && (l.kind & 0xFF) != MRT_K_SPHERE) T->blazy = 1;
    if (bleaf.empty()) bleaf.push_back(mrt_node{});
    T->nbleaf = T->blist ? nodes[v->biased].b : 1u;
}

// Cornell shape: the hit table of the tolerance contract's walk (mrt_sig.h cornell_fast_hit; the
// entry layout is described there) -- per hit identity what the walk's per-lane selects and its
// record code computed for every ray, from the same program words with the same expressions:
//   room face 2 a + side: plane hi / lo [a] and material m[2 a + side] of the END op
//     (cornell_room_fill), normal sign side ? -1 : 1;
//   the light: op 3's plane f[4], side f[5] and material;
//   box face of axis a, the ray going up it or not: normal sign -1 / 1, the face's plane in the box
//     frame lo / hi [a] (op 8's f[6..11]), the normal rotated back by rotate_y's (s, c) (op 7's
//     f[6], f[7]) as unrotate_rec does -- every product has a factor 0 or +-1, so it is exact, and a
//     contracted multiply-add gives the same bits (a denormal sine or cosine aside, which the
//     kernel's build flushes to zero);
//   the sphere: op 17's material (its normal is the ray's own).
static void cornell_hit_fill(const std::vector<LinOp>& prog, const std::vector<DMat>& dmats, std::vector<uint32_t>* out) {
    out->assign((size_t)kHitCount * kHitWords, 0u);
    auto put = [&](uint32_t id, const float n[3], float k, uint32_t code, uint32_t mat) {
        uint32_t* e = out->data() + (size_t)id * kHitWords;
        const DMat m = mat < dmats.size() ? dmats[mat] : DMat{};  // (a face the room lacks: never hit)
        const float f[12] = {n[0], n[1], n[2], k, 0.0f, 0.0f, m.p, 0.0f, m.col[0], m.col[1], m.col[2], m.col[3]};
        memcpy(e, f, sizeof f);
        e[4] = code;
        e[5] = m.kind;
        e[7] = m.flags;
    };
    auto one_hot = [](uint32_t a, float ns, float n[3]) {
        n[0] = a == 0u ? ns : 0.0f;
        n[1] = a == 1u ? ns : 0.0f;
        n[2] = a == 2u ? ns : 0.0f;
    };
    const LinOp& e = prog[kSigs[SIG_CORNELL].n - 1];
    for (uint32_t a = 0; a < 3; a++)
        for (uint32_t side = 0; side < 2; side++) {
            float n[3];
            one_hot(a, side ? -1.0f : 1.0f, n);
            uint32_t mat;
            memcpy(&mat, &e.f[6 + a * 2 + side], 4);
            put(kHitRoom + a * 2 + side, n, side ? e.f[3 + a] : e.f[a], 1u + a, mat);
        }
    {
        const LinOp& l = prog[3];
        float n[3];
        one_hot(1u, l.f[5], n);
        put(kHitLight, n, l.f[4], 2u, l.mat);
    }
    const LinOp &io = prog[7], &bo = prog[8];
    const float s = io.f[6], c = io.f[7];
    for (uint32_t a = 0; a < 3; a++)
        for (uint32_t up = 0; up < 2; up++) {
            const float ns = up ? -1.0f : 1.0f;
            float l[3];
            one_hot(a, ns, l);
            const float lx = l[0], ly = l[1], lz = l[2];
            const float n[3] = {c * lx + s * lz, ly, c * lz - s * lx};
            put(kHitBox + 2 * a + up, n, ns < 0.0f ? bo.f[6 + a] : bo.f[9 + a], 4u + a, bo.mat);
        }
    const float none[3] = {0.0f, 0.0f, 0.0f};
    put(kHitSphere, none, 0.0f, 7u, prog[17].mat);
}

// The linear hit program (LinCompiler; empty + LOP_END when the graph has none or MRT_FORCE_GENERIC
// is set) and what follows from it: FT_LIN / FT_VSUB and the shape id (not under MRT_NO_SIG) into
// T->features, light_once (reads T->bleaf), the tolerance contract's rewrite.
static void linear_program(const mrt_scene_view* v, const std::vector<mrt_node>& nodes, SceneTables* T) {
    LinCompiler lc{nodes, v, {}};
    const bool lin = !hook_set("MRT_FORCE_GENERIC") && lc.emit(v->root, 0, 0, 0);
    if (!lin) lc.prog.clear();
    T->prog_ops = (uint32_t)lc.prog.size();
    lc.prog.push_back(LinOp{});  // LOP_END
    if (lin) {
        T->features |= FT_LIN;
        if (lc.vsub) T->features |= FT_VSUB;
        cornell_room_fill(lc.prog.data(), (uint32_t)lc.prog.size());  // (Cornell shape: the room into the END op)
        if (!hook_set("MRT_NO_SIG")) T->features |= MRT_SIG_BITS(lin_sig_of(lc.prog.data(), (uint32_t)lc.prog.size()));
        // the Cornell walk tests op 3 (the light) once per ray; the same test serves xz_rect::pdf_value where
        // the biased list is that one rect: same bounds, plane and side, bit for bit
        T->light_once = (MRT_SIG_OF(T->features) == SIG_CORNELL && v->biased != MRT_NONE && T->bleaf.size() == 1 &&
                         (T->bleaf[0].kind & 0xFF) == MRT_K_XZ && memcmp(T->bleaf[0].f, lc.prog[3].f, 6 * sizeof(float)) == 0)
                            ? 1u : 0u;
        if (MRT_SIG_OF(T->features) == SIG_CORNELL) cornell_hit_fill(lc.prog, T->dmats, &T->cornell_hits);
        T->prog_fast = lin_rewrite_fast(lc.prog);
    }
    T->prog.swap(lc.prog);
}

// The scene's device tables (mrt_tables.h), built on the host from the caller's view into a fresh
// SceneTables; both backends run on them.
mrt_status mrt_internal_scene_tables(const mrt_scene_view* v, SceneTables* T) {
    auto refuse = [](const std::string& why) { return mrt_internal_fail(MRT_ERR_INVALID, why.c_str()); };
    if (!v || !T || v->root >= v->n_nodes) return refuse("mrt_scene_upload: bad view");
    const std::string bad = view_range_error(v);
    if (!bad.empty()) return refuse("mrt_scene_upload: " + bad);
    std::vector<mrt_node> nodes(v->nodes, v->nodes + v->n_nodes);
    flag_nodes(v, nodes);
    recognise_box_lists(v, nodes);
    fuse_translate_rotate(nodes);
    if (!mesh_wide(v, nodes, T->wide)) return refuse("mesh BVH outside the device encoding (leaf > 127 triangles or > 2^24 triangles)");
    BvhSubtrees B;
    if (!bvh_wide(v, nodes, B)) return refuse("bvh_node leaf outside the device encoding (> 127 primitives or > 2^24 leaf records)");
    const std::string why = check_graph(v, nodes, B.depth, T);
    if (!why.empty()) return refuse(why);
    T->dmats = material_table(v);
    biased_leaves(v, nodes, T);
    T->features = scene_features(v, nodes, B.absorbed);
    linear_program(v, nodes, T);
    T->nodes.swap(nodes);
    T->bwide.swap(B.bwide);
    T->bprims.swap(B.bprims);
    return MRT_OK;
}

// Test hook (tests/test_host.py): the scene's linear hit program as compiled, or its
// tolerance-contract rewrite (mrt_sig.h lin_rewrite_fast) -- per op its code word and skip.
extern "C" int mrt_debug_lin_program(const mrt_scene_view* v, int rewritten, uint32_t* codes, uint32_t* skips, uint32_t cap,
                                     uint32_t* n) {
    SceneTables T;
    if (mrt_internal_scene_tables(v, &T) != MRT_OK) return 1;
    const std::vector<LinOp>& p = rewritten ? T.prog_fast : T.prog;
    *n = (uint32_t)p.size();
    for (uint32_t i = 0; i < p.size() && i < cap; i++) {
        codes[i] = p[i].code;
        skips[i] = p[i].skip;
    }
    return 0;
}

// Test hook (tests/test_cornell_hit_table.py): the Cornell walk's hit table as built for the view,
// *n its words (0: the view has no Cornell shape), the first min(cap, *n) copied out.
extern "C" int mrt_debug_cornell_hits(const mrt_scene_view* v, uint32_t* words, uint32_t cap, uint32_t* n) {
    SceneTables T;
    if (mrt_internal_scene_tables(v, &T) != MRT_OK) return 1;
    *n = (uint32_t)T.cornell_hits.size();
    memcpy(words, T.cornell_hits.data(), std::min<size_t>(cap, T.cornell_hits.size()) * 4);
    return 0;
}

// Test hook (tests/test_cornell_light_gpu.py): the light's quad of a Cornell-shape view -- the extents and
// area a Cornell walk kernel's waves compute once per launch from op 3's words (mrt_sig.h
// cornell_light_quad, the same function, here in the host's arithmetic: no contraction), and op 3's four
// bounds as the program holds them.  Returns 1 where the view is refused, 2 where it has another shape.
extern "C" int mrt_debug_cornell_light_quad(const mrt_scene_view* v, float quad[4], float bounds[4]) {
    SceneTables T;
    if (mrt_internal_scene_tables(v, &T) != MRT_OK) return 1;
    if (MRT_SIG_OF(T.features) != SIG_CORNELL) return 2;
    const LinOp& l = T.prog[3];
    const LightQuad q = cornell_light_quad(l.f[0], l.f[1], l.f[2], l.f[3]);
    const float w[4] = {q.ex, q.ez, q.area, 0.0f};
    memcpy(quad, w, sizeof w);
    memcpy(bounds, l.f, 4 * sizeof(float));
    return 0;
}

// Test hook (tests/test_tables_digest.py, tools/tables_digest.py): the tables as 17 words -- FNV-1a 64
// over the length and bytes of nodes, wide, bwide, bprims, dmats, bleaf, prog, prog_fast (their
// records have no padding), then blist, nbleaf, blazy, light_once, prog_ops, features, max_frames,
// max_rays, max_mesh.
static uint64_t fnv1a64(const void* p, size_t n, uint64_t h) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t*)p)[i]) * 0x100000001b3ull;
    return h;
}
template <typename V>
static uint64_t table_hash(const V& t) {
    const uint64_t n = t.size();
    return fnv1a64(t.data(), n * sizeof(t[0]), fnv1a64(&n, 8, 0xcbf29ce484222325ull));
}
void mrt_internal_tables_digest(const SceneTables& T, uint64_t d[MRT_TABLES_DIGEST_WORDS]) {
    const uint64_t w[MRT_TABLES_DIGEST_WORDS] = {table_hash(T.nodes), table_hash(T.wide), table_hash(T.bwide), table_hash(T.bprims),
                                                 table_hash(T.dmats), table_hash(T.bleaf), table_hash(T.prog), table_hash(T.prog_fast),
                                                 T.blist, T.nbleaf, T.blazy, T.light_once, T.prog_ops, T.features,
                                                 (uint32_t)T.max_frames, (uint32_t)T.max_rays, (uint32_t)T.max_mesh};
    memcpy(d, w, sizeof w);
}
// 0 and the first min(cap, 17) words, or the builder's status (mrt_last_error says why)
extern "C" int mrt_debug_tables_digest(const mrt_scene_view* v, uint64_t* out, uint32_t cap) {
    SceneTables T;
    const mrt_status st = mrt_internal_scene_tables(v, &T);
    if (st != MRT_OK) return (int)st;
    uint64_t d[MRT_TABLES_DIGEST_WORDS];
    mrt_internal_tables_digest(T, d);
    memcpy(out, d, std::min<size_t>(cap, MRT_TABLES_DIGEST_WORDS) * 8);
    return 0;
}
