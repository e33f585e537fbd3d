/* mrt_temporal.h -- temporal reprojection: one pixel of the accumulated ("history") frame, written
 * once for the host (mrt_reproject) and the device kernel (mrt_reproject_kernel) so both produce the
 * same bits: IEEE add / mul / div / sqrt and floorf only, without contraction (-ffp-contract=off).
 *
 * Frames are row-major, one float4 per pixel, row 0 at the bottom (like G_linearBackBuffer):
 *   c       the current frame's colour (xyz; w is not read)
 *   normal  (n.xyz, coverage), albedo (a.xyz, depth): the current frame's first-hit feature buffers
 *           (mrt_render_aux); h, normal', albedo': the previous history frame and the feature buffers
 *           it was made with (primes mark the previous frame and the previous camera throughout)
 *   h       (accumulated rgb, N) with N the history length; the output has the same form
 * "No history" below means out = (c.xyz, 1).  A NULL h (the first frame) is no history everywhere.
 *
 * Per-launch constants (mrt_reproject_setup_make, computed once on the host for both sides), with
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z:
 *   fW = (float)W, fH = (float)H
 *   d0'    = llcorner' - origin'
 *   focus' = dot(origin' - llcorner', w')             (the focus distance: the image plane's depth)
 *   hh'    = dot(horz', horz'), vv' = dot(vert', vert')
 *   albedo_tol2 = albedo_tol * albedo_tol
 *
 * Pixel p = (x, y):
 *  1. Current-pixel check.  No history unless normal.w == 1 (every sample hit a surface: partial
 *     coverage dilutes the mean depth), albedo.w > 0 and lp = dot(n, n) > 0.
 *  2. World point, by the pinhole ray through the pixel centre:
 *       s = ((float)x + 0.5) / fW, t = ((float)y + 0.5) / fH
 *       d = ((llcorner + s horz) + t vert) - origin,   d^ = d / sqrt(dot(d, d))
 *       P = origin + depth d^                           (depth = albedo.w)
 *  3. Projection into the previous camera:
 *       e  = P - origin',  zc = -dot(e, w');  no history unless zc > 0 (behind the camera)
 *       q  = e (focus' / zc) - d0'
 *       fx = (dot(q, horz') / hh') fW - 0.5,  fy = (dot(q, vert') / vv') fH - 0.5
 *     Each of fx, fy is snapped to r = floorf(f + 0.5) when |f - r| <= 1/32, so a still camera
 *     reads exactly its own pixel.  No history unless -1 < fx < fW and -1 < fy < fH.
 *  4. Bilinear taps: x0 = floorf(fx), ax = fx - x0 (y alike); in this order
 *       (x0, y0) (1-ax)(1-ay);  (x0+1, y0) ax (1-ay);  (x0, y0+1) (1-ax) ay;  (x0+1, y0+1) ax ay
 *     A tap q with weight w counts only when all of these hold, tested in this order:
 *       w > 0;  q inside the image;  normal'_q.w == 1;  lq = dot(n'_q, n'_q) > 0 and
 *       dot(n / sqrt(lp), n'_q / sqrt(lq)) >= normal_min;
 *       |z'_q - |e|| <= depth_tol |e|   (|e| = sqrt(dot(e, e)): the point's distance from the
 *                                        previous camera, what z'_q = albedo'_q.w measures);
 *       dot(a - a'_q, a - a'_q) <= albedo_tol2   (the albedo of an emitter is its radiance, so the
 *                                        light never bleeds into the ceiling beside it)
 *     and then adds  sw += w,  s += w h_q  (all four channels, each product rounded, then the sum).
 *  5. Blend.  No history unless sw >= min_weight.  Otherwise
 *       hist = s / sw (four channels),  N' = min(hist.w + 1, max_history),  r = 1 / N'
 *       out.xyz = hist.xyz + (c.xyz - hist.xyz) r,  out.w = N'
 *
 * Every comparison is written so that a NaN fails it: non-finite inputs end as "no history".
 *
 * Approximations: the lens is a pinhole at `origin` (history under depth of field is out of scope);
 * the cameras' time0 / time1 are ignored (moving spheres rely on the depth, normal and albedo tests:
 * there are no per-object motion vectors); the depth is the mean hit distance of the feature buffers.
 */
#ifndef MRT_TEMPORAL_H
#define MRT_TEMPORAL_H
#include "mrt_denoise.h" /* MRT_HD, mrt_f4 */
#include "mrt_scene.h"   /* mrt_camera */

typedef struct mrt_reproject_setup {
    unsigned int width, height;
    float fw, fh;
    float d0[3];   /* llcorner' - origin' */
    float focus;   /* dot(origin' - llcorner', w') */
    float hh, vv;  /* dot(horz', horz'), dot(vert', vert') */
    float max_history, normal_min, depth_tol, albedo_tol2, min_weight;
} mrt_reproject_setup;

MRT_HD float mrt_tp_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

MRT_HD void mrt_reproject_setup_make(unsigned int width, unsigned int height, const mrt_camera* prev, float max_history, float normal_min,
                                     float depth_tol, float albedo_tol, float min_weight, mrt_reproject_setup* rs) {
    rs->width = width;
    rs->height = height;
    rs->fw = (float)width;
    rs->fh = (float)height;
    rs->d0[0] = rs->d0[1] = rs->d0[2] = 0.0f;
    rs->focus = rs->hh = rs->vv = 0.0f;
    if (prev) {
        for (int k = 0; k < 3; k++) rs->d0[k] = prev->llcorner[k] - prev->origin[k];
        rs->focus = mrt_tp_dot(prev->origin[0] - prev->llcorner[0], prev->origin[1] - prev->llcorner[1], prev->origin[2] - prev->llcorner[2],
                               prev->w[0], prev->w[1], prev->w[2]);
        rs->hh = mrt_tp_dot(prev->horz[0], prev->horz[1], prev->horz[2], prev->horz[0], prev->horz[1], prev->horz[2]);
        rs->vv = mrt_tp_dot(prev->vert[0], prev->vert[1], prev->vert[2], prev->vert[0], prev->vert[1], prev->vert[2]);
    }
    rs->max_history = max_history;
    rs->normal_min = normal_min;
    rs->depth_tol = depth_tol;
    rs->albedo_tol2 = albedo_tol * albedo_tol;
    rs->min_weight = min_weight;
}

/* a coordinate within 1/32 of an integer becomes that integer */
MRT_HD float mrt_tp_snap(float f) {
    const float r = floorf(f + 0.5f);
    const float d = f > r ? f - r : r - f;
    return d <= 0.03125f ? r : f;
}

/* pixel (x, y) of the new history frame; hist == NULL: the first frame (pnormal, palbedo and pcam
 * are not read) */
MRT_HD mrt_f4 mrt_reproject_pixel(const mrt_reproject_setup* rs, const mrt_camera* cam, const mrt_camera* pcam, const mrt_f4* rgb,
                                  const mrt_f4* normal, const mrt_f4* albedo, const mrt_f4* hist, const mrt_f4* pnormal, const mrt_f4* palbedo,
                                  unsigned int x, unsigned int y) {
    const unsigned long long W = rs->width;
    const unsigned long long p = (unsigned long long)y * W + x;
    const mrt_f4 cp = rgb[p];
    mrt_f4 o;
    o.x = cp.x;
    o.y = cp.y;
    o.z = cp.z;
    o.w = 1.0f;
    if (!hist) return o;
    /* 1. the current pixel */
    const mrt_f4 np = normal[p], ap = albedo[p];
    const float lp = mrt_tp_dot(np.x, np.y, np.z, np.x, np.y, np.z);
    if (!(np.w == 1.0f) || !(ap.w > 0.0f) || !(lp > 0.0f)) return o;
    /* 2. the world point */
    const float s = ((float)x + 0.5f) / rs->fw, t = ((float)y + 0.5f) / rs->fh;
    const float dx = ((cam->llcorner[0] + s * cam->horz[0]) + t * cam->vert[0]) - cam->origin[0];
    const float dy = ((cam->llcorner[1] + s * cam->horz[1]) + t * cam->vert[1]) - cam->origin[1];
    const float dz = ((cam->llcorner[2] + s * cam->horz[2]) + t * cam->vert[2]) - cam->origin[2];
    const float dl = sqrtf(mrt_tp_dot(dx, dy, dz, dx, dy, dz));
    const float px = cam->origin[0] + ap.w * (dx / dl);
    const float py = cam->origin[1] + ap.w * (dy / dl);
    const float pz = cam->origin[2] + ap.w * (dz / dl);
    /* 3. into the previous camera */
    const float ex = px - pcam->origin[0], ey = py - pcam->origin[1], ez = pz - pcam->origin[2];
    const float zc = -mrt_tp_dot(ex, ey, ez, pcam->w[0], pcam->w[1], pcam->w[2]);
    if (!(zc > 0.0f)) return o;
    const float k = rs->focus / zc;
    const float qx = ex * k - rs->d0[0], qy = ey * k - rs->d0[1], qz = ez * k - rs->d0[2];
    float fx = (mrt_tp_dot(qx, qy, qz, pcam->horz[0], pcam->horz[1], pcam->horz[2]) / rs->hh) * rs->fw - 0.5f;
    float fy = (mrt_tp_dot(qx, qy, qz, pcam->vert[0], pcam->vert[1], pcam->vert[2]) / rs->vv) * rs->fh - 0.5f;
    fx = mrt_tp_snap(fx);
    fy = mrt_tp_snap(fy);
    if (!(fx > -1.0f && fx < rs->fw && fy > -1.0f && fy < rs->fh)) return o;
    /* 4. the taps */
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float el = sqrtf(mrt_tp_dot(ex, ey, ez, ex, ey, ez));
    const float ztol = rs->depth_tol * el;
    const float lps = sqrtf(lp);
    const float n0 = np.x / lps, n1 = np.y / lps, n2 = np.z / lps;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, sw = 0.0f;
    for (int i = 0; i < 4; i++) {
        const int tx = x0 + (i & 1), ty = y0 + (i >> 1);
        const float w = ((i & 1) ? ax : 1.0f - ax) * ((i >> 1) ? ay : 1.0f - ay);
        if (!(w > 0.0f)) continue;
        if (tx < 0 || ty < 0 || tx >= (int)rs->width || ty >= (int)rs->height) continue;
        const unsigned long long q = (unsigned long long)ty * W + (unsigned long long)tx;
        const mrt_f4 nq = pnormal[q];
        if (!(nq.w == 1.0f)) continue;
        const float lq = mrt_tp_dot(nq.x, nq.y, nq.z, nq.x, nq.y, nq.z);
        if (!(lq > 0.0f)) continue;
        const float lqs = sqrtf(lq);
        if (!(mrt_tp_dot(n0, n1, n2, nq.x / lqs, nq.y / lqs, nq.z / lqs) >= rs->normal_min)) continue;
        const mrt_f4 aq = palbedo[q];
        const float dzq = aq.w > el ? aq.w - el : el - aq.w;
        if (!(dzq <= ztol)) continue;
        const float a0 = ap.x - aq.x, a1 = ap.y - aq.y, a2 = ap.z - aq.z;
        if (!(mrt_tp_dot(a0, a1, a2, a0, a1, a2) <= rs->albedo_tol2)) continue;
        const mrt_f4 hq = hist[q];
        s0 = s0 + w * hq.x;
        s1 = s1 + w * hq.y;
        s2 = s2 + w * hq.z;
        s3 = s3 + w * hq.w;
        sw = sw + w;
    }
    /* 5. the blend */
    if (!(sw >= rs->min_weight)) return o;
    const float h0 = s0 / sw, h1 = s1 / sw, h2 = s2 / sw, h3 = s3 / sw;
    const float n1p = h3 + 1.0f;
    const float nn = n1p < rs->max_history ? n1p : rs->max_history;
    const float r = 1.0f / nn;
    o.x = h0 + (cp.x - h0) * r;
    o.y = h1 + (cp.y - h1) * r;
    o.z = h2 + (cp.z - h2) * r;
    o.w = nn;
    return o;
}

#endif
