// gfx950 kernels of the surface-baking stage: per bake point -- a face, barycentrics, a side -- one cosine-weighted ray that starts on
// the surface, written as 3 + 3 doubles where wf_shade_kernel reads a probe item's ray (RenderParams::probe_o / probe_d), and the resolve of the
// bake film {sum L, count} into irradiance or outgoing diffuse radiance.  mcpt_bake runs the ray kernel and then the unchanged wavefront pipeline,
// once per sample.  Between the two stands a first-hit kernel that corrects the records from outside: bk_unlit_kernel (emitters are one-sided for a
// surface point) or, with MCPT_BAKE_DIRECT_MIS, bk_direct_kernel, which also samples the lights at the bake point itself (fp32, tests/bake_direct_ref.py).
//
// One lane per point, no lane reads what another writes.  The corners come from tri_pos64 and the vertex normals from tri_shade, the records every
// context holds and every live-scene update rewrites (rf_triangles_kernel, refit.hip).  tests/bake_ref.py restates the ray in float64, one rounding
// per operation: contraction is off for everything this file adds (the Makefile says so too), sqrt and the divisions are the correctly rounded
// ones and sincos the device library's.  The exception by design: the uv and the texel of MCPT_BAKE_DIFFUSE come from load_hit_shade and tex_color
// of pt_device.h, and that header is compiled here the way the render kernels compile it (contraction allowed), so that the colour is the one
// a shaded hit at that point gets.
#pragma clang fp contract(fast)
#include "pt_device.h"
#pragma clang fp contract(off)
#include "bake.h"

namespace {

#define BK_PI 3.14159265358979323846

struct BkRay { d3 o, n; f3 d; bool dead; };

DEV bool bk_ok(double len) { return len > 0.0 && isfinite(len); }      // a length that can be divided by
DEV double bk_len(d3 a) { return sqrt((a.x * a.x + a.y * a.y) + a.z * a.z); }

// The ray of point `p` as item `item` of sample `sample`.
DEV BkRay bk_ray(const DevScene& sc, const BkPoint p, uint32_t item, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi) {
    const double* P = sc.tri_pos64 + 9 * (size_t)p.tri;
    const d3 v0 = ld_d3(P), v1 = ld_d3(P + 3), v2 = ld_d3(P + 6);
    const float4* S = sc.tri_shade + MCPT_TRI_SHADE_F4 * (size_t)p.tri;
    const float4 s0 = S[0], s1 = S[1], s2 = S[2];
    const double u = (double)p.u, v = (double)p.v, w = (1.0 - u) - v;
    const d3 e1 = mkd(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z), e2 = mkd(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z);
    BkRay r;
    r.o = mkd((v0.x + u * e1.x) + v * e2.x, (v0.y + u * e1.y) + v * e2.y, (v0.z + u * e1.z) + v * e2.z);
    d3 n = mkd((w * (double)s0.x + u * (double)s1.x) + v * (double)s2.x, (w * (double)s0.y + u * (double)s1.y) + v * (double)s2.y,
               (w * (double)s0.z + u * (double)s1.z) + v * (double)s2.z);
    double len = bk_len(n);
    if (!bk_ok(len)) {                                                  // the geometric normal instead
        n = mkd(e1.y * e2.z - e2.y * e1.z, e1.z * e2.x - e2.z * e1.x, e1.x * e2.y - e2.x * e1.y);
        len = bk_len(n);
    }
    r.dead = !bk_ok(len);
    if (r.dead) {                                                       // a proper ray for the pipeline: no NaN, no zero direction
        r.o = mkd(isfinite(r.o.x) ? r.o.x : 0.0, isfinite(r.o.y) ? r.o.y : 0.0, isfinite(r.o.z) ? r.o.z : 0.0);
        r.n = mkd(0.0, 0.0, 0.0); r.d = mk3(0.f, 0.f, 1.f);
        return r;
    }
    n = mkd(n.x / len, n.y / len, n.z / len);
    if (p.flags & MCPT_BAKE_BACK_SIDE) n = mkd(-n.x, -n.y, -n.z);
    r.n = n;
    const Rng4 xi = rng_block(item, sample, 0u, seed_lo, seed_hi);      // block 0: the camera stage's; v[2], v[3] unused and reserved
    const double x0 = (double)xi.v[0], z = sqrt(1.0 - x0), rad = sqrt(x0), th = (2.0 * BK_PI) * (double)xi.v[1];
    double sn, cs; sincos(th, &sn, &cs);
    // the branch-free frame of Duff et al. 2017
    const double s = copysign(1.0, n.z), a = -1.0 / (s + n.z), b = (n.x * n.y) * a;
    const d3 T = mkd(1.0 + s * ((n.x * n.x) * a), s * b, -s * n.x), B = mkd(b, s + (n.y * n.y) * a, -n.y);
    const double rc = rad * cs, rs = rad * sn;
    r.d = mk3((float)((rc * T.x + rs * B.x) + z * n.x), (float)((rc * T.y + rs * B.y) + z * n.y), (float)((rc * T.z + rs * B.z) + z * n.z));
    return r;
}

DEV void bk_store3(double* __restrict__ a, size_t k, double x, double y, double z) { a[3 * k] = x; a[3 * k + 1] = y; a[3 * k + 2] = z; }

__global__ void __launch_bounds__(BK_BLOCK) bk_rays_kernel(DevScene sc, const BkPoint* __restrict__ points, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi,
                                                           double* __restrict__ origin, double* __restrict__ dir, uint8_t* __restrict__ dead) {
    const uint32_t i = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const BkRay r = bk_ray(sc, points[i], i, sample, seed_lo, seed_hi);
    bk_store3(origin, i, r.o.x, r.o.y, r.o.z);
    bk_store3(dir, i, (double)r.d.x, (double)r.d.y, (double)r.d.z);
    dead[i] = r.dead ? 1 : 0;
}

__global__ void __launch_bounds__(BK_BLOCK) bk_probe_kernel(DevScene sc, const BkPoint* __restrict__ points, uint32_t first, uint32_t n, uint32_t sample, uint32_t seed_lo,
                                                            uint32_t seed_hi, double* __restrict__ origin, double* __restrict__ dir, double* __restrict__ normal,
                                                            uint8_t* __restrict__ dead) {
    const uint32_t k = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (k >= n) return;
    const BkRay r = bk_ray(sc, points[first + k], first + k, sample, seed_lo, seed_hi);   // (first + n <= the list's length: mcpt_probe_bake_rays checked)
    bk_store3(origin, k, r.o.x, r.o.y, r.o.z);
    bk_store3(dir, k, (double)r.d.x, (double)r.d.y, (double)r.d.z);
    bk_store3(normal, k, r.n.x, r.n.y, r.n.z);
    dead[k] = r.dead ? 1 : 0;
}

__global__ void __launch_bounds__(BK_BLOCK) bk_resolve_kernel(DevScene sc, const BkPoint* __restrict__ points, const uint8_t* __restrict__ dead,
                                                              const float4* __restrict__ film, uint32_t n, uint32_t mode, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 f = film[i];
    if (dead[i] || !(f.w > 0.f)) { out[i] = make_float4(0.f, 0.f, 0.f, 0.f); return; }
    const float mx = f.x / f.w, my = f.y / f.w, mz = f.z / f.w;        // (the count is an integer held as a float: float(count) is f.w)
    if (mode == MCPT_BAKE_IRRADIANCE) { const float pi = (float)BK_PI; out[i] = make_float4(pi * mx, pi * my, pi * mz, f.w); return; }
    const BkPoint p = points[i];
    const HitShade h = load_hit_shade(sc, p.tri, p.u, p.v, mk3(0.f, 0.f, 1.f));          // (its uv and material; the normal is not used)
    uint32_t fetches = 0;
    const f3 kd = tex_color(sc, sc.mats[h.mat], h.tu, h.tv, fetches);
    out[i] = make_float4(kd.x * mx, kd.y * my, kd.z * mz, f.w);
}

// An item's ray enters the pipeline as a path's PRIMARY ray, and wf_shade_kernel adds the emission of a primary hit whatever side it is hit from
// (the reference shows a lamp's back to the camera, Render.cpp:121-122); hits of later bounces emit from the front only.  For a surface point
// the ray is morally a later bounce: this kernel finds the ray's first hit with the library's one triangle test (bvh_traverse over the
// binary tree, a primary ray's epsilon and acceptance rule, load_hit_shade's side from the traversal's barycentrics) and, where that is an emitter seen from behind, takes the radiance the pass
// is about to add out of the item's record beforehand.  Runs between the ray kernel and the pass; one lane per item, no barrier.
static_assert(BK_BLOCK == MCPT_BLOCK, "bvh_traverse strides its LDS stack by MCPT_BLOCK");
__global__ void __launch_bounds__(BK_BLOCK) bk_unlit_kernel(DevScene sc, const double* __restrict__ origin, const double* __restrict__ dir, const uint8_t* __restrict__ dead,
                                                            uint32_t n, float4* __restrict__ film) {
    __shared__ int s_stack[MCPT_STACK_DEPTH * MCPT_BLOCK];
    int* stk = s_stack + threadIdx.x;
    const uint32_t i = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (i >= n || dead[i]) return;
    const f3 o = to_f3(ld_d3(origin + 3 * (size_t)i)), d = mk3((float)dir[3 * (size_t)i], (float)dir[3 * (size_t)i + 1], (float)dir[3 * (size_t)i + 2]);
    int tri = -1; float ht = 0.f, hu = 0.f, hv = 0.f; TravCount tc = {0, 0};
    if (!bvh_traverse<false, false>(sc, o, d, 1e-4f, 3.0e38f, -1, stk, tri, ht, hu, hv, tc)) return;
    const HitShade hs = load_hit_shade(sc, tri, hu, hv, d);              // (the traversal's fp32 barycentrics, as wf_shade_kernel passes them)
    const DevMaterial& mat = sc.mats[hs.mat];
    if (!(mat.flags & MAT_EMIT_0) || hs.front) return;
    float4 f = film[i];
    f.x -= mat.radiance[0]; f.y -= mat.radiance[1]; f.z -= mat.radiance[2];
    film[i] = f;
}

// MCPT_BAKE_DIRECT_MIS ("Direct light"): next-event estimation at the bake point itself, combined with the cosine ray by the power
// heuristic.  Per live item two terms, both in fp32 with one rounding per operation (tests/bake_direct_ref.py restates them):
//   sub  what the pass is about to add for the cosine ray's first hit and the estimator does not want: the whole radiance of an emitter met from
//        behind (bk_unlit_kernel's rule), the share 1 - w_b of a LIGHT (MAT_EMIT_REC, the light list's membership test) met from its front, nothing
//        for a faint emitter (MAT_EMIT_0 alone: no light sample can reach it) or anything else;
//   add  one light sample from random-number block 0xFFFFFFFF of the item -- a path draws blocks 1 + 2 b and 2 + 2 b and would need 2^31 bounces to
//        get there --, weighted w_l, where the light faces the point, lies above the point's horizon and nothing stands between.
// The bake's own vertex ignores LightSample::self_hit: that quirk exists for parity with a reference that has no baker, so the vertex always
// behaves as MCPT_FLAG_CORRECT_SHADOW_T2 does.  The fields of a term that is not reached stay 0.
struct BkDirect {
    f3 sub, add; float w_b, w_l, p_b, p_l, p_bl, p_lf;
    int hit_tri, front, light_tri, state;                               // leaf-order triangles (-1: none); state: MCPT_BAKE_DIRECT_STATE_* of mcpt.h
};

DEV float bk_dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// P, N: the item's origin and unit normal (bk_ray's), d: its fp32 direction.  Both traversals use the lane's one LDS stack, one after the other.
DEV BkDirect bk_direct(const DevScene& sc, d3 P, d3 N, f3 d, uint32_t item, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, int* stk) {
    BkDirect r;
    r.sub = mk3(0.f, 0.f, 0.f); r.add = mk3(0.f, 0.f, 0.f);
    r.w_b = r.w_l = r.p_b = r.p_l = r.p_bl = r.p_lf = 0.f;
    r.hit_tri = -1; r.front = 0; r.light_tri = -1; r.state = 1;
    const f3 n32 = to_f3(N), o = to_f3(P);
    const float pi = (float)BK_PI, nl = (float)sc.n_lights;
    // ---- A: the cosine ray's first hit, found as bk_unlit_kernel finds it
    int tri = -1; float ht = 0.f, hu = 0.f, hv = 0.f; TravCount tc = {0, 0};
    if (bvh_traverse<false, false>(sc, o, d, 1e-4f, 3.0e38f, -1, stk, tri, ht, hu, hv, tc)) {
        const HitShade hs = load_hit_shade(sc, tri, hu, hv, d);
        const DevMaterial& mat = sc.mats[hs.mat];
        const f3 le = mk3(mat.radiance[0], mat.radiance[1], mat.radiance[2]);
        r.hit_tri = tri; r.front = hs.front ? 1 : 0;
        if ((mat.flags & MAT_EMIT_0) && !hs.front) r.sub = le;
        else if ((mat.flags & MAT_EMIT_REC) && hs.front) {
            r.p_b = fmaxf(bk_dot(d, n32), 0.f) / pi;
            const float cos_l = -bk_dot(d, hs.n);
            r.p_l = cos_l != 0.f ? (ht * ht) * rcp((cos_l * nl) * tri_area(sc, tri)) : 0.f;    // wf_shade_kernel's pdf of a light met by a later bounce
            r.w_b = power_heuristic(r.p_b, r.p_l);
            const float keep = 1.f - r.w_b;
            r.sub = mk3(keep * le.x, keep * le.y, keep * le.z);
        }
    }
    // ---- B: one light sample
    if (sc.n_lights <= 0) return r;                                     // (no context is created without lights: the table is never indexed empty)
    const Rng4 xi = rng_block(item, sample, 0xFFFFFFFFu, seed_lo, seed_hi);
    const LightSample ls = sample_light(sc, P, xi.v[0], xi.v[1], xi.v[2], true);
    r.light_tri = ls.tri;
    if (!(isfinite(ls.pdf) && ls.pdf > 0.f) || !(ls.t2 > 1e-4f)) return r;            // a light seen from behind or in its own plane; a point on the light
    r.state = 2;
    const float cos_p = bk_dot(ls.wo, n32);
    if (!(cos_p > 0.f)) return r;                                       // below the point's horizon
    r.state = 3;
    r.p_bl = cos_p / pi;
    r.p_lf = ls.pdf * rcp(nl);
    r.w_l = power_heuristic(r.p_lf, r.p_bl);
    int stri = -1; float st = 0.f, su = 0.f, sv = 0.f;
    if (bvh_traverse<true, false>(sc, o, ls.wo, 1e-4f, ls.t2, ls.tri, stk, stri, st, su, sv, tc)) return r;   // occluded
    r.state = 4;
    const float ratio = r.p_bl / r.p_lf;
    r.add = mk3((r.w_l * ls.rad.x) * ratio, (r.w_l * ls.rad.y) * ratio, (r.w_l * ls.rad.z) * ratio);
    return r;
}

// Launched INSTEAD of bk_unlit_kernel where the context's mode is MCPT_BAKE_DIRECT_MIS (its `sub` holds that kernel's correction): the first
// traversal is paid once.  The normal is bk_ray's again (the direction's part of bk_ray is dead code here: the fp32 direction comes from the
// ray array the ray kernel filled); the count is left to the pass.  One lane per item, no barrier.
__global__ void __launch_bounds__(BK_BLOCK) bk_direct_kernel(DevScene sc, const BkPoint* __restrict__ points, const double* __restrict__ dir, uint32_t n, uint32_t sample,
                                                             uint32_t seed_lo, uint32_t seed_hi, float4* __restrict__ film) {
    __shared__ int s_stack[MCPT_STACK_DEPTH * MCPT_BLOCK];
    int* stk = s_stack + threadIdx.x;
    const uint32_t i = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const BkRay ray = bk_ray(sc, points[i], i, sample, seed_lo, seed_hi);
    if (ray.dead) return;
    const f3 d = mk3((float)dir[3 * (size_t)i], (float)dir[3 * (size_t)i + 1], (float)dir[3 * (size_t)i + 2]);
    const BkDirect t = bk_direct(sc, ray.o, ray.n, d, i, sample, seed_lo, seed_hi, stk);
    float4 f = film[i];
    const float dx = t.add.x - t.sub.x, dy = t.add.y - t.sub.y, dz = t.add.z - t.sub.z;
    f.x += dx; f.y += dy; f.z += dz;
    film[i] = f;
}

__global__ void __launch_bounds__(BK_BLOCK) bk_direct_probe_kernel(DevScene sc, const BkPoint* __restrict__ points, uint32_t first, uint32_t n, uint32_t sample,
                                                                   uint32_t seed_lo, uint32_t seed_hi, float* __restrict__ out12, int32_t* __restrict__ out4) {
    __shared__ int s_stack[MCPT_STACK_DEPTH * MCPT_BLOCK];
    int* stk = s_stack + threadIdx.x;
    const uint32_t k = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (k >= n) return;
    const BkRay ray = bk_ray(sc, points[first + k], first + k, sample, seed_lo, seed_hi);   // (first + n <= the list's length: mcpt_probe_bake_direct checked)
    float* o12 = out12 + 12 * (size_t)k; int32_t* o4 = out4 + 4 * (size_t)k;
    if (ray.dead) {
        for (int j = 0; j < 12; j++) o12[j] = 0.f;
        o4[0] = -1; o4[1] = 0; o4[2] = -1; o4[3] = MCPT_BAKE_DIRECT_STATE_DEAD;
        return;
    }
    const BkDirect t = bk_direct(sc, ray.o, ray.n, ray.d, first + k, sample, seed_lo, seed_hi, stk);
    o12[0] = t.sub.x; o12[1] = t.sub.y; o12[2] = t.sub.z; o12[3] = t.add.x; o12[4] = t.add.y; o12[5] = t.add.z;
    o12[6] = t.w_b; o12[7] = t.w_l; o12[8] = t.p_b; o12[9] = t.p_l; o12[10] = t.p_bl; o12[11] = t.p_lf;
    o4[0] = t.hit_tri >= 0 ? sc.tri_face[t.hit_tri] : -1; o4[1] = t.front;
    o4[2] = t.light_tri >= 0 ? sc.tri_face[t.light_tri] : -1; o4[3] = t.state;
}

dim3 bk_grid(uint32_t n) { return dim3((n + BK_BLOCK - 1) / BK_BLOCK); }

}  // namespace

hipError_t launch_bk_direct(const DevScene& sc, const BkPoint* points, const double* dir, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, float4* film,
                            hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bk_direct_kernel, bk_grid(n), dim3(BK_BLOCK), 0, stream, sc, points, dir, n, sample, seed_lo, seed_hi, film);
    return hipGetLastError();
}

hipError_t launch_bk_direct_probe(const DevScene& sc, const BkPoint* points, uint32_t first, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, float* out12,
                                  int32_t* out4, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bk_direct_probe_kernel, bk_grid(n), dim3(BK_BLOCK), 0, stream, sc, points, first, n, sample, seed_lo, seed_hi, out12, out4);
    return hipGetLastError();
}

hipError_t launch_bk_rays(const DevScene& sc, const BkPoint* points, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin, double* dir,
                          uint8_t* dead, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bk_rays_kernel, bk_grid(n), dim3(BK_BLOCK), 0, stream, sc, points, n, sample, seed_lo, seed_hi, origin, dir, dead);
    return hipGetLastError();
}

hipError_t launch_bk_unlit(const DevScene& sc, const double* origin, const double* dir, const uint8_t* dead, uint32_t n, float4* film, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bk_unlit_kernel, bk_grid(n), dim3(BK_BLOCK), 0, stream, sc, origin, dir, dead, n, film);
    return hipGetLastError();
}

hipError_t launch_bk_probe(const DevScene& sc, const BkPoint* points, uint32_t first, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin,
                           double* dir, double* normal, uint8_t* dead, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bk_probe_kernel, bk_grid(n), dim3(BK_BLOCK), 0, stream, sc, points, first, n, sample, seed_lo, seed_hi, origin, dir, normal, dead);
    return hipGetLastError();
}

hipError_t launch_bk_resolve(const DevScene& sc, const BkPoint* points, const uint8_t* dead, const float4* film, uint32_t n, uint32_t mode, float4* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bk_resolve_kernel, bk_grid(n), dim3(BK_BLOCK), 0, stream, sc, points, dead, film, n, mode, out);
    return hipGetLastError();
}
