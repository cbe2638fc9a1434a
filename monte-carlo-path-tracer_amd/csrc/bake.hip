// gfx950 kernels of the surface-baking stage: per bake point -- a face, barycentrics, a side -- one cosine-weighted ray that starts on
// the surface, written as 3 + 3 doubles where wf_shade_kernel reads a probe item's ray (RenderParams::probe_o / probe_d), and the resolve of the
// bake film {sum L, count} into irradiance or outgoing diffuse radiance.  mcpt_bake runs the ray kernel and then the unchanged wavefront pipeline,
// once per sample.
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

dim3 bk_grid(uint32_t n) { return dim3((n + BK_BLOCK - 1) / BK_BLOCK); }

}  // namespace

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
