// gfx950 kernels of the light-probe stage: a probe is a point in free space, no surface and no normal; it stores the radiance
// around it as 9 spherical-harmonic coefficients per colour channel (bands 0 .. 2).  Per pass every probe starts SH_DIRS = 64 rays, one wave64
// per probe: item i is probe i >> 6 and direction slot i & 63 of an 8 x 8 stratification of the sphere.  mcpt_bake_sh runs, per pass, the ray
// kernel, the first-hit kernel (emitters are one-sided for a free-space point too, and every item gets a class byte: miss, front, back), the
// unchanged wavefront pipeline into a scratch film of one record per item, and the projection kernel, which reduces the wave's 64 x 27 products
// in ONE fixed order and adds them to the probe's accumulators.
//
// tests/shprobe_ref.py restates all of it: the ray in float64, one rounding per operation (contraction is off for everything this file adds -- the
// Makefile says so too --, sqrt and the divisions are the correctly rounded ones and sincos the device library's), the basis, the products and
// the tree in fp32, bit for bit.  pt_device.h is compiled here the way the render kernels compile it (contraction allowed): bvh_traverse and
// load_hit_shade give the first hit the pipeline's own kernels would give.
#pragma clang fp contract(fast)
#include "pt_device.h"
#pragma clang fp contract(off)
#include "shprobe.h"

namespace {

#define SH_PI 3.14159265358979323846

struct ShRay { d3 o; f3 d; };

// The ray of item `item` (probe item >> 6, slot item & 63) of sample `sample`.
DEV ShRay sh_ray(const double* __restrict__ pos, uint32_t item, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi) {
    const uint32_t j = item & (SH_DIRS - 1u), jx = j & 7u, jy = j >> 3;
    ShRay r;
    r.o = ld_d3(pos + 3 * (size_t)(item >> 6));
    const Rng4 xi = rng_block(item, sample, 0u, seed_lo, seed_hi);      // block 0: the camera and bake stages'; v[2], v[3] unused and reserved
    const double u = ((double)jx + (double)xi.v[0]) / 8.0, v = ((double)jy + (double)xi.v[1]) / 8.0;
    const double z = 1.0 - 2.0 * u, rad = 2.0 * sqrt(u * (1.0 - u)), phi = (2.0 * SH_PI) * v;
    double sn, cs; sincos(phi, &sn, &cs);
    r.d = mk3((float)(rad * cs), (float)(rad * sn), (float)z);
    return r;
}

DEV void sh_store3(double* __restrict__ a, size_t k, double x, double y, double z) { a[3 * k] = x; a[3 * k + 1] = y; a[3 * k + 2] = z; }

__global__ void __launch_bounds__(SH_BLOCK) sh_rays_kernel(const double* __restrict__ pos, uint32_t n_items, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi,
                                                           double* __restrict__ origin, double* __restrict__ dir) {
    const uint32_t i = blockIdx.x * SH_BLOCK + threadIdx.x;
    if (i >= n_items) return;
    const ShRay r = sh_ray(pos, i, sample, seed_lo, seed_hi);
    sh_store3(origin, i, r.o.x, r.o.y, r.o.z);
    sh_store3(dir, i, (double)r.d.x, (double)r.d.y, (double)r.d.z);
}

__global__ void __launch_bounds__(SH_BLOCK) sh_probe_kernel(const double* __restrict__ pos, uint32_t first, uint32_t n_items, uint32_t sample, uint32_t seed_lo,
                                                            uint32_t seed_hi, double* __restrict__ origin, double* __restrict__ dir) {
    const uint32_t k = blockIdx.x * SH_BLOCK + threadIdx.x;
    if (k >= n_items) return;
    const ShRay r = sh_ray(pos, first + k, sample, seed_lo, seed_hi);   // (first + n_items <= 64 x the number of probes: mcpt_probe_sh_rays checked)
    sh_store3(origin, k, r.o.x, r.o.y, r.o.z);
    sh_store3(dir, k, (double)r.d.x, (double)r.d.y, (double)r.d.z);
}

// bk_unlit_kernel's rule (bake.hip) with the same traversal call: an item's ray enters the pipeline as a path's PRIMARY ray, whose hit on an
// emitter adds its radiance whatever side it is hit from; a free-space point must not see a lamp's back, so that radiance leaves the item's
// (zeroed) record before the pass adds it.  The class byte is the hit's side, emitter or not.  One lane per item, no barrier.
static_assert(SH_BLOCK == MCPT_BLOCK, "bvh_traverse strides its LDS stack by MCPT_BLOCK");
__global__ void __launch_bounds__(SH_BLOCK) sh_first_hit_kernel(DevScene sc, const double* __restrict__ origin, const double* __restrict__ dir, uint32_t n_items,
                                                                float4* __restrict__ film, uint8_t* __restrict__ cls) {
    __shared__ int s_stack[MCPT_STACK_DEPTH * MCPT_BLOCK];
    int* stk = s_stack + threadIdx.x;
    const uint32_t i = blockIdx.x * SH_BLOCK + threadIdx.x;
    if (i >= n_items) return;
    const f3 o = to_f3(ld_d3(origin + 3 * (size_t)i)), d = mk3((float)dir[3 * (size_t)i], (float)dir[3 * (size_t)i + 1], (float)dir[3 * (size_t)i + 2]);
    int tri = -1; float ht = 0.f, hu = 0.f, hv = 0.f; TravCount tc = {0, 0};
    if (!bvh_traverse<false, false>(sc, o, d, 1e-4f, 3.0e38f, -1, stk, tri, ht, hu, hv, tc)) { cls[i] = 0; return; }
    const HitShade hs = load_hit_shade(sc, tri, hu, hv, d);              // (the traversal's fp32 barycentrics, as wf_shade_kernel passes them)
    cls[i] = hs.front ? 1 : 2;
    const DevMaterial& mat = sc.mats[hs.mat];
    if (!(mat.flags & MAT_EMIT_0) || hs.front) return;
    float4 f = film[i];
    f.x -= mat.radiance[0]; f.y -= mat.radiance[1]; f.z -= mat.radiance[2];
    film[i] = f;
}

// The wave's sum of v in the tree s[j] + s[j + 32], then + 16, ... + 1, as lane 0 sees it: an xor butterfly (fp32 addition commutes, so every
// lane ends with lane 0's bits).
DEV float sh_wave_sum(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

DEV float sh_finite(float x) { return isfinite(x) ? x : 0.f; }

// One wave per probe (4 per block); a wave whose probe is >= n leaves as a whole, so every shuffle below has its 64 lanes.
__global__ void __launch_bounds__(SH_BLOCK) sh_project_kernel(const float4* __restrict__ film, const double* __restrict__ dir, const uint8_t* __restrict__ cls, uint32_t n,
                                                              float* __restrict__ acc, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u, p = blockIdx.x * (SH_BLOCK / 64) + (threadIdx.x >> 6);
    if (p >= n) return;
    const size_t i = (size_t)p * SH_DIRS + lane;
    const float4 f = film[i];
    const float L[3] = {sh_finite(f.x), sh_finite(f.y), sh_finite(f.z)};
    const float x = (float)dir[3 * i], y = (float)dir[3 * i + 1], z = (float)dir[3 * i + 2];
    const float c1 = 0.4886025119029199f, c2 = 1.0925484305920792f;
    const float Y[9] = {0.28209479177387814f, c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), 0.31539156525252005f * (3.f * (z * z) - 1.f), c2 * (x * z),
                        0.5462742152960396f * ((x * x) - (y * y))};
    float sum[SH_COEFFS];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 9; k++) sum[9 * c + k] = sh_wave_sum(L[c] * Y[k]);
    const uint8_t k = cls[i];
    const uint32_t back = (uint32_t)__popcll(__ballot(k == 2)), miss = (uint32_t)__popcll(__ballot(k == 0));
    if (lane != 0) return;
    float* a = acc + (size_t)SH_COEFFS * p;                             // one writer per probe, passes ordered on the stream
#pragma unroll
    for (int q = 0; q < SH_COEFFS; q++) a[q] = a[q] + sum[q];
    uint32_t* n3 = counts + 3 * (size_t)p;
    n3[0] += SH_DIRS; n3[1] += back; n3[2] += miss;
}

__global__ void __launch_bounds__(SH_BLOCK) sh_resolve_kernel(const float* __restrict__ acc, const uint32_t* __restrict__ counts, uint32_t n, uint32_t mode,
                                                              float* __restrict__ out) {
    const uint32_t p = blockIdx.x * SH_BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t rays = counts[3 * (size_t)p];
    const float kf = rays ? (float)(4.0 * SH_PI) / (float)rays : 0.f;
    const float band[3] = {(float)SH_PI, (float)(2.0 * SH_PI / 3.0), (float)(SH_PI / 4.0)};
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 9; k++) {
            const size_t q = (size_t)SH_COEFFS * p + 9 * c + k;
            const float r = rays ? kf * acc[q] : 0.f;
            out[q] = mode == MCPT_SH_IRRADIANCE ? band[k == 0 ? 0 : k < 4 ? 1 : 2] * r : r;
        }
}

dim3 sh_grid(uint32_t n) { return dim3((n + SH_BLOCK - 1) / SH_BLOCK); }

}  // namespace

hipError_t launch_sh_rays(const double* pos, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin, double* dir, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sh_rays_kernel, sh_grid(n * SH_DIRS), dim3(SH_BLOCK), 0, stream, pos, n * SH_DIRS, sample, seed_lo, seed_hi, origin, dir);
    return hipGetLastError();
}

hipError_t launch_sh_probe(const double* pos, uint32_t first, uint32_t n_items, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin, double* dir,
                           hipStream_t stream) {
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(sh_probe_kernel, sh_grid(n_items), dim3(SH_BLOCK), 0, stream, pos, first, n_items, sample, seed_lo, seed_hi, origin, dir);
    return hipGetLastError();
}

hipError_t launch_sh_first_hit(const DevScene& sc, const double* origin, const double* dir, uint32_t n_items, float4* film, uint8_t* cls, hipStream_t stream) {
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(sh_first_hit_kernel, sh_grid(n_items), dim3(SH_BLOCK), 0, stream, sc, origin, dir, n_items, film, cls);
    return hipGetLastError();
}

hipError_t launch_sh_project(const float4* film, const double* dir, const uint8_t* cls, uint32_t n, float* acc, uint32_t* counts, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sh_project_kernel, dim3((n + SH_BLOCK / 64 - 1) / (SH_BLOCK / 64)), dim3(SH_BLOCK), 0, stream, film, dir, cls, n, acc, counts);
    return hipGetLastError();
}

hipError_t launch_sh_resolve(const float* acc, const uint32_t* counts, uint32_t n, uint32_t mode, float* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sh_resolve_kernel, sh_grid(n), dim3(SH_BLOCK), 0, stream, acc, counts, n, mode, out);
    return hipGetLastError();
}
