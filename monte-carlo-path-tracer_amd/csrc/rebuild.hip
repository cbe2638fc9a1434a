// gfx950 kernels of the tree rebuild: mcpt_rebuild_trees builds both trees anew for the vertices a live context holds and keeps
// everything else.  The builders run where mcpt_create runs them (scene_build.cpp: build_trees); what the device does here is
//   rb_face_bounds_kernel  the builders' input, formed from rf_vtx: per face the fp32 box and, for the host builder, the fp64 bound + centroid;
//   rb_permute_kernel      every leaf-order stream moved from the old leaf order to the new one, out of place, 16 destination bytes per lane;
//   rb_lights_kernel       DevLight::tri renumbered.
// No record is recomputed: the refit kernels keep the streams bit for bit what build_host_scene would form for the current vertices, so moving
// them gives what a fresh mcpt_create would upload.
//
// Floating-point contraction is OFF in this file, as in refit.hip: rb_face_bounds_kernel restates build_host_scene's bounds operation for
// operation (its min / max are std::min / std::max spelled out: fmin / fmax may pick the other zero of a +0 / -0 pair).  Plain C++ loads and
// vector stores only; no lane reads what another lane of its launch writes, so there are no atomics, fences or barriers.
#include "rebuild.h"

#pragma clang fp contract(off)

namespace {

// scene_build.cpp: round_down / round_up with a pad of 0
__device__ __forceinline__ float rb_down(double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; }
__device__ __forceinline__ float rb_up(double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; }
__device__ __forceinline__ double rb_min(double a, double b) { return b < a ? b : a; }   // std::min
__device__ __forceinline__ double rb_max(double a, double b) { return a < b ? b : a; }   // std::max

// ---------------------------------------------------------------------------------------------- the builders' input
__global__ void __launch_bounds__(RB_BLOCK) rb_face_bounds_kernel(const double* __restrict__ vertex, const int32_t* __restrict__ idx6, const int32_t* __restrict__ tri_face,
                                                                  RfCentre ctr, float* __restrict__ box32, double* __restrict__ bound64, uint32_t n_tris) {
    const uint32_t i = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (i >= n_tris) return;
    const uint32_t f = (uint32_t)tri_face[i];
    if (f >= n_tris) return;                                                          // (the host has checked the order: never taken)
    const int2* ip = reinterpret_cast<const int2*>(idx6 + 6 * (size_t)i);
    const int2 i01 = ip[0], i2n = ip[1];
    const double* w0 = vertex + 3 * (size_t)i01.x; const double* w1 = vertex + 3 * (size_t)i01.y; const double* w2 = vertex + 3 * (size_t)i2n.x;
    const double c[3] = {ctr.x, ctr.y, ctr.z};
    double lo[3], hi[3], cen[3];
    for (int a = 0; a < 3; a++) {
        const double x0 = w0[a] - c[a], x1 = w1[a] - c[a], x2 = w2[a] - c[a];
        lo[a] = rb_min(x0, rb_min(x1, x2)); hi[a] = rb_max(x0, rb_max(x1, x2));
        cen[a] = (x0 + x1 + x2) / 3.0;
    }
    float2* b = reinterpret_cast<float2*>(box32 + 6 * (size_t)f);                      // 24-B records: 8-B aligned
    b[0] = make_float2(rb_down(lo[0]), rb_down(lo[1])); b[1] = make_float2(rb_down(lo[2]), rb_up(hi[0])); b[2] = make_float2(rb_up(hi[1]), rb_up(hi[2]));
    if (bound64) {
        double* B = bound64 + 9 * (size_t)f;
        for (int a = 0; a < 3; a++) { B[a] = lo[a]; B[3 + a] = hi[a]; B[6 + a] = cen[a]; }
    }
}

// ---------------------------------------------------------------------------------------------- the streams, old leaf order -> new
// Lane u owns 16 bytes of one destination stream; the streams follow each other in u (rb_permute_units).  A wave's stores are contiguous; the
// lanes that share a source record read it contiguously.  tri_pos64 (72 B), idx6 (24 B) and tri_face (4 B) records are no multiple of 16 B: a
// unit is put together from the 8-B or 4-B pieces of up to two (tri_face: four) source records, and the last unit of a stream may be short.
__global__ void __launch_bounds__(RB_BLOCK) rb_permute_kernel(RbStreams src, RbStreams dst, const uint32_t* __restrict__ src_of_dst, uint32_t n_tris, uint32_t keep_rank) {
    const uint64_t N = n_tris;
    uint64_t u = (uint64_t)blockIdx.x * RB_BLOCK + threadIdx.x;
    if (u < 8 * N) {                                                                  // tri_shade: 8 units per record, one 128-B line
        const uint32_t i = (uint32_t)(u >> 3), k = (uint32_t)u & 7u;
        dst.tri_shade[u] = src.tri_shade[(size_t)MCPT_TRI_SHADE_F4 * src_of_dst[i] + k];
        return;
    }
    u -= 8 * N;
    if (u < 3 * N) {                                                                  // tri_isect: 3 units per record
        const uint32_t i = (uint32_t)(u / 3), k = (uint32_t)(u - 3 * (uint64_t)i);
        float4 r = src.tri_isect[3 * (size_t)src_of_dst[i] + k];
        if (k == 0 && !keep_rank) r.w = __uint_as_float((__float_as_uint(r.w) & ~(uint32_t)HIT_TRI_MASK) | i);   // lobe class kept, tie rank = the new position
        dst.tri_isect[u] = r;
        return;
    }
    u -= 3 * N;
    const uint64_t n_dbl = 9 * N, u_pos = (n_dbl + 1) / 2;
    if (u < u_pos) {                                                                  // tri_pos64: doubles 2u and 2u + 1
        const uint64_t d0 = 2 * u;
        const uint32_t i0 = (uint32_t)(d0 / 9), k0 = (uint32_t)(d0 - 9 * (uint64_t)i0);
        const double a = src.tri_pos64[9 * (size_t)src_of_dst[i0] + k0];
        if (d0 + 1 < n_dbl) {
            const uint32_t i1 = k0 == 8u ? i0 + 1u : i0, k1 = k0 == 8u ? 0u : k0 + 1u;
            const double b = src.tri_pos64[9 * (size_t)src_of_dst[i1] + k1];
            reinterpret_cast<double2*>(dst.tri_pos64)[u] = make_double2(a, b);
        } else dst.tri_pos64[d0] = a;
        return;
    }
    u -= u_pos;
    const uint64_t n_pair = 3 * N, u_idx = (n_pair + 1) / 2;
    if (u < u_idx) {                                                                  // idx6: index pairs 2u and 2u + 1
        const uint64_t p0 = 2 * u;
        const uint32_t i0 = (uint32_t)(p0 / 3), k0 = (uint32_t)(p0 - 3 * (uint64_t)i0);
        const int2 a = reinterpret_cast<const int2*>(src.idx6)[3 * (size_t)src_of_dst[i0] + k0];
        if (p0 + 1 < n_pair) {
            const uint32_t i1 = k0 == 2u ? i0 + 1u : i0, k1 = k0 == 2u ? 0u : k0 + 1u;
            const int2 b = reinterpret_cast<const int2*>(src.idx6)[3 * (size_t)src_of_dst[i1] + k1];
            reinterpret_cast<int4*>(dst.idx6)[u] = make_int4(a.x, a.y, b.x, b.y);
        } else reinterpret_cast<int2*>(dst.idx6)[p0] = a;
        return;
    }
    u -= u_idx;
    if (u < (N + 3) / 4) {                                                            // tri_face: four records
        const uint32_t i = (uint32_t)(4 * u);
        if (i + 3u < n_tris) {
            reinterpret_cast<int4*>(dst.tri_face)[u] = make_int4(src.tri_face[src_of_dst[i]], src.tri_face[src_of_dst[i + 1u]], src.tri_face[src_of_dst[i + 2u]],
                                                                 src.tri_face[src_of_dst[i + 3u]]);
        } else for (uint32_t j = i; j < n_tris; j++) dst.tri_face[j] = src.tri_face[src_of_dst[j]];
    }
}

// ---------------------------------------------------------------------------------------------- lights
__global__ void __launch_bounds__(RB_BLOCK) rb_lights_kernel(DevLight* __restrict__ lights, const uint32_t* __restrict__ dst_of_src, uint32_t n_lights, uint32_t n_tris) {
    const uint32_t k = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (k >= n_lights) return;
    const uint32_t tri = (uint32_t)lights[k].tri;
    if (tri < n_tris) lights[k].tri = (int32_t)dst_of_src[tri];
}

}  // namespace

hipError_t launch_rb_face_bounds(const double* vertex, const int32_t* idx6, const int32_t* tri_face, RfCentre centre, float* box32, double* bound64,
                                 uint32_t n_tris, hipStream_t stream) {
    if (n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_face_bounds_kernel, dim3((n_tris + RB_BLOCK - 1) / RB_BLOCK), dim3(RB_BLOCK), 0, stream, vertex, idx6, tri_face, centre, box32, bound64, n_tris);
    return hipGetLastError();
}

hipError_t launch_rb_permute(RbStreams src, RbStreams dst, const uint32_t* src_of_dst, uint32_t n_tris, bool keep_rank, hipStream_t stream) {
    if (n_tris == 0) return hipSuccess;
    const uint64_t blocks = (rb_permute_units(n_tris) + RB_BLOCK - 1) / RB_BLOCK;      // n_tris < 2^28: below 2^25 blocks
    hipLaunchKernelGGL(rb_permute_kernel, dim3((uint32_t)blocks), dim3(RB_BLOCK), 0, stream, src, dst, src_of_dst, n_tris, keep_rank ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_rb_lights(DevLight* lights, const uint32_t* dst_of_src, uint32_t n_lights, uint32_t n_tris, hipStream_t stream) {
    if (n_lights == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_lights_kernel, dim3((n_lights + RB_BLOCK - 1) / RB_BLOCK), dim3(RB_BLOCK), 0, stream, lights, dst_of_src, n_lights, n_tris);
    return hipGetLastError();
}
