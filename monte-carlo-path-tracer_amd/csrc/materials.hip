// gfx950 kernels of the material update: mcpt_update_materials edits what a surface looks like on a live scene -- same geometry,
// same trees.  What changes on the device is small: the 64-B material records (copied in by the host), four bits per triangle (the lobe class in
// tri_isect[3 i].w) and the light list, whose membership follows |radiance| > 0.01 (and, on a context with a visibility mask, "visible": §24) and
// whose order is the input's face order, not the leaf order: a stream compaction over the faces.  Everything a light record holds is resident already (tri_isect, tri_shade, tri_pos64, mats).
//
// Everything runs on the context's stream, ordered like a render call.  The scan is three launches (per-block sums, one block over the sums, the
// per-block scan from its offset): a launch reads only what earlier launches wrote, so no block ever waits for another block of its own launch.
//
// Floating-point contraction is OFF in this file (the library is built with -ffp-contract=fast): mt_emit_kernel restates build_host_scene's light
// record operation for operation, and the host's x86 code does not fuse.  Plain C++ loads and vector stores only.
#include "materials.h"

#pragma clang fp contract(off)

namespace {

// Exclusive scan of one value per thread over the block; *total = the block's sum.  s: MT_BLOCK words of LDS.
__device__ __forceinline__ uint32_t mt_block_scan(uint32_t v, uint32_t* s, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < MT_BLOCK; d <<= 1) {                        // Hillis-Steele inclusive scan
        const uint32_t a = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    *total = s[MT_BLOCK - 1];
    return s[t] - v;
}

__device__ __forceinline__ uint32_t mt_material_of(const float4* __restrict__ tri_shade, uint32_t i) {
    return __float_as_uint(tri_shade[(size_t)MCPT_TRI_SHADE_F4 * i + 3].w);
}

// ---------------------------------------------------------------------------------------------- lobe classes and light flags
__global__ void __launch_bounds__(MT_BLOCK) mt_classes_kernel(float4* __restrict__ tri_isect, const float4* __restrict__ tri_shade, const int32_t* __restrict__ tri_face,
                                                              const DevMaterial* __restrict__ mats, uint32_t n_mats, uint32_t* __restrict__ flag, uint32_t n_tris,
                                                              const uint8_t* __restrict__ visible) {
    const uint32_t i = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= n_tris) return;
    const uint32_t m = mt_material_of(tri_shade, i), face = (uint32_t)tri_face[i];
    if (m >= n_mats || face >= n_tris) return;                            // (cannot happen: mcpt_create checked both)
    const uint32_t mflags = mats[m].flags;
    const uint32_t lobe_class = !(mflags & MAT_HAS_SPEC) ? HIT_CLASS_DIFFUSE : (mflags & MAT_MIRROR) ? HIT_CLASS_MIRROR : HIT_CLASS_PHONG;
    float4* I = tri_isect + 3 * (size_t)i;
    float4 r = I[0];
    r.w = __uint_as_float((__float_as_uint(r.w) & (uint32_t)HIT_TRI_MASK) | (lobe_class << HIT_CLASS_SHIFT));   // the tie rank stays
    I[0] = r;
    flag[face] = (mflags & MAT_EMIT_REC) && (!visible || visible[face]) ? 1u : 0u;   // §24: a hidden face is no light
}

// ---------------------------------------------------------------------------------------------- exclusive scan in face order
__global__ void __launch_bounds__(MT_BLOCK) mt_sums_kernel(const uint32_t* __restrict__ flag, uint32_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_part[MT_BLOCK / 64];
    const uint32_t i = blockIdx.x * MT_BLOCK + threadIdx.x;
    uint32_t v = i < n ? flag[i] : 0u;
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t t = 0u; for (int w = 0; w < MT_BLOCK / 64; w++) t += s_part[w]; sums[blockIdx.x] = t; }
}

// One block: thread t adds up a contiguous run of the block sums, the scan over the MT_BLOCK runs gives every block the number of lights before it.
__global__ void __launch_bounds__(MT_BLOCK) mt_offsets_kernel(uint32_t* __restrict__ sums, uint32_t nb) {
    __shared__ uint32_t s_scan[MT_BLOCK];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nb + MT_BLOCK - 1) / MT_BLOCK;
    const uint32_t lo = min(nb, t * per), hi = min(nb, lo + per);
    uint32_t run = 0u, total;
    for (uint32_t b = lo; b < hi; b++) run += sums[b];
    run = mt_block_scan(run, s_scan, &total);
    for (uint32_t b = lo; b < hi; b++) { const uint32_t v = sums[b]; sums[b] = run; run += v; }   // (a thread reads and writes its own run only)
}

__global__ void __launch_bounds__(MT_BLOCK) mt_apply_kernel(uint32_t* __restrict__ flag, uint32_t n, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_scan[MT_BLOCK];
    const uint32_t i = blockIdx.x * MT_BLOCK + threadIdx.x;
    uint32_t total;
    const uint32_t before = mt_block_scan(i < n ? flag[i] : 0u, s_scan, &total);
    if (i < n) flag[i] = sums[blockIdx.x] + before;
}

// ---------------------------------------------------------------------------------------------- light records
// build_host_scene's "lights in face order" loop (scene_build.cpp) for one triangle: slot = the number of lights among the faces before its own.
__global__ void __launch_bounds__(MT_BLOCK) mt_emit_kernel(const float4* __restrict__ tri_isect, const float4* __restrict__ tri_shade, const double* __restrict__ tri_pos64,
                                                           const int32_t* __restrict__ tri_face, const DevMaterial* __restrict__ mats, uint32_t n_mats,
                                                           const uint32_t* __restrict__ scan, DevLight* __restrict__ lights, double* __restrict__ light_pos64,
                                                           uint32_t capacity, uint32_t n_tris, const uint8_t* __restrict__ visible) {
    const uint32_t i = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= n_tris) return;
    const uint32_t m = mt_material_of(tri_shade, i), face = (uint32_t)tri_face[i];
    if (m >= n_mats || face >= n_tris) return;
    if (visible && !visible[face]) return;                                // §24: a hidden emitter has no slot (scan[face] is the next visible light's)
    const float4* M = reinterpret_cast<const float4*>(mats + m);         // 64 B: ks ns | radiance flags | ...
    const float4 rad = M[1];
    if (!(__float_as_uint(rad.w) & MAT_EMIT_REC)) return;
    const uint32_t slot = scan[face];
    if (slot >= capacity) return;                                         // (cannot happen: the host sized the list from the same test)
    const float4 e1 = tri_isect[3 * (size_t)i + 1], e2 = tri_isect[3 * (size_t)i + 2];
    const float cx = e1.y * e2.z - e2.y * e1.z, cy = e1.z * e2.x - e2.z * e1.x, cz = e1.x * e2.y - e2.x * e1.y;
    const float area = 0.5f * (float)sqrt((double)((cx * cx + cy * cy) + cz * cz));   // (fp64 root rounded once = the correctly rounded fp32 root of std::sqrt)
    const float4* S = tri_shade + (size_t)MCPT_TRI_SHADE_F4 * i;
    const float4 n0 = S[0], n1 = S[1], n2 = S[2];
    float4* R = reinterpret_cast<float4*>(lights + slot);                 // 64 B: tri area rad.xy | rad.z n0.xyz | n1.xyz n2.x | n2.yz pad pad
    R[0] = make_float4(__int_as_float((int)i), area, rad.x, rad.y);
    R[1] = make_float4(rad.z, n0.x, n0.y, n0.z);
    R[2] = make_float4(n1.x, n1.y, n1.z, n2.x);
    R[3] = make_float4(n2.y, n2.z, 0.f, 0.f);
    for (int a = 0; a < 9; a++) light_pos64[9 * (size_t)slot + a] = tri_pos64[9 * (size_t)i + a];
}

}  // namespace

hipError_t launch_mt_classes(float4* tri_isect, const float4* tri_shade, const int32_t* tri_face, const DevMaterial* mats, uint32_t n_mats,
                             uint32_t* flag, uint32_t n_tris, hipStream_t stream, const uint8_t* visible) {
    if (n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_classes_kernel, dim3(mt_blocks(n_tris)), dim3(MT_BLOCK), 0, stream, tri_isect, tri_shade, tri_face, mats, n_mats, flag, n_tris, visible);
    return hipGetLastError();
}

hipError_t launch_mt_scan(uint32_t* flag, uint32_t* sums, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t nb = mt_blocks(n);
    hipLaunchKernelGGL(mt_sums_kernel, dim3(nb), dim3(MT_BLOCK), 0, stream, flag, n, sums);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mt_offsets_kernel, dim3(1), dim3(MT_BLOCK), 0, stream, sums, nb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(mt_apply_kernel, dim3(nb), dim3(MT_BLOCK), 0, stream, flag, n, sums);
    return hipGetLastError();
}

hipError_t launch_mt_emit(const float4* tri_isect, const float4* tri_shade, const double* tri_pos64, const int32_t* tri_face, const DevMaterial* mats,
                          uint32_t n_mats, const uint32_t* scan, DevLight* lights, double* light_pos64, uint32_t capacity, uint32_t n_tris,
                          hipStream_t stream, const uint8_t* visible) {
    if (n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_emit_kernel, dim3(mt_blocks(n_tris)), dim3(MT_BLOCK), 0, stream, tri_isect, tri_shade, tri_pos64, tri_face, mats, n_mats, scan, lights,
                       light_pos64, capacity, n_tris, visible);
    return hipGetLastError();
}
