// gfx950 kernel of the face-visibility pass: a live context shows and hides faces without a new upload, new trees or a lost film.
// A hidden triangle keeps its place in every stream; what changes is that nothing can hit it: both edge records become +0, so the determinant `a`
// of the one tri_test every traversal kernel shares is exactly +-0 for every ray and fails |a| >= 1e-5 (closest hit) and |a| >= 1e-6 (any hit).
// Its box becomes the point v0, so the refit that follows -- unchanged -- stops counting it in its ancestors' boxes, and the soundness walks still
// find the (degenerate) triangle inside its leaf.
//
// Runs on the context's stream between rf_triangles_kernel, which has just rewritten every record from the vertices, and the level loops of the
// refit.  One lane per triangle, no lane reads what another writes.  No arithmetic at all; contraction is off as in refit.hip, one rule for the
// files of the scene update.  Plain C++ loads and vector stores only.
#include "visibility.h"

#pragma clang fp contract(off)

namespace {

__global__ void __launch_bounds__(VS_BLOCK) vs_hide_kernel(const uint8_t* __restrict__ visible, const int32_t* __restrict__ tri_face, float4* __restrict__ tri_isect,
                                                           float* __restrict__ tri_box, uint32_t n_tris) {
    const uint32_t i = blockIdx.x * VS_BLOCK + threadIdx.x;
    if (i >= n_tris) return;
    const uint32_t face = (uint32_t)tri_face[i];
    if (face >= n_tris || visible[face]) return;                          // (face >= n_tris cannot happen: mcpt_create checked the leaf order)
    float4* I = tri_isect + 3 * (size_t)i;
    const float4 v0 = I[0];
    I[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    I[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    float2* b = reinterpret_cast<float2*>(tri_box + 6 * (size_t)i);       // 24-B records: 8-B aligned (refit.hip: rf_store_box)
    b[0] = make_float2(v0.x, v0.y); b[1] = make_float2(v0.z, v0.x); b[2] = make_float2(v0.y, v0.z);
}

}  // namespace

hipError_t launch_vs_hide(const uint8_t* visible, const int32_t* tri_face, float4* tri_isect, float* tri_box, uint32_t n_tris, hipStream_t stream) {
    if (n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(vs_hide_kernel, dim3((n_tris + VS_BLOCK - 1) / VS_BLOCK), dim3(VS_BLOCK), 0, stream, visible, tri_face, tri_isect, tri_box, n_tris);
    return hipGetLastError();
}
