// gfx950 kernels of the rigid-part update: mcpt_update_transforms moves the parts of a live scene by one 3x4 matrix per group.
// The rest pose (vertices and normals as they were when mcpt_set_vertex_groups was called) and a group id per vertex and per normal stay on the
// device; per call only the table of matrices crosses the bus.  The two kernels here write the context's CURRENT arrays (rf_vtx / rf_nrm) from
// the rest pose; the refit of refit.hip follows on the same stream, exactly as after mcpt_update_vertices' upload.
//
// Floating-point contraction is OFF in this file, as in refit.hip: every product, sum, quotient and root below is one correctly rounded fp64
// operation in a fixed association, so tests/transform_ref.py (numpy, the same association) gives the same arrays bit for bit.  Plain C++ loads
// and vector stores only.
#include "transform.h"

#pragma clang fp contract(off)

void xf_group_record(const double* m, double* r) {
    for (int k = 0; k < 12; k++) r[k] = m[k];
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    r[12] = a11 * a22 - a12 * a21; r[13] = a12 * a20 - a10 * a22; r[14] = a10 * a21 - a11 * a20;
    r[15] = a02 * a21 - a01 * a22; r[16] = a00 * a22 - a02 * a20; r[17] = a01 * a20 - a00 * a21;
    r[18] = a01 * a12 - a02 * a11; r[19] = a02 * a10 - a00 * a12; r[20] = a00 * a11 - a01 * a10;
}

double xf_record_det(const double* r) { return (r[0] * r[12] + r[1] * r[13]) + r[2] * r[14]; }
double xf_row_reach(const double* a, double radius) { return ((fabs(a[0]) + fabs(a[1])) + fabs(a[2])) * radius + fabs(a[3]); }

namespace {

__global__ void __launch_bounds__(XF_BLOCK) xf_vertices_kernel(const double* __restrict__ rest, const uint32_t* __restrict__ group, const double* __restrict__ table,
                                                               double* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * XF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double* p = rest + 3 * (size_t)i;
    const double x = p[0], y = p[1], z = p[2];
    const double* m = table + XF_RECORD * (size_t)group[i];
    double* o = out + 3 * (size_t)i;
#pragma unroll
    for (int a = 0; a < 3; a++) o[a] = ((m[4 * a] * x + m[4 * a + 1] * y) + m[4 * a + 2] * z) + m[4 * a + 3];
}

__global__ void __launch_bounds__(XF_BLOCK) xf_normals_kernel(const double* __restrict__ rest, const uint32_t* __restrict__ group, const double* __restrict__ table,
                                                              double* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * XF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double* p = rest + 3 * (size_t)i;
    const double x = p[0], y = p[1], z = p[2];
    const double* c = table + XF_RECORD * (size_t)group[i] + 12;
    double v[3];
#pragma unroll
    for (int a = 0; a < 3; a++) v[a] = (c[3 * a] * x + c[3 * a + 1] * y) + c[3 * a + 2] * z;
    const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const bool unit = len > 0.0 && len < INFINITY;                                  // (NaN fails both)
    double* o = out + 3 * (size_t)i;
#pragma unroll
    for (int a = 0; a < 3; a++) o[a] = unit ? v[a] / len : v[a];
}

inline dim3 xf_grid(uint32_t n) { return dim3((n + XF_BLOCK - 1) / XF_BLOCK); }

}  // namespace

hipError_t launch_xf_vertices(const double* rest, const uint32_t* group, const double* table, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(xf_vertices_kernel, xf_grid(n), dim3(XF_BLOCK), 0, stream, rest, group, table, out, n);
    return hipGetLastError();
}

hipError_t launch_xf_normals(const double* rest, const uint32_t* group, const double* table, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(xf_normals_kernel, xf_grid(n), dim3(XF_BLOCK), 0, stream, rest, group, table, out, n);
    return hipGetLastError();
}
