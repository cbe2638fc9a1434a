// gfx950 kernels of linear-blend skinning: mcpt_update_skin deforms a live scene by one 3x4 matrix per bone.  The skin's rest pose
// (vertices and normals as they were when mcpt_set_vertex_skin was called), four bone ids and four weights per vertex and per normal stay on the
// device; per call only the table of matrices crosses the bus.  The two kernels here write the context's CURRENT arrays (rf_vtx / rf_nrm) from the
// rest pose; the refit of refit.hip follows on the same stream, exactly as after mcpt_update_vertices' upload.
//
// Floating-point contraction is OFF in this file, as in transform.hip: every product, sum, difference, quotient and root below is one correctly
// rounded fp64 operation in a fixed association, so tests/skin_ref.py (numpy, the same association) gives the same arrays bit for bit.  All four
// influence slots are accumulated, a slot of weight 0 included: leaving one out would change the sign of a zero.  Plain C++ loads and vector
// stores only; the table is gathered from global memory, as transform.hip gathers its own.
#include "skin.h"
#include "transform.h"

#pragma clang fp contract(off)

double sk_bone_det(const double* m) {
    double rec[XF_RECORD];
    xf_group_record(m, rec);
    return xf_record_det(rec);
}

double sk_row_reach(const double* a, double radius) {
    const double slack = 1.0 + 0x1p-16;
    return slack * (((fabs(a[0]) + fabs(a[1])) + fabs(a[2])) * radius + fabs(a[3]));
}

namespace {

// A record's influences: the four bones' matrices in the table and their weights.  The ids come as one 16-byte load, the weights as two.
struct SkInfluences {
    const double *m0, *m1, *m2, *m3;
    double w0, w1, w2, w3;
    __device__ SkInfluences(const uint32_t* __restrict__ bone, const double* __restrict__ weight, const double* __restrict__ table, uint32_t i) {
        const uint4 b = reinterpret_cast<const uint4*>(bone)[i];
        const double2 wa = reinterpret_cast<const double2*>(weight)[2 * (size_t)i], wb = reinterpret_cast<const double2*>(weight)[2 * (size_t)i + 1];
        m0 = table + SK_RECORD * (size_t)b.x; m1 = table + SK_RECORD * (size_t)b.y; m2 = table + SK_RECORD * (size_t)b.z; m3 = table + SK_RECORD * (size_t)b.w;
        w0 = wa.x; w1 = wa.y; w2 = wb.x; w3 = wb.y;
    }
    __device__ double blend(int k) const { return ((w0 * m0[k] + w1 * m1[k]) + w2 * m2[k]) + w3 * m3[k]; }   // entry k of B
};

__global__ void __launch_bounds__(SK_BLOCK) sk_vertices_kernel(const double* __restrict__ rest, const uint32_t* __restrict__ bone, const double* __restrict__ weight,
                                                               const double* __restrict__ table, double* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * SK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double* p = rest + 3 * (size_t)i;
    const double x = p[0], y = p[1], z = p[2];
    const SkInfluences s(bone, weight, table, i);
    double* o = out + 3 * (size_t)i;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double b0 = s.blend(4 * a), b1 = s.blend(4 * a + 1), b2 = s.blend(4 * a + 2), b3 = s.blend(4 * a + 3);
        o[a] = ((b0 * x + b1 * y) + b2 * z) + b3;
    }
}

__global__ void __launch_bounds__(SK_BLOCK) sk_normals_kernel(const double* __restrict__ rest, const uint32_t* __restrict__ bone, const double* __restrict__ weight,
                                                              const double* __restrict__ table, double* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * SK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double* p = rest + 3 * (size_t)i;
    const double x = p[0], y = p[1], z = p[2];
    const SkInfluences s(bone, weight, table, i);
    const double a00 = s.blend(0), a01 = s.blend(1), a02 = s.blend(2), a10 = s.blend(4), a11 = s.blend(5), a12 = s.blend(6), a20 = s.blend(8), a21 = s.blend(9),
                 a22 = s.blend(10);
    // cof(A_B): xf_group_record's nine formulas
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double c10 = a02 * a21 - a01 * a22, c11 = a00 * a22 - a02 * a20, c12 = a01 * a20 - a00 * a21;
    const double c20 = a01 * a12 - a02 * a11, c21 = a02 * a10 - a00 * a12, c22 = a00 * a11 - a01 * a10;
    const double vx = (c00 * x + c01 * y) + c02 * z, vy = (c10 * x + c11 * y) + c12 * z, vz = (c20 * x + c21 * y) + c22 * z;
    const double len = sqrt((vx * vx + vy * vy) + vz * vz);
    const bool unit = len > 0.0 && len < INFINITY;                                  // (NaN fails both)
    double* o = out + 3 * (size_t)i;
    o[0] = unit ? vx / len : vx; o[1] = unit ? vy / len : vy; o[2] = unit ? vz / len : vz;
}

inline dim3 sk_grid(uint32_t n) { return dim3((n + SK_BLOCK - 1) / SK_BLOCK); }

}  // namespace

hipError_t launch_sk_vertices(const double* rest, const uint32_t* bone, const double* weight, const double* table, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sk_vertices_kernel, sk_grid(n), dim3(SK_BLOCK), 0, stream, rest, bone, weight, table, out, n);
    return hipGetLastError();
}

hipError_t launch_sk_normals(const double* rest, const uint32_t* bone, const double* weight, const double* table, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sk_normals_kernel, sk_grid(n), dim3(SK_BLOCK), 0, stream, rest, bone, weight, table, out, n);
    return hipGetLastError();
}
