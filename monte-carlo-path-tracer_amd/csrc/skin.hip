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

// ---- dual-quaternion mode: the host half.  Every expression below is restated by tests/skin_dq_ref.py in the same association.
void sk_bone_gram(const double* m, double* g) {
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    g[0] = (a00 * a00 + a10 * a10) + a20 * a20; g[1] = (a00 * a01 + a10 * a11) + a20 * a21; g[2] = (a00 * a02 + a10 * a12) + a20 * a22;
    g[3] = (a01 * a01 + a11 * a11) + a21 * a21; g[4] = (a01 * a02 + a11 * a12) + a21 * a22; g[5] = (a02 * a02 + a12 * a12) + a22 * a22;
}

bool sk_bone_rigid(const double* m) {
    if (!(sk_bone_det(m) > 0.0)) return false;
    double g[6];
    sk_bone_gram(m, g);
    const double one[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
    for (int k = 0; k < 6; k++)
        if (!(fabs(g[k] - one[k]) <= SK_DQ_RIGID_TOLERANCE)) return false;
    return true;
}

double sk_dq_reach(const double* m, double radius) {
    const double slack = 1.0 + 0x1p-16;
    return slack * (2.0 * radius + 16.0 * ((fabs(m[3]) + fabs(m[7])) + fabs(m[11])));
}

void sk_bone_dualquat(const double* m, double* out) {
    const double a00 = m[0], a01 = m[1], a02 = m[2], tx = m[3], a10 = m[4], a11 = m[5], a12 = m[6], ty = m[7], a20 = m[8], a21 = m[9], a22 = m[10], tz = m[11];
    const double tr = (a00 + a11) + a22;
    int pick = 0; double best = tr;                                                 // Shepperd: the largest of {tr, a00, a11, a22}, the first wins a tie
    if (a00 > best) { pick = 1; best = a00; }
    if (a11 > best) { pick = 2; best = a11; }
    if (a22 > best) { pick = 3; best = a22; }
    double w, x, y, z;
    if (pick == 0) {
        const double s = 2.0 * sqrt(1.0 + tr);
        w = 0.25 * s; x = (a21 - a12) / s; y = (a02 - a20) / s; z = (a10 - a01) / s;
    } else if (pick == 1) {
        const double s = 2.0 * sqrt(1.0 + ((a00 - a11) - a22));
        w = (a21 - a12) / s; x = 0.25 * s; y = (a01 + a10) / s; z = (a02 + a20) / s;
    } else if (pick == 2) {
        const double s = 2.0 * sqrt(1.0 + ((a11 - a00) - a22));
        w = (a02 - a20) / s; x = (a01 + a10) / s; y = 0.25 * s; z = (a12 + a21) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + ((a22 - a00) - a11));
        w = (a10 - a01) / s; x = (a02 + a20) / s; y = (a12 + a21) / s; z = 0.25 * s;
    }
    const double len = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / len; x = x / len; y = y / len; z = z / len;
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    out[0] = w; out[1] = x; out[2] = y; out[3] = z;                                  // the dual part: 1/2 (0, t) q
    out[4] = -0.5 * ((tx * x + ty * y) + tz * z);
    out[5] = 0.5 * ((w * tx + ty * z) - tz * y);
    out[6] = 0.5 * ((w * ty + tz * x) - tx * z);
    out[7] = 0.5 * ((w * tz + tx * y) - ty * x);
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

// ---- dual-quaternion mode.  A bone of the table: {w, x, y, z, dw, dx, dy, dz}, 64 bytes, read as 16-byte loads.
struct SkQuat { double w, x, y, z; };
__device__ inline SkQuat sk_dq_load(const double* __restrict__ table, uint32_t bone, int half) {
    const double2* q = reinterpret_cast<const double2*>(table) + 4 * (size_t)bone + 2 * half;
    const double2 a = q[0], b = q[1];
    return SkQuat{a.x, a.y, b.x, b.y};
}
__device__ inline double sk_dq_dot(const SkQuat& a, const SkQuat& b) { return ((a.w * b.w + a.x * b.x) + a.y * b.y) + a.z * b.z; }
__device__ inline SkQuat sk_dq_blend(double w0, const SkQuat& a, double w1, const SkQuat& b, double w2, const SkQuat& c, double w3, const SkQuat& d) {
    return SkQuat{((w0 * a.w + w1 * b.w) + w2 * c.w) + w3 * d.w, ((w0 * a.x + w1 * b.x) + w2 * c.x) + w3 * d.x, ((w0 * a.y + w1 * b.y) + w2 * c.y) + w3 * d.y,
                  ((w0 * a.z + w1 * b.z) + w2 * c.z) + w3 * d.z};
}
__device__ inline SkQuat sk_dq_over(const SkQuat& q, double n) { return SkQuat{q.w / n, q.x / n, q.y / n, q.z / n}; }

// A record's influences in dual-quaternion mode: the ids as one 16-byte load, the weights as two; slot 0 is the pivot, and a slot whose rotation
// lies in the other hemisphere from the pivot's enters with its weight negated (q and -q are the same rotation: blend the short way round).
struct SkDqInfluences {
    uint4 b;
    double w0, w1, w2, w3;                                                          // w1 .. w3 carry their sign
    SkQuat q0, q1, q2, q3;                                                          // the real parts
    __device__ SkDqInfluences(const uint32_t* __restrict__ bone, const double* __restrict__ weight, const double* __restrict__ table, uint32_t i) {
        b = reinterpret_cast<const uint4*>(bone)[i];
        const double2 wa = reinterpret_cast<const double2*>(weight)[2 * (size_t)i], wb = reinterpret_cast<const double2*>(weight)[2 * (size_t)i + 1];
        q0 = sk_dq_load(table, b.x, 0); q1 = sk_dq_load(table, b.y, 0); q2 = sk_dq_load(table, b.z, 0); q3 = sk_dq_load(table, b.w, 0);
        w0 = wa.x;
        w1 = wa.y * (sk_dq_dot(q0, q1) < 0.0 ? -1.0 : 1.0);
        w2 = wb.x * (sk_dq_dot(q0, q2) < 0.0 ? -1.0 : 1.0);
        w3 = wb.y * (sk_dq_dot(q0, q3) < 0.0 ? -1.0 : 1.0);
    }
    __device__ SkQuat real() const { return sk_dq_blend(w0, q0, w1, q1, w2, q2, w3, q3); }
    __device__ SkQuat dual(const double* __restrict__ table) const {
        return sk_dq_blend(w0, sk_dq_load(table, b.x, 1), w1, sk_dq_load(table, b.y, 1), w2, sk_dq_load(table, b.z, 1), w3, sk_dq_load(table, b.w, 1));
    }
};
__device__ inline double sk_dq_norm2(const SkQuat& q) { return ((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z; }
__device__ inline bool sk_dq_regular(double n2) { return n2 >= SK_DQ_MIN_NORM2 && n2 < INFINITY; }   // (NaN fails both)

// The rotation matrix of a unit quaternion, row-major: the usual nine formulas.
struct SkRot { double m[9]; };
__device__ inline SkRot sk_dq_rotation(const SkQuat& r) {
    const double w = r.w, x = r.x, y = r.y, z = r.z;
    return SkRot{{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                  2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                  2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
}

__global__ void __launch_bounds__(SK_BLOCK) sk_dq_vertices_kernel(const double* __restrict__ rest, const uint32_t* __restrict__ bone, const double* __restrict__ weight,
                                                                  const double* __restrict__ table, double* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * SK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double* p = rest + 3 * (size_t)i;
    const double x = p[0], y = p[1], z = p[2];
    const SkDqInfluences s(bone, weight, table, i);
    const SkQuat br = s.real();
    const double n2 = sk_dq_norm2(br);
    double* o = out + 3 * (size_t)i;
    if (!sk_dq_regular(n2)) { o[0] = x; o[1] = y; o[2] = z; return; }                // a degenerate blend: the rest pose's record
    const SkQuat bd = s.dual(table);
    const double len = sqrt(n2);
    const SkQuat r = sk_dq_over(br, len), d = sk_dq_over(bd, len);
    const SkRot R = sk_dq_rotation(r);
    const double tx = 2.0 * (((r.w * d.x - d.w * r.x) + r.y * d.z) - r.z * d.y);     // t = 2 (r.w d_v - d.w r_v + r_v x d_v)
    const double ty = 2.0 * (((r.w * d.y - d.w * r.y) + r.z * d.x) - r.x * d.z);
    const double tz = 2.0 * (((r.w * d.z - d.w * r.z) + r.x * d.y) - r.y * d.x);
    o[0] = ((R.m[0] * x + R.m[1] * y) + R.m[2] * z) + tx;
    o[1] = ((R.m[3] * x + R.m[4] * y) + R.m[5] * z) + ty;
    o[2] = ((R.m[6] * x + R.m[7] * y) + R.m[8] * z) + tz;
}

__global__ void __launch_bounds__(SK_BLOCK) sk_dq_normals_kernel(const double* __restrict__ rest, const uint32_t* __restrict__ bone, const double* __restrict__ weight,
                                                                 const double* __restrict__ table, double* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * SK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double* p = rest + 3 * (size_t)i;
    const double x = p[0], y = p[1], z = p[2];
    const SkDqInfluences s(bone, weight, table, i);
    const SkQuat br = s.real();
    const double n2 = sk_dq_norm2(br);
    double* o = out + 3 * (size_t)i;
    if (!sk_dq_regular(n2)) { o[0] = x; o[1] = y; o[2] = z; return; }                // copied, NOT normalised
    const SkRot R = sk_dq_rotation(sk_dq_over(br, sqrt(n2)));
    const double vx = (R.m[0] * x + R.m[1] * y) + R.m[2] * z, vy = (R.m[3] * x + R.m[4] * y) + R.m[5] * z, vz = (R.m[6] * x + R.m[7] * y) + R.m[8] * z;
    const double len = sqrt((vx * vx + vy * vy) + vz * vz);
    const bool unit = len > 0.0 && len < INFINITY;                                  // (NaN fails both)
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

hipError_t launch_sk_dq_vertices(const double* rest, const uint32_t* bone, const double* weight, const double* table, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sk_dq_vertices_kernel, sk_grid(n), dim3(SK_BLOCK), 0, stream, rest, bone, weight, table, out, n);
    return hipGetLastError();
}

hipError_t launch_sk_dq_normals(const double* rest, const uint32_t* bone, const double* weight, const double* table, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sk_dq_normals_kernel, sk_grid(n), dim3(SK_BLOCK), 0, stream, rest, bone, weight, table, out, n);
    return hipGetLastError();
}
