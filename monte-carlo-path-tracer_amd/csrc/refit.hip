// gfx950 kernels of the scene update: mcpt_update_vertices moves the vertices of a live scene -- same faces, same materials --
// and pays for a REFIT of the two trees instead of a rebuild.  Topology, leaf order, octant slots and every link stay as mcpt_create made
// them; only coordinates change: the triangle streams, the light records, the binary tree's child boxes, the 8-wide tree's frames and
// quantised planes.  Closest hit and any hit do not depend on the tree, so a refitted context traces what a fresh mcpt_create of the moved
// scene traces; a large deformation makes traversal slower, never wrong.
//
// Everything runs on the context's stream, ordered like a render call.  The trees are refitted bottom-up with ONE LAUNCH PER LEVEL (binary
// tree: by node height; 8-wide tree: by depth, deepest first -- its breadth-first numbering makes a level one contiguous record range): a
// level reads only what earlier launches wrote, so no block ever waits for, or reads the fresh stores of, another block of its own launch.
//
// Floating-point contraction is OFF in this file (the library is built with -ffp-contract=fast): rf_triangles_kernel and rf_lights_kernel
// restate build_host_scene's arithmetic, operation for operation, and the host's x86 code does not fuse -- an update with the creation
// vertices reproduces the created streams bit for bit.  Plain C++ loads and vector stores only.
#include "refit.h"

#pragma clang fp contract(off)

namespace {

// scene_build.cpp: round_down / round_up without the pad
__device__ __forceinline__ float rf_down(double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; }
__device__ __forceinline__ float rf_up(double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; }

struct RfBox { float lo[3], hi[3]; };
__device__ __forceinline__ RfBox rf_load_box(const float* __restrict__ boxes, size_t i) {
    const float2* p = reinterpret_cast<const float2*>(boxes + 6 * i);          // 24-B records: 8-B aligned
    const float2 a = p[0], b = p[1], c = p[2];
    return RfBox{{a.x, a.y, b.x}, {b.y, c.x, c.y}};
}
__device__ __forceinline__ void rf_store_box(float* __restrict__ boxes, size_t i, const RfBox& b) {
    float2* p = reinterpret_cast<float2*>(boxes + 6 * i);
    p[0] = make_float2(b.lo[0], b.lo[1]); p[1] = make_float2(b.lo[2], b.hi[0]); p[2] = make_float2(b.hi[1], b.hi[2]);
}
__device__ __forceinline__ void rf_grow(RfBox& a, const RfBox& b) {
    for (int x = 0; x < 3; x++) { a.lo[x] = fminf(a.lo[x], b.lo[x]); a.hi[x] = fmaxf(a.hi[x], b.hi[x]); }
}
// The box of a leaf child: the bound of its triangles, padded by write_node's rule (scene_build.cpp): max |coordinate| * 1e-6 + 1e-30
__device__ __forceinline__ RfBox rf_leaf_box(const float* __restrict__ tri_box, uint32_t first, uint32_t cnt) {
    RfBox b = rf_load_box(tri_box, first);
    for (uint32_t t = 1; t < cnt; t++) rf_grow(b, rf_load_box(tri_box, (size_t)first + t));
    float m = 0.f;
    for (int x = 0; x < 3; x++) m = fmaxf(m, fmaxf(fabsf(b.lo[x]), fabsf(b.hi[x])));
    const float pad = (float)((double)m * 1e-6 + 1e-30);
    for (int x = 0; x < 3; x++) { b.lo[x] -= pad; b.hi[x] += pad; }
    return b;
}

// ---------------------------------------------------------------------------------------------- triangle streams
// The statements of build_host_scene's stream loop (scene_build.cpp) for one triangle, in its order.
__global__ void __launch_bounds__(RF_BLOCK) rf_triangles_kernel(const double* __restrict__ vertex, const double* __restrict__ normal, const int32_t* __restrict__ idx6,
                                                                RfCentre ctr, float4* __restrict__ tri_isect, float4* __restrict__ tri_shade,
                                                                double* __restrict__ tri_pos64, float* __restrict__ tri_box, uint32_t n_tris) {
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= n_tris) return;
    const int2* ip = reinterpret_cast<const int2*>(idx6 + 6 * (size_t)i);
    const int2 i01 = ip[0], i2n = ip[1], n12 = ip[2];
    const double* w0 = vertex + 3 * (size_t)i01.x; const double* w1 = vertex + 3 * (size_t)i01.y; const double* w2 = vertex + 3 * (size_t)i2n.x;
    const double c[3] = {ctr.x, ctr.y, ctr.z};
    double W0[3], W1[3], W2[3], v0[3], v1[3], v2[3];
    for (int a = 0; a < 3; a++) { W0[a] = w0[a]; W1[a] = w1[a]; W2[a] = w2[a]; v0[a] = W0[a] - c[a]; v1[a] = W1[a] - c[a]; v2[a] = W2[a] - c[a]; }
    float4* I = tri_isect + 3 * (size_t)i;
    const float keep = I[0].w;                                                         // lobe class | tie rank: creation's
    I[0] = make_float4((float)v0[0], (float)v0[1], (float)v0[2], keep);
    I[1] = make_float4((float)(W1[0] - W0[0]), (float)(W1[1] - W0[1]), (float)(W1[2] - W0[2]), 0.f);   // (edges from the world coordinates)
    I[2] = make_float4((float)(W2[0] - W0[0]), (float)(W2[1] - W0[1]), (float)(W2[2] - W0[2]), 0.f);
    float4* S = tri_shade + (size_t)MCPT_TRI_SHADE_F4 * i;
    if (normal) {
        const double* n0 = normal + 3 * (size_t)i2n.y; const double* n1 = normal + 3 * (size_t)n12.x; const double* n2 = normal + 3 * (size_t)n12.y;
        const float4 s0 = S[0], s1 = S[1], s2 = S[2];                                  // .w: texture coordinates, kept
        S[0] = make_float4((float)n0[0], (float)n0[1], (float)n0[2], s0.w);
        S[1] = make_float4((float)n1[0], (float)n1[1], (float)n1[2], s1.w);
        S[2] = make_float4((float)n2[0], (float)n2[1], (float)n2[2], s2.w);
    }
    double* P = tri_pos64 + 9 * (size_t)i;
    for (int a = 0; a < 3; a++) { P[a] = v0[a]; P[3 + a] = v1[a]; P[6 + a] = v2[a]; }
    {
        const double ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2], bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
        const double nx = ay * bz - by * az, ny = az * bx - bz * ax, nz = ax * by - bx * ay;
        const double d = nx * v0[0] + ny * v0[1] + nz * v0[2];
        double2* pl = reinterpret_cast<double2*>(S + 4);                               // the fp64 plane: second half of the record
        pl[0] = make_double2(nx, ny); pl[1] = make_double2(nz, d);
    }
    RfBox b;
    for (int a = 0; a < 3; a++) { b.lo[a] = rf_down(fmin(v0[a], fmin(v1[a], v2[a]))); b.hi[a] = rf_up(fmax(v0[a], fmax(v1[a], v2[a]))); }
    rf_store_box(tri_box, i, b);
}

// ---------------------------------------------------------------------------------------------- lights
__global__ void __launch_bounds__(RF_BLOCK) rf_lights_kernel(DevLight* __restrict__ lights, double* __restrict__ light_pos64, const float4* __restrict__ tri_isect,
                                                             const double* __restrict__ tri_pos64, const double* __restrict__ normal, const int32_t* __restrict__ idx6,
                                                             uint32_t n_lights) {
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= n_lights) return;
    float4* R = reinterpret_cast<float4*>(lights + i);                                 // 64 B: tri area rad.xy | rad.z n0.xyz | n1.xyz n2.x | n2.yz pad pad
    float4 r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3];
    const uint32_t tri = (uint32_t)__float_as_int(r0.x);
    const float4 e1 = tri_isect[3 * (size_t)tri + 1], e2 = tri_isect[3 * (size_t)tri + 2];
    const float cx = e1.y * e2.z - e2.y * e1.z, cy = e1.z * e2.x - e2.z * e1.x, cz = e1.x * e2.y - e2.x * e1.y;
    r0.y = 0.5f * (float)sqrt((double)((cx * cx + cy * cy) + cz * cz));                // (fp64 root rounded once = the correctly rounded fp32 root of std::sqrt)
    if (normal) {
        const int32_t* ix = idx6 + 6 * (size_t)tri + 3;
        const double* n0 = normal + 3 * (size_t)ix[0]; const double* n1 = normal + 3 * (size_t)ix[1]; const double* n2 = normal + 3 * (size_t)ix[2];
        r1.y = (float)n0[0]; r1.z = (float)n0[1]; r1.w = (float)n0[2];
        r2.x = (float)n1[0]; r2.y = (float)n1[1]; r2.z = (float)n1[2];
        r2.w = (float)n2[0]; r3.x = (float)n2[1]; r3.y = (float)n2[2];
    }
    R[0] = r0; R[1] = r1; R[2] = r2; R[3] = r3;
    for (int a = 0; a < 9; a++) light_pos64[9 * (size_t)i + a] = tri_pos64[9 * (size_t)tri + a];
}

// ---------------------------------------------------------------------------------------------- binary tree
// A leaf child's box: the padded bound of its triangles.  An inner child's box: the union of that child's own two child boxes (refitted by an
// earlier launch).  The empty second child of a one-leaf scene keeps its box.  Links untouched.
__global__ void __launch_bounds__(RF_BLOCK) rf_binary_kernel(float4* __restrict__ nodes, const uint32_t* __restrict__ order, uint32_t begin, uint32_t end,
                                                             const float* __restrict__ tri_box) {
    const uint32_t k = begin + blockIdx.x * RF_BLOCK + threadIdx.x;
    if (k >= end) return;
    float4* N = nodes + 4 * (size_t)order[k];
    const float4 a0 = N[0], a1 = N[1], az = N[2], links = N[3];
    RfBox b[2] = {{{a0.x, a0.z, az.x}, {a0.y, a0.w, az.y}}, {{a1.x, a1.z, az.z}, {a1.y, a1.w, az.w}}};
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int code = __float_as_int(c == 0 ? links.x : links.y);
        if (code >= 0) {
            const float4* C = nodes + 4 * (size_t)code;
            const float4 c0 = C[0], c1 = C[1], cz = C[2];
            b[c] = RfBox{{fminf(c0.x, c1.x), fminf(c0.z, c1.z), fminf(cz.x, cz.z)}, {fmaxf(c0.y, c1.y), fmaxf(c0.w, c1.w), fmaxf(cz.y, cz.w)}};
        } else {
            const uint32_t leaf = (uint32_t)~code, cnt = leaf & 7u;
            if (cnt) b[c] = rf_leaf_box(tri_box, leaf >> 3, cnt);
        }
    }
    N[0] = make_float4(b[0].lo[0], b[0].hi[0], b[0].lo[1], b[0].hi[1]);
    N[1] = make_float4(b[1].lo[0], b[1].hi[0], b[1].lo[1], b[1].hi[1]);
    N[2] = make_float4(b[0].lo[2], b[0].hi[2], b[1].lo[2], b[1].hi[2]);
}

// ---------------------------------------------------------------------------------------------- 8-wide tree
// One lane per record.  The exact fp32 boxes of the children in their slots (leaf child: rf_leaf_box; inner child: node_box of its record),
// their union into node_box, then the frame and the planes.  The quantisation is build_bvh8's rule (scene_build.cpp) RESTATED here, not shared
// with it: the host function and c8_emit_kernel (bvh_gpu.hip) must keep producing the bits wide_tree_hash pins, and neither is touched.
// child_base, tri_base, imask, p0, p1 and the slot of every child stay.
__global__ void __launch_bounds__(RF_BLOCK) rf_wide_kernel(float4* __restrict__ nodes8, uint32_t begin, uint32_t end, const float* __restrict__ tri_box,
                                                           float* __restrict__ node_box) {
    const uint32_t rec = begin + blockIdx.x * RF_BLOCK + threadIdx.x;
    if (rec >= end) return;
    float4* r = nodes8 + 5 * (size_t)rec;
    const float4 r1 = r[1];
    const uint32_t child_base = __float_as_uint(r1.x), tri_base = __float_as_uint(r1.y), masks = __float_as_uint(r1.w);
    const uint32_t imask = masks & 0xffu, p0 = (masks >> 8) & 0xffu, p1 = (masks >> 16) & 0xffu, occupied = imask | p0 | p1;
    float klo[8][3], khi[8][3];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int sl = 0; sl < 8; sl++) {
        RfBox b{{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
        if ((occupied >> sl) & 1u) {
            const uint32_t below = (1u << sl) - 1u;
            if ((imask >> sl) & 1u) b = rf_load_box(node_box, (size_t)child_base + __popc(imask & below));
            else b = rf_leaf_box(tri_box, tri_base + __popc(p0 & below) + 2u * __popc(p1 & below), ((p0 >> sl) & 1u) + 2u * ((p1 >> sl) & 1u));
            for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], b.lo[a]); hi[a] = fmaxf(hi[a], b.hi[a]); }
        }
        for (int a = 0; a < 3; a++) { klo[sl][a] = b.lo[a]; khi[sl][a] = b.hi[a]; }
    }
    if (!occupied) for (int a = 0; a < 3; a++) lo[a] = hi[a] = 0.f;
    rf_store_box(node_box, rec, RfBox{{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}});
    // the frame: a power-of-two step and a stored origin 1024 + 2 margins steps below the lowest child bound, rounded down to fp32 FIRST
    int ebits[3]; double scale[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double ext = (double)hi[a] - (double)lo[a];
        int e = ext > 0 ? (int)ceil(log2(ext / 255.0)) : -100;
        e = e < -126 ? -126 : (e > 127 ? 127 : e);
        float org = lo[a];
        for (;; e++) {
            const double sc = ldexp(1.0, e), of = (double)lo[a] - (1024.0 + 2.0 * MCPT_Q_MARGIN) * sc;
            org = (float)of; if ((double)org > of) org = nextafterf(org, -INFINITY);
            if (!(ext > 0) || e >= 127 || ((double)hi[a] - (double)org) / sc - 1024.0 + MCPT_Q_MARGIN <= 255.0) break;
        }
        lo[a] = org; ebits[a] = e; scale[a] = ldexp(1.0, e);
    }
    // planes floored / ceiled with the margin against the ROUNDED origin; empty slots keep an inverted box
    uint32_t q[3][4];
#pragma unroll
    for (int a = 0; a < 3; a++) for (int j = 0; j < 4; j++) q[a][j] = MCPT_N8_EMPTY_WORD;
#pragma unroll
    for (int sl = 0; sl < 8; sl++) {
        if (!((occupied >> sl) & 1u)) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            double ql = floor(((double)klo[sl][a] - (double)lo[a]) / scale[a] - 1024.0 - MCPT_Q_MARGIN);
            double qh = ceil(((double)khi[sl][a] - (double)lo[a]) / scale[a] - 1024.0 + MCPT_Q_MARGIN);
            ql = fmin(255.0, fmax(0.0, ql)); qh = fmin(255.0, fmax(0.0, qh));
            q[a][MCPT_N8_WORD(sl)] = (q[a][MCPT_N8_WORD(sl)] & ~(0xffu << MCPT_N8_LO_SHIFT(sl)) & ~(0xffu << MCPT_N8_HI_SHIFT(sl))) |
                                     ((uint32_t)ql << MCPT_N8_LO_SHIFT(sl)) | ((uint32_t)qh << MCPT_N8_HI_SHIFT(sl));
        }
    }
    auto bf16 = [](int e) { return (uint32_t)(e + 127) << 7; };
    r[0] = make_float4(lo[0], lo[1], lo[2], __uint_as_float((bf16(ebits[0]) << 16) | bf16(ebits[1])));
    r[1] = make_float4(r1.x, r1.y, __uint_as_float(bf16(ebits[2]) << 16), r1.w);
    r[2] = make_float4(__uint_as_float(q[0][0]), __uint_as_float(q[0][1]), __uint_as_float(q[0][2]), __uint_as_float(q[0][3]));
    r[3] = make_float4(__uint_as_float(q[1][0]), __uint_as_float(q[1][1]), __uint_as_float(q[1][2]), __uint_as_float(q[1][3]));
    r[4] = make_float4(__uint_as_float(q[2][0]), __uint_as_float(q[2][1]), __uint_as_float(q[2][2]), __uint_as_float(q[2][3]));
}

// ---------------------------------------------------------------------------------------------- wide_area_ratio
// Per record the surface areas of its occupied slots' boxes, dequantised the way validate_bvh8 does (origin + (1024 + q) * step), summed in
// fp64; one partial sum per block, in a fixed order -- the host adds the partials, so the figure is reproducible.
__global__ void __launch_bounds__(RF_BLOCK) rf_wide_area_kernel(const float4* __restrict__ nodes8, uint32_t n, double* __restrict__ partial) {
    __shared__ double s_sum[RF_BLOCK / 64];
    const uint32_t rec = blockIdx.x * RF_BLOCK + threadIdx.x;
    double area = 0.0;
    if (rec < n) {
        const float4* r = nodes8 + 5 * (size_t)rec;
        const float4 r0 = r[0], r1 = r[1];
        const uint32_t sxy = __float_as_uint(r0.w), szw = __float_as_uint(r1.z), masks = __float_as_uint(r1.w);
        const float sc[3] = {__uint_as_float(sxy & 0xffff0000u), __uint_as_float(sxy << 16), __uint_as_float(szw & 0xffff0000u)};
        const float org[3] = {r0.x, r0.y, r0.z};
        const uint32_t occupied = (masks | (masks >> 8) | (masks >> 16)) & 0xffu;
        const float4 Q[3] = {r[2], r[3], r[4]};
#pragma unroll
        for (int sl = 0; sl < 8; sl++) {
            if (!((occupied >> sl) & 1u)) continue;
            double ext[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int j = MCPT_N8_WORD(sl);
                const uint32_t word = __float_as_uint(j == 0 ? Q[a].x : j == 1 ? Q[a].y : j == 2 ? Q[a].z : Q[a].w);
                const float qlo = (float)((word >> MCPT_N8_LO_SHIFT(sl)) & 0xffu), qhi = (float)((word >> MCPT_N8_HI_SHIFT(sl)) & 0xffu);
                ext[a] = (double)(org[a] + (1024.0f + qhi) * sc[a]) - (double)(org[a] + (1024.0f + qlo) * sc[a]);
            }
            area += 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]);
        }
    }
    for (int m = 32; m >= 1; m >>= 1) area += __shfl_xor(area, m, 64);
    if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = area;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0.0; for (int w = 0; w < RF_BLOCK / 64; w++) t += s_sum[w]; partial[blockIdx.x] = t; }
}

inline dim3 rf_grid(uint32_t n) { return dim3((n + RF_BLOCK - 1) / RF_BLOCK); }

}  // namespace

hipError_t launch_rf_triangles(const double* vertex, const double* normal, const int32_t* idx6, RfCentre centre, float4* tri_isect, float4* tri_shade,
                               double* tri_pos64, float* tri_box, uint32_t n_tris, hipStream_t stream) {
    if (n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(rf_triangles_kernel, rf_grid(n_tris), dim3(RF_BLOCK), 0, stream, vertex, normal, idx6, centre, tri_isect, tri_shade, tri_pos64, tri_box, n_tris);
    return hipGetLastError();
}

hipError_t launch_rf_lights(DevLight* lights, double* light_pos64, const float4* tri_isect, const double* tri_pos64, const double* normal,
                            const int32_t* idx6, uint32_t n_lights, hipStream_t stream) {
    if (n_lights == 0) return hipSuccess;
    hipLaunchKernelGGL(rf_lights_kernel, rf_grid(n_lights), dim3(RF_BLOCK), 0, stream, lights, light_pos64, tri_isect, tri_pos64, normal, idx6, n_lights);
    return hipGetLastError();
}

hipError_t launch_rf_binary_level(float4* nodes, const uint32_t* order, uint32_t begin, uint32_t end, const float* tri_box, hipStream_t stream) {
    if (end <= begin) return hipSuccess;
    hipLaunchKernelGGL(rf_binary_kernel, rf_grid(end - begin), dim3(RF_BLOCK), 0, stream, nodes, order, begin, end, tri_box);
    return hipGetLastError();
}

hipError_t launch_rf_wide_level(float4* nodes8, uint32_t begin, uint32_t end, const float* tri_box, float* node_box, hipStream_t stream) {
    if (end <= begin) return hipSuccess;
    hipLaunchKernelGGL(rf_wide_kernel, rf_grid(end - begin), dim3(RF_BLOCK), 0, stream, nodes8, begin, end, tri_box, node_box);
    return hipGetLastError();
}

hipError_t launch_rf_wide_area(const float4* nodes8, uint32_t n_nodes8, double* partial, hipStream_t stream) {
    if (n_nodes8 == 0) return hipSuccess;
    hipLaunchKernelGGL(rf_wide_area_kernel, rf_grid(n_nodes8), dim3(RF_BLOCK), 0, stream, nodes8, n_nodes8, partial);
    return hipGetLastError();
}
