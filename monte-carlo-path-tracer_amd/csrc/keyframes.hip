// gfx950 kernels of keyframe playback: mcpt_update_keyframes deforms a live scene by ONE number, the time.  The frames -- whole
// vertex arrays and, optionally, normal arrays, uniformly spaced in time -- stay on the device; per call the host turns the time into a segment,
// 2 or 4 tap indices and as many weights, and those travel as kernel arguments: nothing is staged, nothing is copied from the host.  The two
// kernels here write the context's CURRENT arrays (rf_vtx / rf_nrm) and the refit of refit.hip follows on the same stream, exactly as after
// mcpt_update_vertices' upload.
//
// Both are memory-bound streams: 8 B x (taps + 1) per double, no LDS, no atomics.  The blend is component-wise, so the vertex kernel sees the
// frames as flat arrays of doubles and moves two per lane and step.  Floating-point contraction is OFF in this file, as in morph.hip: every
// product, sum, quotient and root below is one correctly rounded fp64 operation, so tests/keyframes_ref.py (numpy, the same order) gives the same
// arrays bit for bit.  Plain C++ loads and vector stores only.
#include "keyframes.h"
#include <math.h>

#pragma clang fp contract(off)

KfBlend kf_segment(double time, double start_time, double frame_time, uint32_t n_frames, uint32_t interpolation, uint32_t wrap) {
    const double K = double(n_frames);
    double x = (time - start_time) / frame_time;
    if (wrap == 0) {                                                         // clamp: outside the range the end frames themselves
        if (x <= 0.0) x = 0.0;
        else if (x >= K - 1.0) x = K - 1.0;
    } else {                                                                 // loop: frame K - 1 blends into frame 0
        x = fmod(x, K);
        if (x < 0.0) x = x + K;
        if (!(x < K)) x = 0.0;                                               // (x + K rounded up to K; fmod of an infinite x)
    }
    KfBlend b{};
    b.k = uint32_t(floor(x)); b.u = x - double(b.k);                         // (k is an integer: fmod's -0.0 gives k = 0 and u = -0.0, which is == 0)
    b.taps = interpolation == 0 ? 2u : 4u;
    const int64_t first = int64_t(b.k) - (interpolation == 0 ? 0 : 1), n = int64_t(n_frames);
    for (uint32_t t = 0; t < b.taps; t++) {
        const int64_t i = first + int64_t(t);
        b.tap[t] = uint32_t(wrap == 0 ? (i < 0 ? 0 : i > n - 1 ? n - 1 : i) : (i + n) % n);
    }
    return b;
}

void kf_weights(double u, uint32_t interpolation, double w[4]) {
    if (interpolation == 0) { w[0] = 1.0 - u; w[1] = u; w[2] = 0.0; w[3] = 0.0; return; }
    const double u2 = u * u, u3 = u2 * u;
    w[0] = 0.5 * ((2.0 * u2 - u3) - u);
    w[1] = 0.5 * ((3.0 * u3 - 5.0 * u2) + 2.0);
    w[2] = 0.5 * ((4.0 * u2 - 3.0 * u3) + u);
    w[3] = 0.5 * (u3 - u2);
}

double kf_reach(double radius, uint32_t interpolation) {
    const double slack = 1.0 + 0x1p-16, c = interpolation == 0 ? 1.0 : 1.25;
    return slack * (c * radius);
}

namespace {

// The blend of component i of the tapped frames f0 .. f3; T: double, or double2 for two neighbouring components at once.
template <int TAPS, class T> __device__ inline T kf_mix(const KfBlend& b, const T* __restrict__ f0, const T* __restrict__ f1, const T* __restrict__ f2,
                                                        const T* __restrict__ f3, size_t i) {
    T s = b.w[0] * f0[i] + b.w[1] * f1[i];
    if (TAPS == 4) { s = s + b.w[2] * f2[i]; s = s + b.w[3] * f3[i]; }
    return s;
}
// Where tapped frame t starts (a tap beyond TAPS: frame tap[0], never read).
template <int TAPS> __device__ inline const double* kf_tap(const double* __restrict__ frames, size_t stride, const KfBlend& b, int t) {
    return frames + stride * b.tap[t < TAPS ? t : 0];
}

template <int TAPS> __global__ void __launch_bounds__(KF_BLOCK) kf_vertices_kernel(const double* __restrict__ frames, size_t stride, KfBlend b, double* __restrict__ out,
                                                                                  size_t total) {
    const double *f0 = kf_tap<TAPS>(frames, stride, b, 0), *f1 = kf_tap<TAPS>(frames, stride, b, 1), *f2 = kf_tap<TAPS>(frames, stride, b, 2),
                 *f3 = kf_tap<TAPS>(frames, stride, b, 3);
    const double2 *p0 = reinterpret_cast<const double2*>(f0), *p1 = reinterpret_cast<const double2*>(f1), *p2 = reinterpret_cast<const double2*>(f2),
                  *p3 = reinterpret_cast<const double2*>(f3);
    double2* o2 = reinterpret_cast<double2*>(out);
    const size_t pairs = total / 2, step = size_t(gridDim.x) * KF_BLOCK;
    for (size_t i = size_t(blockIdx.x) * KF_BLOCK + threadIdx.x; i < pairs; i += step) o2[i] = kf_mix<TAPS>(b, p0, p1, p2, p3, i);
    if ((total & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[total - 1] = kf_mix<TAPS>(b, f0, f1, f2, f3, total - 1);   // 3 n is odd: the last double alone
}

template <int TAPS> __global__ void __launch_bounds__(KF_BLOCK) kf_normals_kernel(const double* __restrict__ frames, size_t stride, KfBlend b, double* __restrict__ out,
                                                                                 uint32_t n) {
    const uint32_t i = blockIdx.x * KF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double *f0 = kf_tap<TAPS>(frames, stride, b, 0), *f1 = kf_tap<TAPS>(frames, stride, b, 1), *f2 = kf_tap<TAPS>(frames, stride, b, 2),
                 *f3 = kf_tap<TAPS>(frames, stride, b, 3);
    const size_t at = 3 * size_t(i);
    const double x = kf_mix<TAPS>(b, f0, f1, f2, f3, at), y = kf_mix<TAPS>(b, f0, f1, f2, f3, at + 1), z = kf_mix<TAPS>(b, f0, f1, f2, f3, at + 2);
    const double len = sqrt((x * x + y * y) + z * z);
    const bool unit = len > 0.0 && len < INFINITY;                           // (NaN fails both)
    double* o = out + at;
    o[0] = unit ? x / len : x; o[1] = unit ? y / len : y; o[2] = unit ? z / len : z;
}

}  // namespace

hipError_t launch_kf_vertices(const double* frames, size_t stride, const KfBlend& blend, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t total = 3 * size_t(n), blocks = (total / 2 + KF_BLOCK - 1) / KF_BLOCK;
    const dim3 grid(uint32_t(blocks < 1 ? 1 : blocks > KF_MAX_BLOCKS ? KF_MAX_BLOCKS : blocks));
    if (blend.taps == 2) hipLaunchKernelGGL(kf_vertices_kernel<2>, grid, dim3(KF_BLOCK), 0, stream, frames, stride, blend, out, total);
    else hipLaunchKernelGGL(kf_vertices_kernel<4>, grid, dim3(KF_BLOCK), 0, stream, frames, stride, blend, out, total);
    return hipGetLastError();
}

hipError_t launch_kf_normals(const double* frames, size_t stride, const KfBlend& blend, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + KF_BLOCK - 1) / KF_BLOCK);
    if (blend.taps == 2) hipLaunchKernelGGL(kf_normals_kernel<2>, grid, dim3(KF_BLOCK), 0, stream, frames, stride, blend, out, n);
    else hipLaunchKernelGGL(kf_normals_kernel<4>, grid, dim3(KF_BLOCK), 0, stream, frames, stride, blend, out, n);
    return hipGetLastError();
}
