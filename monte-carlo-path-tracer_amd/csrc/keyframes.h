// Launchers and host helpers of keyframe playback (keyframes.hip), called from mcpt_api.cpp: mcpt_update_keyframes writes the context's current
// vertices and normals by interpolating 2 or 4 of the frames that mcpt_set_vertex_keyframes left on the device, in front of the refit of
// refit.hip.  DESIGN.md §22 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#define KF_BLOCK 256                   // threads per block of both kernels (4 wave64)
#define KF_MAX_BLOCKS 2048             // the vertex kernel's grid-stride loop: at most 8 blocks per CU of an MI355X

// Doubles from one frame to the next on the device: the frame's 3 n doubles rounded up to an even number, so that every frame starts 16-byte
// aligned (3 n is odd when n is odd).
inline size_t kf_stride(uint32_t n_records) { return (3 * size_t(n_records) + 1) & ~size_t(1); }

// What one update blends: `taps` frames (2 linear, 4 Catmull-Rom; tap[] and w[] beyond are 0) by their weights.  Travels as a kernel argument.
struct KfBlend { double w[4]; uint32_t tap[4]; uint32_t taps, k; double u; };

// The host functions here are defined in keyframes.hip, where contraction is off: what they return is what tests/keyframes_ref.py restates,
// whatever the host compiler may fuse elsewhere.  None touches a device.  interpolation: MCPT_KEYFRAMES_LINEAR (0) / _CATMULL_ROM (1); wrap:
// MCPT_KEYFRAMES_CLAMP (0) / _LOOP (1); both already validated.
// A finite time to its segment: k, u in [0, 1) and the tap indices (mcpt.h has the rules); w is left 0.
KfBlend kf_segment(double time, double start_time, double frame_time, uint32_t n_frames, uint32_t interpolation, uint32_t wrap);
// The 2 or 4 weights of u, never renormalised; w[] beyond them is 0.
void kf_weights(double u, uint32_t interpolation, double w[4]);
// How far an interpolated coordinate can lie from 0: (1 + 2^-16) (c R), c = 1 linear, 1.25 Catmull-Rom; R: the largest |coordinate| of a vertex
// that a face uses, over all frames.
double kf_reach(double radius, uint32_t interpolation);

// frames: n_frames arrays of `stride` doubles (stride even, the base 16-byte aligned), every tap < n_frames; out: 3 n doubles, 16-byte aligned.
// Per component out = w0 a + w1 b (2 taps) or ((w0 a + w1 b) + w2 c) + w3 d (4 taps).  Two doubles per lane and step (16-byte loads and stores),
// grid-stride; when 3 n is odd the last double is handled alone.  n == 0 launches nothing.  `frames` and `out` must not overlap.
hipError_t launch_kf_vertices(const double* frames, size_t stride, const KfBlend& blend, double* out, uint32_t n, hipStream_t stream);
// One lane per normal: the same sum, then v / |v| with |v| = sqrt((x x + y y) + z z) when that is finite and > 0, else v.
hipError_t launch_kf_normals(const double* frames, size_t stride, const KfBlend& blend, double* out, uint32_t n, hipStream_t stream);
