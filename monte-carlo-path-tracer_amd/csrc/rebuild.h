// Launchers of the tree rebuild (rebuild.hip), called from mcpt_api.cpp: mcpt_rebuild_trees gives a live context new trees for the geometry it
// holds now and moves every leaf-order stream to the new leaf order on the device.  DESIGN.md §17 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include "device_scene.h"
#include "refit.h"

#define RB_BLOCK 256                   // threads per block of every rebuild kernel (4 wave64)

// One lane per leaf-order triangle i: the bound of its three vertices (rf_vtx through idx6, less the centre) goes to slot tri_face[i], FACE order:
// box32 (6 floats per face: the fp64 bound rounded outward, build_host_scene's boxes for the custom builder) and, when bound64 is given, 9 doubles
// per face (lo, hi, centroid: scene_build.h's BTri, the host builder's input).
hipError_t launch_rb_face_bounds(const double* vertex, const int32_t* idx6, const int32_t* tri_face, RfCentre centre, float* box32, double* bound64,
                                 uint32_t n_tris, hipStream_t stream);

// The leaf-order streams of a context: what rb_permute_kernel reads (old) and writes (fresh buffers of the same sizes).
struct RbStreams {
    float4* tri_isect;                 // 3 per triangle, + one spare record at the end (left alone: the fresh buffer is zero-filled by the caller)
    float4* tri_shade;                 // MCPT_TRI_SHADE_F4 per triangle
    double* tri_pos64;                 // 9 per triangle
    int32_t* idx6;                     // 6 per triangle
    int32_t* tri_face;                 // 1 per triangle
};
// Units of 16 destination bytes, one lane each: 8 n (tri_shade) + 3 n (tri_isect) + ceil(9 n / 2) (tri_pos64) + ceil(3 n / 2) (idx6) + ceil(n / 4) (tri_face).
inline uint64_t rb_permute_units(uint32_t n) { const uint64_t N = n; return 8 * N + 3 * N + (9 * N + 1) / 2 + (3 * N + 1) / 2 + (N + 3) / 4; }
// dst record i = src record src_of_dst[i], for every stream.  Record 0's .w of tri_isect keeps its class bits; its tie rank becomes i, or stays
// with keep_rank (MCPT_FLAG_REFERENCE_TIE_ORDER).  Out of place: src and dst are different buffers.
hipError_t launch_rb_permute(RbStreams src, RbStreams dst, const uint32_t* src_of_dst, uint32_t n_tris, bool keep_rank, hipStream_t stream);

// One lane per light: lights[k].tri = dst_of_src[lights[k].tri].
hipError_t launch_rb_lights(DevLight* lights, const uint32_t* dst_of_src, uint32_t n_lights, uint32_t n_tris, hipStream_t stream);
