// Launchers of the material update (materials.hip), called from mcpt_api.cpp: mcpt_update_materials rewrites the lobe class of every triangle and
// rebuilds the light list on the device from new material records.  DESIGN.md §15 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include "device_scene.h"

#define MT_BLOCK 256                   // threads per block of every kernel here (4 wave64); also the faces one scan block covers

inline uint32_t mt_blocks(uint32_t n) { return (n + MT_BLOCK - 1) / MT_BLOCK; }

// One lane per leaf-order triangle: the top four bits of tri_isect[3 i].w become the lobe class of the triangle's material in `mats` (the 28-bit tie
// rank stays), and flag[tri_face[i]] = 1 if the material passes the light list's test (MAT_EMIT_REC), else 0.  Every face is written once.
// visible: null, or one byte per face -- a face whose byte is 0 is no light: its flag is 0 whatever its material.
hipError_t launch_mt_classes(float4* tri_isect, const float4* tri_shade, const int32_t* tri_face, const DevMaterial* mats, uint32_t n_mats,
                             uint32_t* flag, uint32_t n_tris, hipStream_t stream, const uint8_t* visible = nullptr);
// flag[0 .. n) becomes its own exclusive prefix sum, in place: three launches (per-block sums, one block over the sums, per-block scan from its
// offset), none of which waits for another block of its own launch.  sums: mt_blocks(n) words of scratch.
hipError_t launch_mt_scan(uint32_t* flag, uint32_t* sums, uint32_t n, hipStream_t stream);
// One lane per leaf-order triangle: a triangle whose material passes the light list's test writes lights[slot] and light_pos64[9 slot ..] with
// slot = scan[tri_face[i]] -- the record build_host_scene forms, from the streams as they are now.  Slots >= capacity are not written.
// visible: the mask launch_mt_classes got -- a hidden face writes nothing (its scan entry is the slot of the next visible light).
hipError_t launch_mt_emit(const float4* tri_isect, const float4* tri_shade, const double* tri_pos64, const int32_t* tri_face, const DevMaterial* mats,
                          uint32_t n_mats, const uint32_t* scan, DevLight* lights, double* light_pos64, uint32_t capacity, uint32_t n_tris,
                          hipStream_t stream, const uint8_t* visible = nullptr);
