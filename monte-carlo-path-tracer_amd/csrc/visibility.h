// Launcher of the face-visibility pass (visibility.hip), called from mcpt_api.cpp: after every scene update of a context with a mask the hidden
// triangles' intersection records and boxes are overwritten so that no kernel can hit them.  DESIGN.md §24 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define VS_BLOCK 256                   // threads per block (4 wave64)

// One lane per leaf-order triangle i: when visible[tri_face[i]] == 0, tri_isect[3 i + 1] and [3 i + 2] become {+0, +0, +0, 0} and tri_box[6 i ..] the
// point lo = hi = tri_isect[3 i].xyz; record 0 and every visible triangle are left alone.  visible: one byte per face (n_tris of them).
hipError_t launch_vs_hide(const uint8_t* visible, const int32_t* tri_face, float4* tri_isect, float* tri_box, uint32_t n_tris, hipStream_t stream);
