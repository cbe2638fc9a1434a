// Launcher and host helper of automatic smooth normals (normals.hip), called from mcpt_api.cpp: while mcpt_set_auto_normals is in force every
// scene update recomputes the chosen normal records from the deformed faces -- area-weighted face normals, summed per record in a fixed order --
// after the update's route has written rf_vtx / rf_nrm and in front of the refit of refit.hip.  DESIGN.md §20 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#define NR_BLOCK 256                   // threads per block of the kernel (4 wave64)

// One face of one normal record: the face's vertex indices in corner order and whether its geometric normal is negated before it is added.
// 16 bytes, read by a lane as one 16-byte load.
struct alignas(16) NrEntry { uint32_t v0, v1, v2, flip; };
static_assert(sizeof(NrEntry) == 16, "a normals entry is one 16-byte load");

// Defined in normals.hip, where contraction is off: the `flip` dots are exactly what tests/normals_ref.py restates, whatever the host compiler
// may fuse elsewhere.  Touches no device.
// face_vertex / face_normal: 3 indices per face in corner order, faces in Model::face order (already validated: < n_vertex / < n_normal).
// mask: n_normal bytes, != 0 = recompute the record; null = all.  vertex / normal: the reference pose, 3 doubles per record.
// offset gets n_normal + 1 entries; record i owns entries [offset[i], offset[i + 1]): one per face that names it in ANY corner (once, however
// many corners name it), by ascending face index; none for a masked-out or unused record.
// flip = ((g.x n.x + g.y n.y) + g.z n.z) < 0 with g = cross(v1 - v0, v2 - v0) at the reference pose and n the record's reference normal (a
// zero or NaN dot: 0).  Returns the largest number of entries of one record.
uint32_t nr_per_record(const int32_t* face_vertex, const int32_t* face_normal, uint32_t n_face, uint32_t n_normal, const uint8_t* mask,
                       const double* vertex, const double* normal, std::vector<uint32_t>& offset, std::vector<NrEntry>& entry);

// One lane per normal record.  offset: n + 1 entries, entry: 16-byte aligned, every index < the vertex count.  s = +0; per entry in stored order
// s = s + sigma * cross(V[v1] - V[v0], V[v2] - V[v0]) (sigma = -1 when flip, else +1); len = sqrt((s.x s.x + s.y s.y) + s.z s.z);
// normal[i] = s / len when len is finite and > 0.  Otherwise, and for a record without entries, normal[i] is NOT written.  n == 0 launches nothing.
hipError_t launch_nr_normals(const double* vertex, const uint32_t* offset, const NrEntry* entry, double* normal, uint32_t n, hipStream_t stream);
