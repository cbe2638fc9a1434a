// Launchers and host helpers of morph targets (morph.hip), called from mcpt_api.cpp: mcpt_update_morph writes the context's current vertices and
// normals -- or, in front of the skin, two scratch arrays -- from the morph's rest pose, a per-record list of displacement entries and one weight
// per target, in front of the refit of refit.hip.  DESIGN.md §19 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#define MO_BLOCK 256                   // threads per block of both kernels (4 wave64)

// One displacement of one record by one target: 32 bytes, read by a lane as two 16-byte loads.
struct alignas(16) MoEntry { double dx, dy, dz; uint32_t target, pad; };
static_assert(sizeof(MoEntry) == 32, "a morph entry is two 16-byte loads");

// The host functions here are defined in morph.hip, where contraction is off: what they return is what tests/morph_ref.py restates, whatever the
// host compiler may fuse elsewhere.  Neither touches a device.
// The caller's per-TARGET lists (mcpt_morph_targets: target k owns entries [target_offset[k], target_offset[k + 1]), `index` names the record an
// entry displaces, `delta` holds 3 doubles per entry; already validated) turned into the per-RECORD layout the kernels gather from: offset has
// n_records + 1 entries, record i owns entries [offset[i], offset[i + 1]), ordered by ascending target id.  A counting sort, O(entries + records).
void mo_per_record(const uint32_t* target_offset, const uint32_t* index, const double* delta, uint32_t n_targets, uint32_t n_records,
                   std::vector<uint32_t>& offset, std::vector<MoEntry>& entry);
// How far a morphed coordinate can lie from 0: (1 + 2^-16) * (R + sum_k |w_k| D_k), the sum sequential in k starting from R.  R: the largest
// |coordinate| of the rest pose, D_k: the largest |delta component| of target k (both over the vertices a face uses).
double mo_reach(double radius, const double* weight, const double* target_delta, uint32_t n_targets);

// One lane per vertex.  offset: n + 1 entries, entry: 16-byte aligned, every entry's target < the weight table's length.  p = rest; per entry of
// the record in stored order and per component p = p + weight[target] * d -- every entry, whatever its weight; out = p.  A record without entries
// is copied bit for bit.  n == 0 launches nothing.  `rest` and `out` must not overlap.
hipError_t launch_mo_vertices(const double* rest, const uint32_t* offset, const MoEntry* entry, const double* weight, double* out, uint32_t n, hipStream_t stream);
// One lane per normal, with its own lists: the same sum, then v / |v| with |v| = sqrt((x x + y y) + z z) when that is finite and > 0, else v.  A
// record without entries is copied bit for bit, NOT normalised.
hipError_t launch_mo_normals(const double* rest, const uint32_t* offset, const MoEntry* entry, const double* weight, double* out, uint32_t n, hipStream_t stream);
