// Launchers and host helpers of linear-blend skinning (skin.hip), called from mcpt_api.cpp: mcpt_update_skin writes the context's current vertices
// and normals from the skin's rest pose, four bone influences per record and one 3x4 matrix per bone, in front of the refit of refit.hip.
// DESIGN.md §18 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SK_BLOCK 256                   // threads per block of both kernels (4 wave64)
#define SK_INFLUENCES 4                // bone ids and weights per record (include/mcpt.h: MCPT_SKIN_INFLUENCES)
#define SK_RECORD 12                   // doubles per bone in the table: [A | t] row-major, as the caller gives it

// The two host functions here are defined in skin.hip, where contraction is off: what they return is what tests/skin_ref.py restates, whatever
// the host compiler may fuse elsewhere.
// det A of a bone's row-major 3x4 matrix [A | t], by transform.h's xf_group_record and xf_record_det.
double sk_bone_det(const double* m3x4);
// How far a row [a0 a1 a2 | t] of a bone can carry a coordinate of a vertex that lies within |coordinate| <= radius, with the slack that covers
// a weight sum of up to 1 + 1e-6 and the blend's rounding: (1 + 2^-16) * (((|a0| + |a1|) + |a2|) * radius + |t|).
double sk_row_reach(const double* row4, double radius);

// One lane per vertex.  bone: 4 ids per vertex (each < the table's bone count), weight: 4 doubles per vertex, both 16-byte aligned.  Entrywise
// B = ((w0 M0 + w1 M1) + w2 M2) + w3 M3 -- all four slots, whatever their weight -- then out = ((B0 x + B1 y) + B2 z) + B3 per row, x y z from `rest`.
hipError_t launch_sk_vertices(const double* rest, const uint32_t* bone, const double* weight, const double* table, double* out, uint32_t n, hipStream_t stream);
// One lane per normal, with its own influences: the 3x3 of B blended as above, C = cof(A_B) by xf_group_record's nine formulas, v = (C0 x + C1 y) + C2 z
// per row; out = v / |v| when |v| is finite and > 0, else v.
hipError_t launch_sk_normals(const double* rest, const uint32_t* bone, const double* weight, const double* table, double* out, uint32_t n, hipStream_t stream);
