// Launchers and host helpers of linear-blend skinning (skin.hip), called from mcpt_api.cpp: mcpt_update_skin writes the context's current vertices
// and normals from the skin's rest pose, four bone influences per record and one 3x4 matrix per bone, in front of the refit of refit.hip.
// DESIGN.md §18 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SK_BLOCK 256                   // threads per block of both kernels (4 wave64)
#define SK_INFLUENCES 4                // bone ids and weights per record (include/mcpt.h: MCPT_SKIN_INFLUENCES)
#define SK_RECORD 12                   // doubles per bone in the table: [A | t] row-major, as the caller gives it
#define SK_DQ_RECORD 8                 // doubles per bone in dual-quaternion mode's table: {w, x, y, z, dw, dx, dy, dz}
#define SK_DQ_RIGID_TOLERANCE 1e-6     // |A^T A - I| per entry of a bone that dual-quaternion mode accepts (mcpt_set_vertex_skin's weight tolerance)
#define SK_DQ_MIN_NORM2 0x1p-8         // a blended rotation quaternion of squared length below this (length < 1/16) is degenerate: the record keeps its rest pose

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

// ---- dual-quaternion mode (MCPT_SKIN_DUAL_QUATERNION).  The host functions are defined in skin.hip for the same reason as the two
// above; tests/skin_dq_ref.py restates them.
// The six entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) of A^T A: per entry (a0i a0j + a1i a1j) + a2i a2j.
void sk_bone_gram(const double* m3x4, double* out6);
// A bone that dual-quaternion mode takes: sk_bone_det > 0 and every entry of sk_bone_gram within SK_DQ_RIGID_TOLERANCE of the identity's.
bool sk_bone_rigid(const double* m3x4);
// How far a rigid bone can carry a coordinate of a vertex within |coordinate| <= radius, whatever it is blended with:
// (1 + 2^-16) * (2 * radius + 16 * ((|tx| + |ty|) + |tz|)).
double sk_dq_reach(const double* m3x4, double radius);
// The unit dual quaternion of a rigid bone: the rotation by Shepperd's method, normalised, w >= 0; the dual part 1/2 (0, t) q.
void sk_bone_dualquat(const double* m3x4, double* out8);

// One lane per vertex; `table` holds SK_DQ_RECORD doubles per bone, 16-byte aligned.  Slot 0 is the pivot: slot k enters with the sign s_k = -1
// when its rotation quaternion's dot product with the pivot's is < 0, else +1.  All eight components are blended as
// ((w0 q0 + (w1 s1) q1) + (w2 s2) q2) + (w3 s3) q3; n2 is the squared length of the blended real part.  !(n2 >= 2^-8 && n2 < inf): out = rest.
// Otherwise r = real / sqrt(n2), d = dual / sqrt(n2), R = the rotation matrix of r, t = 2 (r.w d_v - d.w r_v + r_v x d_v),
// out = ((R0 x + R1 y) + R2 z) + t per row.
hipError_t launch_sk_dq_vertices(const double* rest, const uint32_t* bone, const double* weight, const double* table, double* out, uint32_t n, hipStream_t stream);
// One lane per normal, with its own influences: the real parts only, the same signs and the same degenerate rule (the rest normal is copied as
// it is); otherwise v = (R0 x + R1 y) + R2 z per row and out = v / |v| when |v| is finite and > 0, else v.
hipError_t launch_sk_dq_normals(const double* rest, const uint32_t* bone, const double* weight, const double* table, double* out, uint32_t n, hipStream_t stream);
