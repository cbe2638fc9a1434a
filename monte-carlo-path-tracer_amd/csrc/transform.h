// Launchers of the rigid-part update (transform.hip), called from mcpt_api.cpp: mcpt_update_transforms writes the context's current vertices and
// normals from a rest pose and one 3x4 matrix per group, in front of the refit of refit.hip.  DESIGN.md §16 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define XF_BLOCK 256                   // threads per block of both kernels (4 wave64)
#define XF_RECORD 21                   // doubles per group in the table: [A | t] row-major (12), then cof(A) row-major (9)

// One group's table record from its row-major 3x4 matrix [A | t]: the matrix as it is, then the cofactor matrix of A (= det(A) A^-T), every
// entry p*q - r*s rounded as two products and one subtraction.  The three host functions here are defined in transform.hip, where contraction
// is off: what they return is what tests/transform_ref.py restates, whatever the host compiler may fuse elsewhere.
void xf_group_record(const double* m3x4, double* record);
// det(A) = (a00 c00 + a01 c01) + a02 c02 from a record.
double xf_record_det(const double* record);
// How far a row [a0 a1 a2 | t] can carry a coordinate of a group whose vertices lie within |coordinate| <= radius:
// ((|a0| + |a1|) + |a2|) * radius + |t|.
double xf_row_reach(const double* row4, double radius);

// One lane per vertex: out = ((a0 x + a1 y) + a2 z) + t per row of its group's matrix, x y z from `rest`.  group[i] < the table's group count.
hipError_t launch_xf_vertices(const double* rest, const uint32_t* group, const double* table, double* out, uint32_t n, hipStream_t stream);
// One lane per normal: c = cof(A) n, each row (c0 x + c1 y) + c2 z; out = c / |c| when |c| is finite and > 0, else c.
hipError_t launch_xf_normals(const double* rest, const uint32_t* group, const double* table, double* out, uint32_t n, hipStream_t stream);
