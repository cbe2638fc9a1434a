// Launchers of the scene update (refit.hip), called from mcpt_api.cpp: mcpt_update_vertices rewrites the triangle streams and the light records
// from new vertex positions and refits both trees in place.  DESIGN.md §12 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include "device_scene.h"

#define RF_BLOCK 256                   // threads per block of every refit kernel (4 wave64)

struct RfCentre { double x, y, z; };   // DevScene::centre, by value

// One lane per leaf-order triangle: tri_isect (record 0's .w kept), tri_pos64, the fp64 plane in tri_shade[4..5], the normals in
// tri_shade[0..2].xyz when `normal` is given, and tri_box (6 floats per triangle: the fp64 bound rounded outward to fp32, no padding).
// idx6: per triangle its three vertex indices, then its three normal indices.
hipError_t launch_rf_triangles(const double* vertex, const double* normal, const int32_t* idx6, RfCentre centre, float4* tri_isect, float4* tri_shade,
                               double* tri_pos64, float* tri_box, uint32_t n_tris, hipStream_t stream);
// One lane per light: area from the new edges, n0..n2 when `normal` is given, light_pos64 from tri_pos64.
hipError_t launch_rf_lights(DevLight* lights, double* light_pos64, const float4* tri_isect, const double* tri_pos64, const double* normal,
                            const int32_t* idx6, uint32_t n_lights, hipStream_t stream);
// The binary nodes order[begin .. end): both child boxes.  All of them have the same height, and every lower height has been refitted by an
// earlier launch on the stream.
hipError_t launch_rf_binary_level(float4* nodes, const uint32_t* order, uint32_t begin, uint32_t end, const float* tri_box, hipStream_t stream);
// The 8-wide records [begin, end) -- one level of the breadth-first numbering, deeper levels done by earlier launches: node_box (6 floats per
// node: the exact fp32 bound of its children), the frame and the quantised planes.
hipError_t launch_rf_wide_level(float4* nodes8, uint32_t begin, uint32_t end, const float* tri_box, float* node_box, hipStream_t stream);
// partial[b] = sum of the dequantised child-box areas of the records of block b (rf_area_blocks(n) blocks); the caller adds them up.
hipError_t launch_rf_wide_area(const float4* nodes8, uint32_t n_nodes8, double* partial, hipStream_t stream);
inline uint32_t rf_area_blocks(uint32_t n_nodes8) { return (n_nodes8 + RF_BLOCK - 1) / RF_BLOCK; }
