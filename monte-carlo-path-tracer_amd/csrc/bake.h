// Launchers of the surface-baking stage (bake.hip), called from mcpt_api.cpp: one cosine-weighted ray per bake point, written where
// wf_shade_kernel reads a probe item's ray (RenderParams::probe_o / probe_d), and the resolve of the bake film.  DESIGN.md §27 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_scene.h"
#include "../../include/mcpt.h"

#define BK_BLOCK 256                   // threads per block (4 wave64)

// A bake point as the kernels take it: mcpt_bake_point with the face replaced by its leaf-order triangle (the index of tri_pos64 / tri_shade).
struct BkPoint { int32_t tri; float u, v; uint32_t flags; };
static_assert(sizeof(BkPoint) == 16 && sizeof(mcpt_bake_point) == 16, "16 B per point on both sides");

// One lane per point i < n: origin[3 i ..] = the point in device coordinates, dir[3 i ..] = a cosine-weighted direction about its normal (three fp32
// values held as doubles) from rng_block(i, sample, 0, seed).v[0..1], dead[i] = 1 where the point has no normal (the ray is then the point, or 0
// where that is not finite, along +z).  Both ray arrays hold 3 n doubles.
hipError_t launch_bk_rays(const DevScene& sc, const BkPoint* points, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin, double* dir,
                          uint8_t* dead, hipStream_t stream);
// Between the ray kernel and the pass: one lane per item traces its ray to the first hit over the binary tree (the context's binary_ok must
// hold) and, where that is an emitter seen from BEHIND, subtracts the emitter's radiance from film[i] -- what the pass then adds for a primary
// hit, whatever its side.  Dead items are left alone.
hipError_t launch_bk_unlit(const DevScene& sc, const double* origin, const double* dir, const uint8_t* dead, uint32_t n, float4* film, hipStream_t stream);
// MCPT_BAKE_DIRECT_MIS: launched in launch_bk_unlit's place.  One lane per item adds to film[i] the MIS-weighted light sample of the bake point and
// takes out what the pass would add too much for the ray's first hit -- an emitter's back as above, and the share 1 - w_b of a light's front
// (bk_direct in bake.hip).  `points` and the sample's key give the normal again; `dir` is the ray kernel's array.  Dead items are left alone.
hipError_t launch_bk_direct(const DevScene& sc, const BkPoint* points, const double* dir, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, float4* film,
                            hipStream_t stream);
// The same device function for points first .. first + n - 1 (item numbers included), no film touched: 12 floats and 4 ints per point, see
// mcpt_probe_bake_direct.
hipError_t launch_bk_direct_probe(const DevScene& sc, const BkPoint* points, uint32_t first, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, float* out12,
                                  int32_t* out4, hipStream_t stream);
// The ray kernel's device function for points first .. first + n - 1 (item numbers included): ray k goes to row k of the outputs, the unit normal too.
hipError_t launch_bk_probe(const DevScene& sc, const BkPoint* points, uint32_t first, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin,
                           double* dir, double* normal, uint8_t* dead, hipStream_t stream);
// One lane per point: out[i] from film[i] = {sum L, count} by `mode` (MCPT_BAKE_*); {0, 0, 0, 0} for a dead point or a count of 0.
hipError_t launch_bk_resolve(const DevScene& sc, const BkPoint* points, const uint8_t* dead, const float4* film, uint32_t n, uint32_t mode, float4* out, hipStream_t stream);
