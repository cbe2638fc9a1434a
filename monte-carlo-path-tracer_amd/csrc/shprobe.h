// Launchers of the light-probe stage (shprobe.hip), called from mcpt_api.cpp: 64 directions per probe and pass, stratified over the whole sphere and
// written where wf_shade_kernel reads a probe item's ray (RenderParams::probe_o / probe_d), a first-hit kernel, the projection of a pass's radiance
// onto the nine real spherical harmonics of bands 0 .. 2 with a fixed-order reduction over the probe's wave, and the resolve.  DESIGN.md §28 has
// the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_scene.h"
#include "../../include/mcpt.h"

#define SH_BLOCK 256                   // threads per block (4 wave64 = 4 probes)
#define SH_DIRS 64                     // directions per probe and pass: one wave64 per probe, item i = probe i >> 6, slot i & 63
#define SH_COEFFS 27                   // 9 coefficients x 3 channels, channel-major: [9 c + k], k = l (l + 1) + m

// One lane per item i < 64 n: origin[3 i ..] = pos[3 (i >> 6) ..] (the probe in device coordinates), dir[3 i ..] = the slot's stratified direction
// (three fp32 values held as doubles) from rng_block(i, sample, 0, seed).v[0..1].  Both ray arrays hold 3 * 64 n doubles.
hipError_t launch_sh_rays(const double* pos, uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin, double* dir, hipStream_t stream);
// The same device function for items first .. first + n_items - 1 (item numbers included): ray k goes to row k of the outputs.
hipError_t launch_sh_probe(const double* pos, uint32_t first, uint32_t n_items, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin, double* dir,
                           hipStream_t stream);
// Between the ray kernel and the pass, over the zeroed scratch film: one lane per item traces its ray to the first hit over the binary tree (the
// context's binary_ok must hold), writes cls[i] = 0 (miss), 1 (a hit from the front) or 2 (a hit from behind) and, where the hit is an emitter
// seen from BEHIND, subtracts the emitter's radiance from film[i] -- what the pass then adds for a primary hit, whatever its side.
hipError_t launch_sh_first_hit(const DevScene& sc, const double* origin, const double* dir, uint32_t n_items, float4* film, uint8_t* cls, hipStream_t stream);
// After the pass: one wave per probe p < n.  Lane j takes L = film[64 p + j].xyz (a component that is not finite counts as 0) and the fp32
// direction dir[3 (64 p + j) ..], forms the 27 products L_c Y_k and the wave sums them in the fixed tree s[j] + s[j + 32], then + 16, ... + 1; lane 0
// adds the sums to acc[27 p ..] and {64, back hits, misses} to counts[3 p ..].  No atomics.
hipError_t launch_sh_project(const float4* film, const double* dir, const uint8_t* cls, uint32_t n, float* acc, uint32_t* counts, hipStream_t stream);
// One lane per probe: out[27 p + 9 c + k] = float(4 pi) / float(rays) * acc[...] (MCPT_SH_RADIANCE), times the band's factor float(pi),
// float(2 pi / 3), float(pi / 4) for MCPT_SH_IRRADIANCE; all 0 where rays == 0.
hipError_t launch_sh_resolve(const float* acc, const uint32_t* counts, uint32_t n, uint32_t mode, float* out, hipStream_t stream);
