// Launchers of the denoised preview (denoise.hip), called from mcpt_api.cpp.  DESIGN.md §Denoiser has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include "device_scene.h"

#define DN_MAX_SPP 64          // samples per pixel of one mcpt_render_features call
#define DN_MAX_LEVELS 10       // a-trous levels of one mcpt_denoise call

struct DnParams {
    int width, height;
    float sigma_c, sigma_n, sigma_z;
    float theta;               // angle of one pixel: 2 tan(fovy / 2) / height
    float clamp_k;             // firefly clamp: k >= 1, or 0 = no clamp
};

// feat: width * height * 2 float4 = {albedo rgb, coverage f}, {normal sum / hits, mean hit distance z}
// emis: width * height float4 = {emitted radiance of the first hits / spp, emitter hits / spp}.  Either of feat, emis may be null (not both):
// what the other one gets does not depend on it, bit for bit.
hipError_t launch_dn_features(const DevScene& sc, uint32_t spp, uint32_t seed_lo, uint32_t seed_hi, float4* feat, float4* emis, hipStream_t stream);
// film {sum rgb, count} -> out {r, g, b, 1} (count 0: {0, 0, 0, 0}); guide, iv0, iv1: width * height float4 scratch each.  emis non-null: the
// emission is split off before the filter and added back after it; p.clamp_k > 0: fireflies are clamped.
hipError_t launch_dn_filter(const DnParams& p, uint32_t levels, const float4* film, const float4* feat, const float4* emis, float4* guide, float4* iv0,
                            float4* iv1, float4* out, hipStream_t stream);
