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
};

// feat: width * height * 2 float4 = {albedo rgb, coverage f}, {normal sum / hits, mean hit distance z}
hipError_t launch_dn_features(const DevScene& sc, uint32_t spp, uint32_t seed_lo, uint32_t seed_hi, float4* feat, hipStream_t stream);
// film {sum rgb, count} -> out {r, g, b, 1} (count 0: {0, 0, 0, 0}); guide, iv0, iv1: width * height float4 scratch each
hipError_t launch_dn_filter(const DnParams& p, uint32_t levels, const float4* film, const float4* feat, float4* guide, float4* iv0, float4* iv1,
                            float4* out, hipStream_t stream);
