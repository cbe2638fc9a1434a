// Launchers of the ray-generation stage (camera.hip), called from mcpt_api.cpp: one primary ray per pixel for a chosen camera model, written where
// wf_shade_kernel reads a probe item's ray (RenderParams::probe_o / probe_d).  DESIGN.md §25 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_scene.h"
#include "../../include/mcpt.h"

#define CM_BLOCK 256                   // threads per block (4 wave64)
#define CM_MAX_BLADES 16

// The model as the kernel takes it, by value.  vx / vy: the aperture polygon's vertices (cos, sin)(blade_rotation + 2 pi j / blades), j < blades,
// formed on the host in fp64 (cm_make_model); unused entries are 0.  Fields of models other than `model` are ignored.
struct CmModel {
    uint32_t model, blades;            // MCPT_CAMERA_*; 0 = disk, 3..CM_MAX_BLADES = polygon
    double lens_radius, focus_distance, ortho_height;
    double vx[CM_MAX_BLADES], vy[CM_MAX_BLADES];
};
CmModel cm_make_model(const mcpt_camera_model& m);      // host only; `m` has been validated

// One lane per pixel i = y * width + x of cam's film: origin[3 i ..] = the ray's origin in device coordinates (relative to DevScene::centre, like
// DevCamera::eye), dir[3 i ..] = its direction, three fp32 values held as doubles.  Random numbers: rng_block(i, sample, 0, seed), v[0..1] the pixel
// jitter, v[2..3] the lens sample.  Both arrays hold 3 * width * height doubles.
hipError_t launch_cm_rays(const DevCamera& cam, const CmModel& m, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin, double* dir, hipStream_t stream);
// The same device function for n listed pixels (xy: 2 ints each, inside the film): ray k goes to origin[3 k ..] / dir[3 k ..].
hipError_t launch_cm_probe(const DevCamera& cam, const CmModel& m, uint32_t n, const int32_t* xy, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin,
                           double* dir, hipStream_t stream);
