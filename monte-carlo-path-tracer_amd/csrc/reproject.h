// Launcher of temporal reprojection (reproject.hip), called from mcpt_api.cpp.  DESIGN.md §13 has the specification.
//
// After a camera move the film of the OLD view is looked up per pixel of the NEW view: the new pixel's first-hit surface point (its feature
// depth along the pixel-centre ray) is projected into the old view and the old film is gathered bilinearly there, tap by tap under a depth
// and a normal test against the old view's features.  What comes over is a mean and a sample count, the count capped at max_history.
// The cap is the point of the design: reprojected radiance is exact only for view-independent (diffuse) shading; on glossy and mirror
// surfaces it lags behind the view, and the cap bounds how long that stale radiance survives once new samples are added.  Nothing here
// classifies lobes.  Moving geometry is followed by rp_reproject_motion_kernel: the first hit of the new pixel's centre ray names a
// triangle and barycentrics, the vertices the scene had BEFORE the update say where that surface point was, and from there on it is the same gather.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "device_scene.h"

#define RP_BX 64               // a wave is one row segment of 64 pixels (the block shape of dn_atrous_kernel)
#define RP_BY 4

struct RpParams {
    DevCamera old_cam, new_cam;    // both eyes relative to the same creation-time centre
    double inv[9];                 // row-major inverse of the old view's image basis [front | right | up] (rp_basis_inverse)
    float max_history;             // cap on the sample count carried over, >= 1
    float depth_tolerance;         // relative, in (0, 1]
    float normal_threshold;        // minimum cosine, in (0, 1]
};

// camera_constants() keeps the caller's `up` as given -- not unit, not orthogonal to `front` -- so a view maps (a, a u, a w) to
// a (front + u right + w up): a general 3 x 3 basis.  Its inverse, fp64; false when the basis is singular (|det| below 1e-12 of the product
// of the column lengths, or not a number: `up` parallel to `front`), in which case nothing can be reprojected.
inline bool rp_basis_inverse(const DevCamera& c, double inv[9]) {
    const double* f = c.front; const double* r = c.right; const double* u = c.up;
    const double rxu[3] = {r[1] * u[2] - r[2] * u[1], r[2] * u[0] - r[0] * u[2], r[0] * u[1] - r[1] * u[0]};
    const double uxf[3] = {u[1] * f[2] - u[2] * f[1], u[2] * f[0] - u[0] * f[2], u[0] * f[1] - u[1] * f[0]};
    const double fxr[3] = {f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]};
    const double det = f[0] * rxu[0] + f[1] * rxu[1] + f[2] * rxu[2];
    const double lf = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]), lr = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]),
                 lu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    if (!(std::fabs(det) >= 1e-12 * lf * lr * lu) || !(std::fabs(det) > 0.0)) return false;
    for (int a = 0; a < 3; a++) { inv[a] = rxu[a] / det; inv[3 + a] = uxf[a] / det; inv[6 + a] = fxr[a] / det; }
    return true;
}

// old_film: width * height {sum rgb, count} of the old view (a copy: `out` may be the film it was copied from); old_feat / new_feat:
// width * height * 2 float4 in dn_features_kernel's layout; out: {mean * n_hist, n_hist} or {0, 0, 0, 0} per pixel of the new view;
// *reused (zeroed by the caller, in stream order) += the pixels written with n_hist >= 1.
hipError_t launch_rp_reproject(const RpParams& p, const float4* old_film, const float4* old_feat, const float4* new_feat, float4* out,
                               unsigned long long* reused, hipStream_t stream);

// What rp_reproject_motion_kernel needs beside RpParams.  The lengths bound every index the kernel reads from memory.
struct RpMotion {
    const float4* hits;            // width * height {leaf-order triangle or -1, u, v, t} of the NEW scene and view (rp_first_hit_kernel's output)
    const int32_t* idx6;           // 6 per triangle (leaf order): its three vertex indices, then its three normal indices (the refit's rf_idx)
    const double* old_vtx;         // the vertices before the update, WORLD coordinates, 3 per vertex
    const double* old_nrm;         // the normals before the update, 3 per normal
    const float4* tri_shade;       // record [3].w: the triangle's material
    const DevMaterial* mats;
    double centre[3];              // DevScene::centre
    uint32_t n_tris, n_vertex, n_normal, n_mats;
};
// The closest hit of every pixel-centre ray of sc.cam over the binary tree (the caller has checked that the tree fits the traversal stack).
hipError_t launch_rp_first_hit(const DevScene& sc, float4* hits, hipStream_t stream);
// launch_rp_reproject for a scene whose vertices moved: same buffers, same `reused` contract.
hipError_t launch_rp_reproject_motion(const RpParams& p, const RpMotion& m, const float4* old_film, const float4* old_feat, const float4* new_feat,
                                      float4* out, unsigned long long* reused, hipStream_t stream);
