// gfx950 kernels of the ray-generation stage: the primary ray of every pixel for one of four camera models -- pinhole, thin lens
// (disk or polygonal aperture), orthographic, equirectangular panorama -- written as 3 + 3 doubles per pixel where wf_shade_kernel reads a probe
// item's ray (RenderParams::probe_o / probe_d).  mcpt_render_camera runs this kernel and then the unchanged wavefront pipeline, once per sample.
//
// One lane per pixel, no lane reads what another writes.  tests/camera_ref.py restates the three new models in float64, one rounding per
// operation: contraction is off for everything this file adds (the Makefile says so too), sqrt is the correctly rounded one and sincos the
// device library's.  The PINHOLE model is the exception by design: it calls cast_ray of pt_device.h, and that header is compiled here the way the
// render kernels compile it (contraction allowed), so that the stage reproduces today's camera bit for bit.
#pragma clang fp contract(fast)
#include "pt_device.h"
#pragma clang fp contract(off)
#include "camera.h"

#include <cmath>

CmModel cm_make_model(const mcpt_camera_model& m) {
    CmModel c{};
    c.model = m.model;
    if (m.model == MCPT_CAMERA_THIN_LENS) {
        c.blades = m.blades; c.lens_radius = m.lens_radius; c.focus_distance = m.focus_distance;
        for (uint32_t j = 0; j < m.blades && j < CM_MAX_BLADES; j++) {
            const double a = m.blade_rotation + 2.0 * 3.14159265358979323846 * double(j) / double(m.blades);
            c.vx[j] = std::cos(a); c.vy[j] = std::sin(a);
        }
    }
    if (m.model == MCPT_CAMERA_ORTHOGRAPHIC) c.ortho_height = m.ortho_height;
    return c;
}

namespace {

#define CM_PI 3.14159265358979323846

// (pt_device.h's d3 operators were compiled with contraction allowed: the models below use these, one rounding per operation)
DEV d3 cm_axpy(double s, d3 a, d3 b) { return mkd(b.x + s * a.x, b.y + s * a.y, b.z + s * a.z); }              // b + s a
DEV d3 cm_comb(double s, d3 a, double t, d3 b) { return mkd(s * a.x + t * b.x, s * a.y + t * b.y, s * a.z + t * b.z); }
DEV d3 cm_cross(d3 a, d3 b) { return mkd(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }

// The lens point of the thin lens in units of the lens radius: a disk, or the regular polygon of m.vx / m.vy sampled triangle by triangle
// (triangle k = centre, V_k, V_k+1; a point uniform in it by the square-root map).
DEV void cm_lens_point(const CmModel& m, float xi2, float xi3, double& lx, double& ly) {
    if (m.blades == 0u) {
        const double r = sqrt((double)xi2), th = (2.0 * CM_PI) * (double)xi3;
        double s, c; sincos(th, &s, &c);
        lx = r * c; ly = r * s;
        return;
    }
    const int n = (int)m.blades;
    const double x = (double)xi2 * (double)n;
    int k = (int)x; k = k < n - 1 ? k : n - 1;
    const int k1 = k + 1 == n ? 0 : k + 1;
    const double s = sqrt(x - (double)k), a = s * (1.0 - (double)xi3), b = s * (double)xi3;
    lx = a * m.vx[k] + b * m.vx[k1]; ly = a * m.vy[k] + b * m.vy[k1];
}

// The primary ray of pixel (px, py) = `pixel` for sample `sample`: origin in device coordinates, direction as fp32.
DEV void cm_ray(const DevCamera& c, const CmModel& m, int px, int py, uint32_t pixel, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, d3& o, f3& d) {
    const Rng4 r = rng_block(pixel, sample, 0u, seed_lo, seed_hi);
    if (m.model == MCPT_CAMERA_PINHOLE) { f3 o32; cast_ray(c, px, py, r.v[0], r.v[1], o, o32, d); return; }
    const d3 eye = ld_d3(c.eye), front = ld_d3(c.front), right = ld_d3(c.right), up = ld_d3(c.up);
    const double u0 = (double)(((float)px + r.v[0]) / (float)c.width) - 0.5, v0 = (double)(((float)py + r.v[1]) / (float)c.height) - 0.5;
    const d3 lup = cm_cross(right, front);
    if (m.model == MCPT_CAMERA_THIN_LENS) {
        const double u = u0 * c.h * (double)c.width / (double)c.height, v = v0 * c.h;           // cast_ray's first two lines
        const d3 D = cm_axpy(v, up, cm_axpy(u, right, front));
        const d3 P = cm_axpy(m.focus_distance, D, eye);
        double lx, ly; cm_lens_point(m, r.v[2], r.v[3], lx, ly);
        o = cm_axpy(m.lens_radius, cm_comb(lx, right, ly, lup), eye);
        const double qx = P.x - o.x, qy = P.y - o.y, qz = P.z - o.z;
        const double inv = rsq64((qx * qx + qy * qy) + qz * qz);
        d = mk3((float)(qx * inv), (float)(qy * inv), (float)(qz * inv));
    } else if (m.model == MCPT_CAMERA_ORTHOGRAPHIC) {
        const double su = u0 * m.ortho_height * (double)c.width / (double)c.height, sv = v0 * m.ortho_height;
        o = cm_axpy(sv, up, cm_axpy(su, right, eye));
        d = to_f3(front);
    } else {                                                                                    // MCPT_CAMERA_EQUIRECT
        double sl, cl, sp, cp;
        sincos((2.0 * CM_PI) * u0, &sl, &cl); sincos(CM_PI * v0, &sp, &cp);
        const d3 a = cm_comb(cl, front, sl, right);
        o = eye;
        d = to_f3(cm_comb(cp, a, sp, lup));
    }
}

DEV void cm_store(double* __restrict__ origin, double* __restrict__ dir, size_t k, d3 o, f3 d) {
    origin[3 * k] = o.x; origin[3 * k + 1] = o.y; origin[3 * k + 2] = o.z;
    dir[3 * k] = (double)d.x; dir[3 * k + 1] = (double)d.y; dir[3 * k + 2] = (double)d.z;
}

__global__ void __launch_bounds__(CM_BLOCK) cm_rays_kernel(DevCamera cam, CmModel m, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* __restrict__ origin,
                                                           double* __restrict__ dir) {
    const uint32_t w = (uint32_t)cam.width, n = w * (uint32_t)cam.height;
    const uint32_t i = blockIdx.x * CM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int py = (int)(i / w), px = (int)(i - (uint32_t)py * w);
    d3 o; f3 d;
    cm_ray(cam, m, px, py, i, sample, seed_lo, seed_hi, o, d);
    cm_store(origin, dir, i, o, d);
}

__global__ void __launch_bounds__(CM_BLOCK) cm_probe_kernel(DevCamera cam, CmModel m, uint32_t n, const int32_t* __restrict__ xy, uint32_t sample, uint32_t seed_lo,
                                                            uint32_t seed_hi, double* __restrict__ origin, double* __restrict__ dir) {
    const uint32_t k = blockIdx.x * CM_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int px = xy[2 * k], py = xy[2 * k + 1];                          // (inside the film: mcpt_probe_camera_rays checked)
    d3 o; f3 d;
    cm_ray(cam, m, px, py, (uint32_t)py * (uint32_t)cam.width + (uint32_t)px, sample, seed_lo, seed_hi, o, d);
    cm_store(origin, dir, k, o, d);
}

}  // namespace

hipError_t launch_cm_rays(const DevCamera& cam, const CmModel& m, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin, double* dir, hipStream_t stream) {
    const uint32_t n = (uint32_t)cam.width * (uint32_t)cam.height;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cm_rays_kernel, dim3((n + CM_BLOCK - 1) / CM_BLOCK), dim3(CM_BLOCK), 0, stream, cam, m, sample, seed_lo, seed_hi, origin, dir);
    return hipGetLastError();
}

hipError_t launch_cm_probe(const DevCamera& cam, const CmModel& m, uint32_t n, const int32_t* xy, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi, double* origin,
                           double* dir, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cm_probe_kernel, dim3((n + CM_BLOCK - 1) / CM_BLOCK), dim3(CM_BLOCK), 0, stream, cam, m, n, xy, sample, seed_lo, seed_hi, origin, dir);
    return hipGetLastError();
}
