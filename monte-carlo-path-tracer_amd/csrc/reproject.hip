// gfx950 kernel of temporal reprojection: the film of the old view gathered at the surface points of the new view.  It runs on
// the context's stream between the feature render of the new view and the next path kernels, and touches nothing the path kernels read.
// The projection is fp64 like cast_ray (an identity move must land on its own pixel to 1e-13), the film arithmetic fp32.
#include "pt_device.h"
#include "reproject.h"

DEV float4 rp_none() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// One lane per pixel of the NEW view; a wave is one row segment.  Plain loads, one 16-B store per lane, one 8-B atomic per wave.
__global__ void __launch_bounds__(RP_BX * RP_BY) rp_reproject_kernel(RpParams p, const float4* __restrict__ old_film, const float4* __restrict__ old_feat,
                                                                   const float4* __restrict__ new_feat, float4* __restrict__ out,
                                                                   unsigned long long* __restrict__ reused) {
    const int W = p.new_cam.width, H = p.new_cam.height;
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    bool wrote = false;
    if (x < W && y < H) {
        const size_t i = (size_t)y * W + x;
        float4 res = rp_none();
        const float4 fa = new_feat[2 * i], fn = new_feat[2 * i + 1];
        const float nn = fn.x * fn.x + fn.y * fn.y + fn.z * fn.z;
        // no history for background, emitters and mostly-emissive pixels (coverage below one half), nor without a normal
        if (fa.w >= 0.5f && fn.w > 0.f && nn > 0.f) {
            const float ninv = 1.f / sqrtf(nn);
            const float npx = fn.x * ninv, npy = fn.y * ninv, npz = fn.z * ninv;
            // the pixel-centre ray of the new view: cast_ray's arithmetic with xi = 0.5, the centre itself formed in fp64 (cast_ray's float
            // quotient (x + xi) / width is exact only for power-of-two sizes; with it an identity move would miss its own pixel by 1e-5)
            const DevCamera& c = p.new_cam;
            const double u = (((double)x + 0.5) / (double)W - 0.5) * c.h * (double)W / (double)H;
            const double v = (((double)y + 0.5) / (double)H - 0.5) * c.h;
            const double dx = c.front[0] + u * c.right[0] + v * c.up[0];
            const double dy = c.front[1] + u * c.right[1] + v * c.up[1];
            const double dz = c.front[2] + u * c.right[2] + v * c.up[2];
            const double zi = (double)fn.w * rsq64(dx * dx + dy * dy + dz * dz);
            // from the old eye to the surface point
            const DevCamera& o = p.old_cam;
            const double vx = (c.eye[0] - o.eye[0]) + zi * dx, vy = (c.eye[1] - o.eye[1]) + zi * dy, vz = (c.eye[2] - o.eye[2]) + zi * dz;
            const double c0 = p.inv[0] * vx + p.inv[1] * vy + p.inv[2] * vz;
            const double c1 = p.inv[3] * vx + p.inv[4] * vy + p.inv[5] * vz;
            const double c2 = p.inv[6] * vx + p.inv[7] * vy + p.inv[8] * vz;
            if (c0 > 0.0) {                                                       // (else: behind the old eye)
                // continuous old pixel coordinates, pixel centres at integer + 0.5: the inverse of cast_ray's first two lines
                const double sx = ((c1 / c0) / (o.h * (double)W / (double)H) + 0.5) * (double)W - 0.5;
                const double sy = ((c2 / c0) / o.h + 0.5) * (double)H - 0.5;
                if (sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H) {   // (else no tap is inside; also keeps the floor in int range)
                    const float r = (float)sqrt(vx * vx + vy * vy + vz * vz);      // the depth the old view must have seen
                    const double flx = floor(sx), fly = floor(sy);
                    const int x0 = (int)flx, y0 = (int)fly;
                    const float fx = (float)(sx - flx), fy = (float)(sy - fly);
                    const float ztol = p.depth_tolerance * r;
                    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
                        const float wq = ((t & 1) ? fx : 1.f - fx) * ((t >> 1) ? fy : 1.f - fy);
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H || !(wq > 0.f)) continue;
                        const size_t q = (size_t)qy * W + qx;
                        const float4 qf = old_film[q];
                        if (!(qf.w > 0.f)) continue;
                        const float4 qa = old_feat[2 * q];
                        if (!(qa.w >= 0.5f)) continue;
                        const float4 qn = old_feat[2 * q + 1];
                        if (!(fabsf(qn.w - r) <= ztol)) continue;
                        const float qq = qn.x * qn.x + qn.y * qn.y + qn.z * qn.z;
                        if (!(qq > 0.f)) continue;
                        const float qinv = 1.f / sqrtf(qq);
                        if (!((qn.x * npx + qn.y * npy + qn.z * npz) * qinv >= p.normal_threshold)) continue;
                        // NaN components zeroed like the render path's film writes (Scene::set_Pixel)
                        const float mr = qf.x != qf.x ? 0.f : qf.x / qf.w, mg = qf.y != qf.y ? 0.f : qf.y / qf.w, mb = qf.z != qf.z ? 0.f : qf.z / qf.w;
                        sw += wq; sr += wq * mr; sg += wq * mg; sb += wq * mb; sc += wq * qf.w;
                    }
                    if (sw >= 0.25f) {                                            // (less: a thin sliver at a disocclusion edge)
                        // rint, not floor: an identity move lands on x -+ 1e-13 and the stray tap's weight must not drop a count
                        const float nh = fminf(rintf(sc / sw), p.max_history);
                        if (nh >= 1.f) {
                            res = make_float4(sr / sw * nh, sg / sw * nh, sb / sw * nh, nh);
                            wrote = true;
                        }
                    }
                }
            }
        }
        out[i] = res;
    }
    const unsigned long long m = __ballot(wrote);
    if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(reused, (unsigned long long)__popcll(m));
}

hipError_t launch_rp_reproject(const RpParams& p, const float4* old_film, const float4* old_feat, const float4* new_feat, float4* out,
                               unsigned long long* reused, hipStream_t stream) {
    const dim3 grid((p.new_cam.width + RP_BX - 1) / RP_BX, (p.new_cam.height + RP_BY - 1) / RP_BY), block(RP_BX, RP_BY);
    hipLaunchKernelGGL(rp_reproject_kernel, grid, block, 0, stream, p, old_film, old_feat, new_feat, out, reused);
    return hipGetLastError();
}
