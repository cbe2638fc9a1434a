// gfx950 kernels of temporal reprojection: the film of the old view gathered at the surface points of the new view.  They run
// on the context's stream between the feature render of the new view and the next path kernels, and touch nothing the path kernels read.
// The projection is fp64 like cast_ray (an identity move must land on its own pixel to 1e-13), the film arithmetic fp32.
// §13 (a camera move) finds the surface point from the new view's feature depth; §14 (a vertex update, with or without a camera move) finds where
// that point WAS: the first hit of the pixel-centre ray names a triangle and barycentrics, and the old vertices put them back in the old scene.
#include "pt_device.h"
#include "reproject.h"

DEV float4 rp_none() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// §13 steps 3 - 6, shared by both kernels: the surface point old eye + (vx, vy, vz) projected into the old view, the old film gathered bilinearly
// there under the tap rules.  (npx, npy, npz): the unit normal a tap's normal is compared with.  True, and `res` written, when a history of >= 1
// sample comes over; `res` is left as it is otherwise.
DEV bool rp_gather(const RpParams& p, const int W, const int H, const double vx, const double vy, const double vz, const float npx, const float npy,
                   const float npz, const float4* __restrict__ old_film, const float4* __restrict__ old_feat, float4& res) {
    const DevCamera& o = p.old_cam;
    bool wrote = false;
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
    return wrote;
}

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
            wrote = rp_gather(p, W, H, vx, vy, vz, npx, npy, npz, old_film, old_feat, res);
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

// ---------------------------------------------------------------------------------------------- motion vectors
// One lane per pixel like dn_features_kernel, same traversal call and LDS stack: the closest hit of the pixel-centre ray (cast_ray, xi = 0.5, 0.5)
// over the binary tree.  One 16-B record per pixel: {leaf-order triangle or -1, u, v, t}.
__global__ void __launch_bounds__(MCPT_BLOCK) rp_first_hit_kernel(DevScene sc, float4* __restrict__ hits) {
    __shared__ int s_stack[MCPT_STACK_DEPTH * MCPT_BLOCK];
    int* stk = s_stack + threadIdx.x;
    const uint32_t w = (uint32_t)sc.cam.width, n = w * (uint32_t)sc.cam.height;
    const uint32_t i = blockIdx.x * MCPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int py = (int)(i / w), px = (int)(i - (uint32_t)py * w);
    d3 o64; f3 o, d;
    cast_ray(sc.cam, px, py, 0.5f, 0.5f, o64, o, d);
    int tri = -1; float t = 0.f, u = 0.f, v = 0.f; TravCount tc = {0, 0};
    const bool hit = bvh_traverse<false, false>(sc, o, d, 1e-4f, 3.0e38f, -1, stk, tri, t, u, v, tc);
    hits[i] = hit ? make_float4(__int_as_float(tri), u, v, t) : make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
}

// rp_reproject_kernel's block shape, loads, store and count.  Per pixel of the NEW view: where its first-hit surface point was before the update
// (old vertices through the triangle's vertex indices, fp64), the old shading normal there turned towards the old eye, then rp_gather with that
// normal.  Every index read from memory -- the hit's triangle, the triangle's three vertex and three normal indices, its material -- is checked
// against its array's length before it is used; a hit record's u, v need no check (a non-finite one ends in a comparison that is false).
__global__ void __launch_bounds__(RP_BX * RP_BY) rp_reproject_motion_kernel(RpParams p, RpMotion m, const float4* __restrict__ old_film,
                                                                          const float4* __restrict__ old_feat, const float4* __restrict__ new_feat,
                                                                          float4* __restrict__ out, unsigned long long* __restrict__ reused) {
    const int W = p.new_cam.width, H = p.new_cam.height;
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    bool wrote = false;
    if (x < W && y < H) {
        const size_t i = (size_t)y * W + x;
        float4 res = rp_none();
        const float4 fa = new_feat[2 * i], fn = new_feat[2 * i + 1];
        const float nn = fn.x * fn.x + fn.y * fn.y + fn.z * fn.z;
        if (fa.w >= 0.5f && fn.w > 0.f && nn > 0.f) {
            const float4 h = m.hits[i];
            const uint32_t tri = (uint32_t)__float_as_int(h.x);                  // (a miss, -1, is out of range as well)
            if (tri < m.n_tris) {
                const int2* ip = reinterpret_cast<const int2*>(m.idx6 + 6 * (size_t)tri);   // 24-B records: 8-B aligned
                const int2 i01 = ip[0], i2n = ip[1], n12 = ip[2];
                const uint32_t mat = (uint32_t)__float_as_int(m.tri_shade[MCPT_TRI_SHADE_F4 * (size_t)tri + 3].w);
                const bool in_range = (uint32_t)i01.x < m.n_vertex && (uint32_t)i01.y < m.n_vertex && (uint32_t)i2n.x < m.n_vertex &&
                                      (uint32_t)i2n.y < m.n_normal && (uint32_t)n12.x < m.n_normal && (uint32_t)n12.y < m.n_normal && mat < m.n_mats;
                if (in_range && !(m.mats[mat].flags & MAT_EMIT_0)) {               // (emitters carry no history, as in the feature kernel)
                    // load_hit_shade's corner convention: u weighs corner 1, v corner 2
                    const double bu = (double)h.y, bv = (double)h.z, bw = 1.0 - bu - bv;
                    const d3 V0 = ld_d3(m.old_vtx + 3 * (size_t)i01.x), V1 = ld_d3(m.old_vtx + 3 * (size_t)i01.y), V2 = ld_d3(m.old_vtx + 3 * (size_t)i2n.x);
                    const d3 N0 = ld_d3(m.old_nrm + 3 * (size_t)i2n.y), N1 = ld_d3(m.old_nrm + 3 * (size_t)n12.x), N2 = ld_d3(m.old_nrm + 3 * (size_t)n12.y);
                    const DevCamera& o = p.old_cam;
                    // from the old eye to where the surface point was (vertices are world coordinates, the eye is relative to the centre)
                    const double vx = ((bw * V0.x + bu * V1.x + bv * V2.x) - m.centre[0]) - o.eye[0];
                    const double vy = ((bw * V0.y + bu * V1.y + bv * V2.y) - m.centre[1]) - o.eye[1];
                    const double vz = ((bw * V0.z + bu * V1.z + bv * V2.z) - m.centre[2]) - o.eye[2];
                    const double nx = bw * N0.x + bu * N1.x + bv * N2.x, ny = bw * N0.y + bu * N1.y + bv * N2.y, nz = bw * N0.z + bu * N1.z + bv * N2.z;
                    const double nl = nx * nx + ny * ny + nz * nz;
                    if (nl > 0.0) {
                        // the feature kernel's rule: the shading normal faces the eye that saw it
                        const double ninv = (nx * vx + ny * vy + nz * vz) > 0.0 ? -rsq64(nl) : rsq64(nl);
                        wrote = rp_gather(p, W, H, vx, vy, vz, (float)(nx * ninv), (float)(ny * ninv), (float)(nz * ninv), old_film, old_feat, res);
                    }
                }
            }
        }
        out[i] = res;
    }
    const unsigned long long b = __ballot(wrote);
    if (b != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(reused, (unsigned long long)__popcll(b));
}

hipError_t launch_rp_first_hit(const DevScene& sc, float4* hits, hipStream_t stream) {
    const uint32_t n = (uint32_t)sc.cam.width * (uint32_t)sc.cam.height;
    hipLaunchKernelGGL(rp_first_hit_kernel, dim3((n + MCPT_BLOCK - 1) / MCPT_BLOCK), dim3(MCPT_BLOCK), 0, stream, sc, hits);
    return hipGetLastError();
}

hipError_t launch_rp_reproject_motion(const RpParams& p, const RpMotion& m, const float4* old_film, const float4* old_feat, const float4* new_feat,
                                      float4* out, unsigned long long* reused, hipStream_t stream) {
    const dim3 grid((p.new_cam.width + RP_BX - 1) / RP_BX, (p.new_cam.height + RP_BY - 1) / RP_BY), block(RP_BX, RP_BY);
    hipLaunchKernelGGL(rp_reproject_motion_kernel, grid, block, 0, stream, p, m, old_film, old_feat, new_feat, out, reused);
    return hipGetLastError();
}
