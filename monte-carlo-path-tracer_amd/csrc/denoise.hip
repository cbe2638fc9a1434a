// gfx950 kernels of the denoised preview: first-hit feature buffers rendered from the film's own camera rays, and an
// edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with SVGF's variance-steered luminance term (Schied et al. 2017).  They run after
// the path kernels, on the context's stream, and touch nothing the path kernels read or write.
#include "pt_device.h"
#include "denoise.h"

// ---------------------------------------------------------------------------------------------- feature buffers
// One lane per pixel: sample s of seed `seed` traces the camera ray mcpt_render(..., seed, first_sample = 0) traces for that sample
// (rng_block camera block 0, cast_ray), closest hit over the binary tree like probe_trace_kernel.  A first hit whose material is not an
// emitter is a surface hit; per pixel {sum albedo / spp, hits / spp}, {sum camera-facing shading normal / max(hits, 1), sum t / hits}.
// EMIS: the first hits on emitters (MAT_EMIT_0, no side test: what wf_shade_kernel adds at bounce 0) go to the emission buffer
// {sum radiance / spp, emitter hits / spp}.  FEAT false renders the emission alone, from the same rays in the same order: the same bits.
template <bool FEAT, bool EMIS>
__global__ void __launch_bounds__(MCPT_BLOCK) dn_features_kernel(DevScene sc, uint32_t spp, uint32_t seed_lo, uint32_t seed_hi, float4* __restrict__ feat,
                                                                 float4* __restrict__ emis) {
    __shared__ int s_stack[MCPT_STACK_DEPTH * MCPT_BLOCK];
    int* stk = s_stack + threadIdx.x;
    const uint32_t w = (uint32_t)sc.cam.width, n = w * (uint32_t)sc.cam.height;
    const uint32_t i = blockIdx.x * MCPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int py = (int)(i / w), px = (int)(i - (uint32_t)py * w);
    f3 alb = mk3(0.f, 0.f, 0.f), nrm = mk3(0.f, 0.f, 0.f), rad = mk3(0.f, 0.f, 0.f);
    float zsum = 0.f;
    uint32_t hits = 0, lit = 0;
    for (uint32_t s = 0; s < spp; s++) {
        const Rng4 r = rng_block(i, s, 0u, seed_lo, seed_hi);
        d3 o64; f3 o, d;
        cast_ray(sc.cam, px, py, r.v[0], r.v[1], o64, o, d);
        int tri = -1; float t = 0.f, u = 0.f, v = 0.f; TravCount tc = {0, 0};
        if (!bvh_traverse<false, false>(sc, o, d, 1e-4f, 3.0e38f, -1, stk, tri, t, u, v, tc)) continue;
        const HitShade hs = load_hit_shade(sc, tri, u, v, d);
        const DevMaterial mat = sc.mats[hs.mat];
        if (mat.flags & MAT_EMIT_0) {                                             // emitters are neither surface hits nor counted
            if (EMIS) { rad = rad + mk3(mat.radiance[0], mat.radiance[1], mat.radiance[2]); lit++; }
            continue;
        }
        if (!FEAT) continue;
        uint32_t fetches = 0;
        const Bsdf b = make_bsdf(mat, tex_color(sc, mat, hs.tu, hs.tv, fetches), hs.n, d);   // kd, ks after energy_conservation
        alb = alb + (b.kd + b.ks);
        nrm = nrm + (dot(hs.n, d) > 0.f ? -hs.n : hs.n);
        zsum += t;
        hits++;
    }
    const float fs = (float)spp, fh = (float)hits, fn = (float)(hits > 0 ? hits : 1u);
    if (FEAT) {
        feat[2 * (size_t)i] = make_float4(alb.x / fs, alb.y / fs, alb.z / fs, fh / fs);
        feat[2 * (size_t)i + 1] = make_float4(nrm.x / fn, nrm.y / fn, nrm.z / fn, hits ? zsum / fh : 0.f);
    }
    if (EMIS) emis[i] = make_float4(rad.x / fs, rad.y / fs, rad.z / fs, (float)lit / fs);
}

// ---------------------------------------------------------------------------------------------- filter
#define DN_BX 64               // a wave is one row segment of 64 pixels: every tap of the 5x5 stencil is a coalesced row read
#define DN_BY 4

// make_bsdf's luminance, with its roundings spelled out.  Written as r * 0.212671f + g * 0.715160f + b * 0.072169f under -ffp-contract=fast the
// compiler picked which product to keep apart per kernel instantiation: dn_prep_robust_kernel<true, *> rounded the variance's luminance otherwise
// than dn_prep_kernel and dn_prep_robust_kernel<false, true>, so a split with E = 0 was not the filter without the split, bit for bit.  The two
// spellings are the ones the prep kernels of flags = 0 and the a-trous kernels always had: flags = 0 gives the bits it always gave.
DEV float dn_lum_prep(float r, float g, float b) { return fmaf(b, 0.072169f, fmaf(g, 0.715160f, r * 0.212671f)); }   // the prep kernels'
DEV float dn_lum(float r, float g, float b) { return fmaf(b, 0.072169f, fmaf(r, 0.212671f, g * 0.715160f)); }        // the a-trous kernels'
DEV bool dn_valid(const float4 film, const float4 fa) { return film.w > 0.f && fa.w >= 0.5f; }
// demodulated irradiance of a valid pixel: mean / albedo per channel (channels of albedo <= 1e-3 keep the mean)
DEV f3 dn_irr(const float4 film, const float4 fa) {
    const f3 c = mk3(film.x / film.w, film.y / film.w, film.z / film.w);
    return mk3(fa.x > 1e-3f ? c.x / fa.x : c.x, fa.y > 1e-3f ? c.y / fa.y : c.y, fa.z > 1e-3f ? c.z / fa.z : c.z);
}

// Level "-1": validity, demodulation, 3x3 luminance variance.  guide = {unit normal, z} (z = -1 marks an invalid pixel), iv = {irr rgb, var}.
__global__ void __launch_bounds__(DN_BX * DN_BY) dn_prep_kernel(DnParams p, const float4* __restrict__ film, const float4* __restrict__ feat,
                                                               float4* __restrict__ guide, float4* __restrict__ iv) {
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= p.width || y >= p.height) return;
    const size_t i = (size_t)y * p.width + x;
    const float4 fm = film[i], fa = feat[2 * i];
    if (!dn_valid(fm, fa)) { guide[i] = make_float4(0.f, 0.f, 0.f, -1.f); return; }
    float s1 = 0.f, s2 = 0.f, cnt = 0.f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= p.height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= p.width) continue;
            const size_t q = (size_t)qy * p.width + qx;
            const float4 qf = film[q], qa = feat[2 * q];
            if (!dn_valid(qf, qa)) continue;
            const f3 c = dn_irr(qf, qa);
            const float l = dn_lum_prep(c.x, c.y, c.z);
            s1 += l; s2 += l * l; cnt += 1.f;
        }
    }
    const float m1 = s1 / cnt, m2 = s2 / cnt;
    const f3 irr = dn_irr(fm, fa);
    const float4 fn = feat[2 * i + 1];
    const float nn = fn.x * fn.x + fn.y * fn.y + fn.z * fn.z;
    const float inv = nn > 0.f ? 1.f / sqrtf(nn) : 0.f;
    guide[i] = make_float4(fn.x * inv, fn.y * inv, fn.z * inv, fn.w);
    iv[i] = make_float4(irr.x, irr.y, irr.z, fmaxf(m2 - m1 * m1, 0.f));
}

// The same level with the emission split and / or the firefly clamp (mcpt_denoise_opts::flags).  SPLIT: the reflected part
// max(mean - E.rgb, 0) is what gets demodulated.  CLAMP: a valid pixel whose luminance l exceeds k times the largest RAW luminance m among
// its valid 3x3 neighbours is scaled to k m, and the variance is taken over the clamped luminances -- a 5x5 footprint of raw inputs per
// pixel, staged in LDS: the block's raw luminance tile with a halo of 2 (68 x 8, l = -inf marks an invalid or outside pixel, which the
// maximum then skips by itself), from it the clamped tile with a halo of 1 (66 x 6), from that the variance.
// Both tiles are rows of consecutive floats read and written at consecutive lanes: no bank conflicts.
#define DN_RW (DN_BX + 4)
#define DN_RH (DN_BY + 4)
#define DN_CW (DN_BX + 2)
#define DN_CH (DN_BY + 2)
template <bool SPLIT>
DEV f3 dn_irr_split(const float4 film, const float4 fa, const float4* __restrict__ emis, size_t i) {
    f3 c = mk3(film.x / film.w, film.y / film.w, film.z / film.w);
    if (SPLIT) { const float4 e = emis[i]; c = mk3(fmaxf(c.x - e.x, 0.f), fmaxf(c.y - e.y, 0.f), fmaxf(c.z - e.z, 0.f)); }
    return mk3(fa.x > 1e-3f ? c.x / fa.x : c.x, fa.y > 1e-3f ? c.y / fa.y : c.y, fa.z > 1e-3f ? c.z / fa.z : c.z);
}

template <bool SPLIT, bool CLAMP>
__global__ void __launch_bounds__(DN_BX * DN_BY) dn_prep_robust_kernel(DnParams p, const float4* __restrict__ film, const float4* __restrict__ feat,
                                                                      const float4* __restrict__ emis, float4* __restrict__ guide, float4* __restrict__ iv) {
    __shared__ float s_raw[DN_RH * DN_RW];
    __shared__ float s_cl[DN_CH * DN_CW];
    const int tid = threadIdx.y * DN_BX + threadIdx.x;
    const int x0 = blockIdx.x * DN_BX, y0 = blockIdx.y * DN_BY;
    for (int k = tid; k < DN_RH * DN_RW; k += DN_BX * DN_BY) {
        const int ty = k / DN_RW, tx = k - ty * DN_RW;
        const int qx = x0 + tx - 2, qy = y0 + ty - 2;
        float l = -INFINITY;
        if (qx >= 0 && qx < p.width && qy >= 0 && qy < p.height) {
            const size_t q = (size_t)qy * p.width + qx;
            const float4 qf = film[q], qa = feat[2 * q];
            if (dn_valid(qf, qa)) {
                const f3 c = dn_irr_split<SPLIT>(qf, qa, emis, q);
                l = dn_lum_prep(c.x, c.y, c.z);
            }
        }
        s_raw[k] = l;
    }
    __syncthreads();
    for (int k = tid; k < DN_CH * DN_CW; k += DN_BX * DN_BY) {
        const int cy = k / DN_CW, cx = k - cy * DN_CW;
        const float l = s_raw[(cy + 1) * DN_RW + cx + 1];
        float lc = l;
        if (CLAMP && l != -INFINITY) {
            float m = -INFINITY;
            for (int dy = 0; dy <= 2; dy++)
                for (int dx = 0; dx <= 2; dx++)
                    if (dx != 1 || dy != 1) m = fmaxf(m, s_raw[(cy + dy) * DN_RW + cx + dx]);
            if (m != -INFINITY && l > p.clamp_k * m) lc = p.clamp_k * m;
        }
        s_cl[k] = lc;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= p.width || y >= p.height) return;
    const size_t i = (size_t)y * p.width + x;
    const float lr = s_raw[(threadIdx.y + 2) * DN_RW + threadIdx.x + 2];
    if (lr == -INFINITY) { guide[i] = make_float4(0.f, 0.f, 0.f, -1.f); return; }
    float s1 = 0.f, s2 = 0.f, cnt = 0.f;
    for (int dy = 0; dy <= 2; dy++)
        for (int dx = 0; dx <= 2; dx++) {
            const float l = s_cl[(threadIdx.y + dy) * DN_CW + threadIdx.x + dx];
            if (l == -INFINITY) continue;
            s1 += l; s2 += l * l; cnt += 1.f;
        }
    const float m1 = s1 / cnt, m2 = s2 / cnt;
    f3 irr = dn_irr_split<SPLIT>(film[i], feat[2 * i], emis, i);
    if (CLAMP) {
        const float lc = s_cl[(threadIdx.y + 1) * DN_CW + threadIdx.x + 1];
        if (lc < lr) { const float sc = lc / lr; irr = mk3(irr.x * sc, irr.y * sc, irr.z * sc); }
    }
    const float4 fn = feat[2 * i + 1];
    const float nn = fn.x * fn.x + fn.y * fn.y + fn.z * fn.z;
    const float inv = nn > 0.f ? 1.f / sqrtf(nn) : 0.f;
    guide[i] = make_float4(fn.x * inv, fn.y * inv, fn.z * inv, fn.w);
    iv[i] = make_float4(irr.x, irr.y, irr.z, fmaxf(m2 - m1 * m1, 0.f));
}

// One a-trous level at step h: 5x5 taps p + h (dx, dy), B3-spline weights times the luminance, normal and depth edge-stopping terms.  The
// centre tap's weight is k(0)^2 (its three edge-stopping factors are 1 by definition).  LAST: remodulate by the albedo and write the film
// {r, g, b, 1}; invalid pixels pass their mean through (count 0: {0, 0, 0, 0}).  SPLIT (with LAST): the emission set aside by the prep pass is
// added back to the remodulated pixel.
template <bool LAST, bool SPLIT>
__global__ void __launch_bounds__(DN_BX * DN_BY) dn_atrous_kernel(DnParams p, int h, const float4* __restrict__ guide, const float4* __restrict__ iv_in,
                                                                 float4* __restrict__ iv_out, const float4* __restrict__ film, const float4* __restrict__ feat,
                                                                 const float4* __restrict__ emis, float4* __restrict__ out) {
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= p.width || y >= p.height) return;
    const size_t i = (size_t)y * p.width + x;
    const float4 gp = guide[i];
    if (gp.w < 0.f) {
        if (LAST) {
            const float4 fm = film[i];
            out[i] = fm.w > 0.f ? make_float4(fm.x / fm.w, fm.y / fm.w, fm.z / fm.w, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const float4 ip = iv_in[i];
    const float lp = dn_lum(ip.x, ip.y, ip.z);
    // variance steering: (1,2,1) x (1,2,1) blur of var over the valid pixels of the 3x3 neighbourhood (step 1 at every level)
    float gv = 0.f, gw = 0.f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= p.height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= p.width) continue;
            const size_t q = (size_t)qy * p.width + qx;
            if (guide[q].w < 0.f) continue;
            const float k = (float)((2 - dx * dx) * (2 - dy * dy));
            gv += k * iv_in[q].w; gw += k;
        }
    }
    const float sigma = p.sigma_c * sqrtf(gv / gw) + 1e-4f;
    const float inv_sigma = 1.f / sigma;
    const float zs = p.sigma_z * (float)h * p.theta * gp.w;
    const float kw[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + h * dy;
        if (qy < 0 || qy >= p.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + h * dx;
            if (qx < 0 || qx >= p.width) continue;
            const size_t q = (size_t)qy * p.width + qx;
            const float4 gq = guide[q];
            if (gq.w < 0.f) continue;
            const float4 iq = iv_in[q];
            float wt = kw[dx + 2] * kw[dy + 2];
            if (dx != 0 || dy != 0) {
                const float dist = sqrtf((float)(dx * dx + dy * dy));
                const float lq = dn_lum(iq.x, iq.y, iq.z);
                const float nd = fmaxf(gp.x * gq.x + gp.y * gq.y + gp.z * gq.z, 0.f);
                const float el = fabsf(lp - lq) * inv_sigma;
                const float ez = fabsf(gp.w - gq.w) / (zs * dist + 1e-4f);
                wt *= __expf(-(el + ez)) * pow_pos(nd, p.sigma_n);
            }
            sw += wt;
            sr += wt * iq.x; sg += wt * iq.y; sb += wt * iq.z;
            sv += wt * wt * iq.w;
        }
    }
    const float inv_w = 1.f / sw;
    const f3 r = mk3(sr * inv_w, sg * inv_w, sb * inv_w);
    if (LAST) {
        const float4 fa = feat[2 * i];
        float4 o = make_float4(fa.x > 1e-3f ? r.x * fa.x : r.x, fa.y > 1e-3f ? r.y * fa.y : r.y, fa.z > 1e-3f ? r.z * fa.z : r.z, 1.f);
        if (SPLIT) { const float4 e = emis[i]; o.x += e.x; o.y += e.y; o.z += e.z; }
        out[i] = o;
    } else {
        iv_out[i] = make_float4(r.x, r.y, r.z, sv * inv_w * inv_w);
    }
}

hipError_t launch_dn_features(const DevScene& sc, uint32_t spp, uint32_t seed_lo, uint32_t seed_hi, float4* feat, float4* emis, hipStream_t stream) {
    const uint32_t n = (uint32_t)sc.cam.width * (uint32_t)sc.cam.height;
    const dim3 grid((n + MCPT_BLOCK - 1) / MCPT_BLOCK), block(MCPT_BLOCK);
    if (feat && emis) hipLaunchKernelGGL((dn_features_kernel<true, true>), grid, block, 0, stream, sc, spp, seed_lo, seed_hi, feat, emis);
    else if (feat) hipLaunchKernelGGL((dn_features_kernel<true, false>), grid, block, 0, stream, sc, spp, seed_lo, seed_hi, feat, emis);
    else if (emis) hipLaunchKernelGGL((dn_features_kernel<false, true>), grid, block, 0, stream, sc, spp, seed_lo, seed_hi, feat, emis);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_dn_filter(const DnParams& p, uint32_t levels, const float4* film, const float4* feat, const float4* emis, float4* guide, float4* iv0,
                            float4* iv1, float4* out, hipStream_t stream) {
    const dim3 grid((p.width + DN_BX - 1) / DN_BX, (p.height + DN_BY - 1) / DN_BY), block(DN_BX, DN_BY);
    const bool split = emis != nullptr, clamp = p.clamp_k > 0.f;
    if (split && clamp) hipLaunchKernelGGL((dn_prep_robust_kernel<true, true>), grid, block, 0, stream, p, film, feat, emis, guide, iv0);
    else if (split) hipLaunchKernelGGL((dn_prep_robust_kernel<true, false>), grid, block, 0, stream, p, film, feat, emis, guide, iv0);
    else if (clamp) hipLaunchKernelGGL((dn_prep_robust_kernel<false, true>), grid, block, 0, stream, p, film, feat, emis, guide, iv0);
    else hipLaunchKernelGGL(dn_prep_kernel, grid, block, 0, stream, p, film, feat, guide, iv0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    float4* src = iv0; float4* dst = iv1;
    for (uint32_t lv = 0; lv < levels; lv++) {
        const int h = 1 << lv;
        if (lv + 1 < levels) hipLaunchKernelGGL((dn_atrous_kernel<false, false>), grid, block, 0, stream, p, h, guide, src, dst, film, feat, emis, out);
        else if (split) hipLaunchKernelGGL((dn_atrous_kernel<true, true>), grid, block, 0, stream, p, h, guide, src, dst, film, feat, emis, out);
        else hipLaunchKernelGGL((dn_atrous_kernel<true, false>), grid, block, 0, stream, p, h, guide, src, dst, film, feat, emis, out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        float4* t = src; src = dst; dst = t;
    }
    return hipSuccess;
}
