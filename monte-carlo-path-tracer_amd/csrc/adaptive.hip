// gfx950 kernels of adaptive sampling: the per-tile error estimate of two half films, the compaction of the tiles that still
// need samples into a list in ascending tile order, and the merge of the half films into the context film.  They run on the context's stream
// between the render passes of mcpt_render_adaptive and touch nothing the path kernels read.  Plain C++ loads and vector stores only.
#include "adaptive.h"

// ---------------------------------------------------------------------------------------------- tile error
// One wave64 per 8x8 tile, lane = pixel at (lane & 7, lane >> 3) of the tile -- the renderer's work-item layout.  Per in-image pixel
//   e_p = sum over rgb of |sqrt(clamp(H / nH, 0, 1)) - sqrt(clamp(O / nO, 0, 1))|      (a count of 0 reads as a mean of 0)
// how different the two halves look after mcpt_tonemap's clamp and square root.  E_t = max e_p over the tile, c_t = nH + nO of the tile's
// first pixel (the counts are uniform within a tile under mcpt_render_adaptive).  Active: E_t >= threshold && c_t < max_spp.
__device__ __forceinline__ float ad_display(float sum, float n) {
    const float m = n > 0.f ? __fdiv_rn(sum, n) : 0.f;
    // clamp as tonemap_kernel does (NaN -> 0 through fmaxf); the square root in fp64, rounded once to fp32: a correctly rounded fp32 root
    // (53 >= 2 * 24 + 2), so exact squares such as 0.25 or 0.5625 give exact roots and ties at the threshold are decided exactly
    return (float)sqrt((double)fminf(fmaxf(m, 0.f), 1.f));
}

__global__ void __launch_bounds__(AD_BLOCK) ad_error_kernel(const float4* __restrict__ h, const float4* __restrict__ o, int width, int height,
                                                            uint32_t tiles_x, uint32_t n_tiles, float threshold, uint32_t max_spp,
                                                            float* __restrict__ err, uint32_t* __restrict__ flags, uint4* __restrict__ block_counts) {
    __shared__ uint32_t s_act[AD_TILES_PER_BLOCK], s_hot[AD_TILES_PER_BLOCK], s_px[AD_TILES_PER_BLOCK];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x * AD_TILES_PER_BLOCK + wv;
    float e = 0.f, count = 0.f;
    bool in = false;
    if (tile < n_tiles) {
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
        in = px < (uint32_t)width && py < (uint32_t)height;
        if (in) {
            const size_t i = (size_t)py * (uint32_t)width + px;
            const float4 a = h[i], b = o[i];
            e = fabsf(ad_display(a.x, a.w) - ad_display(b.x, b.w)) + fabsf(ad_display(a.y, a.w) - ad_display(b.y, b.w)) +
                fabsf(ad_display(a.z, a.w) - ad_display(b.z, b.w));
            count = a.w + b.w;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) e = fmaxf(e, __shfl_xor(e, m, 64));
    const unsigned long long in_mask = __ballot(in);
    const float c_t = __shfl(count, 0, 64);                            // lane 0 = the tile's first pixel, always inside the image
    if (lane == 0) {
        const bool valid = tile < n_tiles;
        const bool hot = valid && e >= threshold;
        const bool active = hot && c_t < (float)max_spp;
        if (valid) { err[tile] = e; flags[tile] = active ? 1u : 0u; }
        s_act[wv] = active ? 1u : 0u; s_hot[wv] = hot ? 1u : 0u;
        s_px[wv] = active ? (uint32_t)__popcll(in_mask) : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint4 c = make_uint4(0u, 0u, 0u, 0u);
        for (uint32_t k = 0; k < AD_TILES_PER_BLOCK; k++) { c.x += s_act[k]; c.y += s_hot[k]; c.z += s_px[k]; }
        block_counts[blockIdx.x] = c;
    }
}

// ---------------------------------------------------------------------------------------------- compaction
// One block: thread t sums a contiguous run of the per-block counts, an exclusive scan over the 1024 runs in LDS gives every error block the
// offset of its first active tile in the list; the totals go to `tot`.
__global__ void __launch_bounds__(AD_SCAN_BLOCK) ad_scan_kernel(const uint4* __restrict__ block_counts, uint32_t nb, uint32_t* __restrict__ offsets,
                                                                AdTotals* __restrict__ tot) {
    __shared__ uint32_t s_scan[AD_SCAN_BLOCK];
    __shared__ uint32_t s_hot, s_px;
    const uint32_t t = threadIdx.x;
    if (t == 0) { s_hot = 0u; s_px = 0u; }
    const uint32_t per = (nb + AD_SCAN_BLOCK - 1) / AD_SCAN_BLOCK;
    const uint32_t lo = min(nb, t * per), hi = min(nb, lo + per);
    uint32_t act = 0u, hot = 0u, px = 0u;
    for (uint32_t b = lo; b < hi; b++) { const uint4 c = block_counts[b]; act += c.x; hot += c.y; px += c.z; }
    s_scan[t] = act;
    __syncthreads();
    atomicAdd(&s_hot, hot); atomicAdd(&s_px, px);
    for (uint32_t d = 1; d < AD_SCAN_BLOCK; d <<= 1) {                // Hillis-Steele inclusive scan
        const uint32_t v = t >= d ? s_scan[t - d] : 0u;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    uint32_t run = s_scan[t] - act;                                     // exclusive
    for (uint32_t b = lo; b < hi; b++) { offsets[b] = run; run += block_counts[b].x; }
    if (t == AD_SCAN_BLOCK - 1) {
        AdTotals r; r.n_active = s_scan[t]; r.n_hot = s_hot; r.active_pixels = s_px; r.pad = 0u;
        *tot = r;
    }
}

// One thread per error block: its active tiles, in tile order, from its offset on.
__global__ void __launch_bounds__(256) ad_scatter_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offsets, uint32_t nb,
                                                         uint32_t n_tiles, uint32_t* __restrict__ list) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    uint32_t at = offsets[b];
    for (uint32_t k = 0; k < AD_TILES_PER_BLOCK; k++) {
        const uint32_t tile = b * AD_TILES_PER_BLOCK + k;
        if (tile < n_tiles && flags[tile]) list[at++] = tile;
    }
}

// ---------------------------------------------------------------------------------------------- merge
__global__ void __launch_bounds__(256) ad_merge_kernel(float4* __restrict__ film, const float4* __restrict__ h, const float4* __restrict__ o, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 f = film[i], a = h[i], b = o[i];
    film[i] = make_float4(f.x + (a.x + b.x), f.y + (a.y + b.y), f.z + (a.z + b.z), f.w + (a.w + b.w));
}

// ---------------------------------------------------------------------------------------------- launchers
hipError_t launch_ad_error_compact(const float4* h, const float4* o, int width, int height, float threshold, uint32_t max_spp,
                                   float* err, uint32_t* list, const AdScratch& s, hipStream_t stream) {
    const uint32_t tiles_x = (uint32_t)(width + 7) / 8u, tiles_y = (uint32_t)(height + 7) / 8u, n_tiles = tiles_x * tiles_y;
    const uint32_t nb = ad_blocks(n_tiles);
    hipLaunchKernelGGL(ad_error_kernel, dim3(nb), dim3(AD_BLOCK), 0, stream, h, o, width, height, tiles_x, n_tiles, threshold, max_spp, err, s.flags, s.block_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ad_scan_kernel, dim3(1), dim3(AD_SCAN_BLOCK), 0, stream, s.block_counts, nb, s.block_offsets, s.totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ad_scatter_kernel, dim3((nb + 255) / 256), dim3(256), 0, stream, s.flags, s.block_offsets, nb, n_tiles, list);
    return hipGetLastError();
}

hipError_t launch_ad_merge(float4* film, const float4* h, const float4* o, uint32_t n_pixels, hipStream_t stream) {
    hipLaunchKernelGGL(ad_merge_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, film, h, o, n_pixels);
    return hipGetLastError();
}
