// Launchers of adaptive sampling (adaptive.hip), called from mcpt_api.cpp.  DESIGN.md §11 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include "device_scene.h"

#define AD_BLOCK 256                   // threads of the error kernel: 4 wave64 = 4 tiles per block
#define AD_TILES_PER_BLOCK (AD_BLOCK / 64)
#define AD_SCAN_BLOCK 1024             // the single block of the scan kernel

// What one error + compaction round leaves for the host (one 16-B read-back per pass).
struct AdTotals {
    uint32_t n_active;                 // tiles with E_t >= threshold && c_t < max_spp: the length of the active list
    uint32_t n_hot;                    // tiles with E_t >= threshold (active or capped)
    uint32_t active_pixels;            // in-image pixels of the active tiles
    uint32_t pad;
};

// Device scratch of a round: per block of AD_TILES_PER_BLOCK tiles one uint4 of counts {active, hot, active pixels, 0} and one exclusive
// offset; per tile one active flag.
struct AdScratch {
    uint4* block_counts;
    uint32_t* block_offsets;
    uint32_t* flags;
    AdTotals* totals;
};
inline uint32_t ad_blocks(uint32_t n_tiles) { return (n_tiles + AD_TILES_PER_BLOCK - 1) / AD_TILES_PER_BLOCK; }

// Tile error E_t of the half films h and o (width * height {sum rgb, count} each) for every tile, the active list in ascending tile order
// (list: capacity n_tiles) and the totals.  Three launches on `stream`: error, scan, scatter.
hipError_t launch_ad_error_compact(const float4* h, const float4* o, int width, int height, float threshold, uint32_t max_spp,
                                   float* err, uint32_t* list, const AdScratch& s, hipStream_t stream);
// film += h + o, per pixel
hipError_t launch_ad_merge(float4* film, const float4* h, const float4* o, uint32_t n_pixels, hipStream_t stream);
