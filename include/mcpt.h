/* mcpt.h -- C ABI of the MI355X-native path-tracing hot path (libmcpt_hip.so).
 *
 * Drop-in boundary for laizesheng1/Monte-Carlo-Path-Tracer's `Render` class: everything a caller hands
 * over is the reference's own `Model` data (src/model.h:51-60) as plain pointers + counts, and what it
 * gets back is the reference's film accumulator `Pixels{vec3 color; float spp}` (src/Scene.h:7-12).
 * The reference has no FFI layer (it is one C++ executable); the entry points below are what a binding
 * for its Render::Render / Render::render pair would call -- see INTEGRATION.md for the ~40-line
 * `Render` replacement a maintainer would add.
 *
 * Plain C, no HIP / torch / STL types.  Every function returns an mcpt_status; nothing throws.
 * There is NO CPU fallback: without a usable HIP device mcpt_create fails with MCPT_ERR_NO_DEVICE.
 */
#ifndef MCPT_H
#define MCPT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCPT_ABI_VERSION 4

typedef enum mcpt_status {
    MCPT_OK = 0,
    MCPT_ERR_INVALID_ARG = 1,   /* null pointer, out-of-range index in `face`, zero-sized image ... */
    MCPT_ERR_NO_DEVICE = 2,     /* no HIP device / device ordinal out of range */
    MCPT_ERR_HIP = 3,           /* a HIP runtime call failed; see mcpt_last_error() */
    MCPT_ERR_NO_LIGHTS = 4,     /* scene has no emissive triangle (reference: UB, Render.cpp:204-206) */
    MCPT_ERR_BVH_DEPTH = 5,     /* BVH deeper than the traversal stack the kernels were built for */
    MCPT_ERR_UNSUPPORTED = 6
} mcpt_status;

/* Texture (src/model.h:21-30): `image_color` as w*h RGB fp32 texels, row 0 first as stb_image returns
 * them (src/model.cpp:8-23).  A 1x1 texture is the constant Kd colour (model.cpp:25-28,32-35). */
typedef struct mcpt_texture {
    int32_t width, height;
    const float* rgb;
} mcpt_texture;

/* Material (src/model.h:32-40).  Tr and Ni are parsed by the reference but never read (SURVEY A-21). */
typedef struct mcpt_material {
    double ks[3];
    double ns;
    double radiance[3];   /* from the XML <light mtlname radiance> (model.cpp:181-182) */
    int32_t map_kd;       /* index into textures[] (Map_Kd) */
    int32_t reserved;
} mcpt_material;

/* CameraInfo (src/model.h:42-49) */
typedef struct mcpt_camera {
    double eye[3], lookat[3], up[3];
    double fovy;          /* vertical field of view in degrees (Render.cpp:73) */
    int32_t width, height;
} mcpt_camera;

/* Model (src/model.h:51-60) */
typedef struct mcpt_scene_desc {
    const double* vertex;   uint32_t n_vertex;    /* xyz per vertex   (Model::vertex)  */
    const double* normal;   uint32_t n_normal;    /* xyz per normal   (Model::normal)  */
    const double* texcoord; uint32_t n_texcoord;  /* uv per entry     (Model::texture) */
    const int32_t* face;    uint32_t n_face;      /* 12 ints per face = glm::imat3x4 (Model::face): for each of the
                                                     3 corners {vertex idx, normal idx, texcoord idx, material idx},
                                                     0-based; the material of a face is corner 0's (Render.cpp:33) */
    const mcpt_material* materials; uint32_t n_materials;
    const mcpt_texture* textures;   uint32_t n_textures;
    mcpt_camera camera;
} mcpt_scene_desc;

/* integrators */
#define MCPT_INTEGRATOR_MIS            0u  /* Render::ray_tracing(Ray&)      Render.cpp:111-175 -- the one that ships */
#define MCPT_INTEGRATOR_RECURSIVE_NEE  1u  /* Render::ray_tracing(Ray&,int)  Render.cpp:83-109 + sample_light :177-200 */

/* flags */
#define MCPT_FLAG_CORRECT_SHADOW_T2   0x1u  /* do NOT reproduce the reference's light self-occlusion (SURVEY A-9):
                                               the sampled light triangle is ignored by its own shadow ray */
#define MCPT_FLAG_DETERMINISTIC       0x2u  /* one thread owns a pixel for the whole call: no float atomics,
                                               bit-reproducible accumulator, worse tail balance */
#define MCPT_FLAG_COUNT_TRAVERSAL     0x4u  /* also count box tests / triangle tests / shaded hits (roofline input) */
#define MCPT_FLAG_GPU_BVH_BUILD       0x8u  /* build the BVH on the device -- SAH-costed agglomerative clustering over the Morton order (PLOC) --
                                               instead of the host's binned-SAH builder: ~2x faster construction, within ~5 % of the host
                                               tree's render speed; rendered results are the same (closest hit does not depend on the tree) */

#define MCPT_FLAG_REFERENCE_TIE_ORDER 0x10u /* among triangles hit at EXACTLY the same distance the one that comes first in the reference's own
                                               BVH::triangles order wins (BVH.cpp:15-54 + :95-113: left, right, own triangles; `t < t2` strict) --
                                               mcpt_create then replays the reference's midpoint partition to learn that order (O(n log n) on the
                                               host).  Default: the lowest index in this library's leaf order wins (any fixed rule gives the same
                                               image up to measure-zero ties; this flag is for tie-break-exact known-answer tests).
                                               The tie rule lives in the production pipeline only (wavefront trace kernel, MCPT_INTEGRATOR_MIS): mcpt_create
                                               refuses the flag with MCPT_ERR_UNSUPPORTED for MCPT_INTEGRATOR_RECURSIVE_NEE and for the cross-check megakernel
                                               (MCPT_PIPELINE=mega), whose binary-tree traversal lets the first triangle IT tests win -- as does mcpt_probe_trace */

#define MCPT_FLAG_DYNAMIC             0x20u /* mcpt_create keeps what mcpt_update_vertices needs: per triangle its vertex and normal indices, the level structure
                                               of both trees and refit scratch (counted in device_bytes); without it that call returns
                                               MCPT_ERR_UNSUPPORTED, and device_bytes and every stream are what they are without the flag */

typedef struct mcpt_opts {
    uint32_t struct_size;       /* = sizeof(mcpt_opts) */
    int32_t  device;            /* HIP device ordinal */
    uint32_t max_depth;         /* 0 = unbounded like the reference; N = stop before shading vertex N
                                   (`for (bounces = 0; bounces < N; ...)`, Render.cpp:116) */
    uint32_t integrator;        /* MCPT_INTEGRATOR_* */
    uint32_t flags;             /* MCPT_FLAG_* */
    uint32_t samples_per_item;  /* samples of one pixel traced back-to-back by one lane; 0 = auto */
    uint32_t reserved[4];
} mcpt_opts;

typedef struct mcpt_counters {
    uint64_t paths;             /* pixel-samples finished */
    uint64_t rays_primary;      /* camera rays traced (Render.cpp:64) */
    uint64_t rays_continuation; /* BSDF-sampled rays traced (Render.cpp:144); the reference's duplicate re-trace
                                   at Render.cpp:118 is never performed and never counted */
    uint64_t rays_shadow;       /* shadow rays traced, i.e. light samples with pdf != 0 (Render.cpp:125) */
    uint64_t box_tests;         /* AABB slab tests        (only with MCPT_FLAG_COUNT_TRAVERSAL) */
    uint64_t tri_tests;         /* triangle tests         (only with MCPT_FLAG_COUNT_TRAVERSAL) */
    uint64_t shaded_hits;       /* hits whose shading record was fetched (only with COUNT_TRAVERSAL) */
    uint64_t texel_fetches;     /* image-texture lookups  (only with COUNT_TRAVERSAL) */
    uint64_t self_shadow_tests; /* light samples that reached the fp64 self-hit predicate (A-9) */
    uint64_t self_shadow_hits;  /* ... and were rejected by it */
    double   kernel_ms;         /* HIP-event duration of all render kernels of the LAST mcpt_render call */
    double   kernel_ms_total;   /* sum of those durations over all mcpt_render calls since the last reset */
    uint64_t launches;          /* mcpt_render calls since the last reset */
    double   trace_ms_total;    /* wavefront pipeline, detailed timing on: summed duration of the traversal kernel ... */
    double   shade_ms_total;    /* ... and of the shade kernel since the last reset (0 when detailed timing is off) */
    uint64_t iterations;        /* [shade, trace] iterations since the last reset (each is one launch of either kernel) */
    uint64_t stack_spills;      /* traversal-stack entries that left LDS for the global overflow area (only with COUNT_TRAVERSAL) */
    uint64_t debug[4];          /* diagnostic library builds only (tools/sched_stats.py); 0 otherwise */
} mcpt_counters;

typedef struct mcpt_scene_info {
    uint32_t n_tris, n_lights, n_nodes, bvh_depth, max_leaf;
    uint32_t width, height;
    uint64_t device_bytes;      /* HBM held by the scene (nodes + triangle streams + textures + accumulator + path pools allocated so far) */
    double   bvh_build_ms, upload_ms;
    /* ABI 3: the wide tree the wavefront trace kernel walks (8 children per node; wide_width is always 8 since round 4, when the round-2 4-wide kernel was removed) */
    uint32_t wide_width, wide_nodes, wide_depth;
    uint32_t bvh_builder;       /* who made the tree in use (this word was reserved0, always 0, so 0 keeps its meaning): 0 = the host SAH builder (always so for
                                   mcpt_check_scene and for scenes of at most 2 triangles); 1 = the device PLOC builder of MCPT_FLAG_GPU_BVH_BUILD, its
                                   tree kept; 2 = the device builder ran and its result was discarded -- the tree came out deeper than the context's
                                   kernels can walk (63 levels, 255 on a wavefront-only context), or the builder gave up (more than 4096 rounds) --
                                   and the host SAH tree is in use.  A clone reports its source's value. */
    uint64_t traversal_bytes;   /* wide nodes + triangle intersection records: what a ray's traversal can touch */
    double   centre[3];         /* device coordinates are relative to this point (the fp64 centre of the scene's bounding box) */
    uint64_t wide_tree_hash;    /* FNV-1a over the wide tree's records and the leaf order: equal hashes = the same tree and triangle order
                                   (how the tests tell that the device collapse reproduces the host collapse bit for bit) */
} mcpt_scene_info;

typedef struct mcpt_ctx mcpt_ctx;

/* ---- lifecycle -------------------------------------------------------------------------------------- */
/* Replaces Render::Render(Model&) (Render.cpp:5-10): copies what it needs from `scene` (the caller may free it
 * afterwards, like the reference's by-value `model` member, Render.h:57), flattens faces into triangles and
 * collects emissive ones as lights (tranform_triangle, Render.cpp:12-44), builds the BVH (BVH.cpp:6-54) and
 * uploads everything to HBM.  Allocates a zeroed width*height accumulator.
 * Refused with MCPT_ERR_INVALID_ARG, the face named in mcpt_last_error: a vertex coordinate or a texture coordinate that a face uses and that is
 * not finite or exceeds 1e18 in magnitude (with the barycentrics of an accepted hit the interpolated uv is then always finite; a texcoord that is
 * not a number would make the texture lookup convert NaN to an integer).  Refused likewise: a camera whose cross(front, up) is zero or not finite
 * -- `up` parallel to the view direction or zero, eye == lookat, a field that is not finite --, since right = cross / |cross| would make every ray
 * NaN.  An `up` that is merely not unit or not orthogonal to the view is used as given. */
mcpt_status mcpt_create(const mcpt_scene_desc* scene, const mcpt_opts* opts, mcpt_ctx** out_ctx);
mcpt_status mcpt_destroy(mcpt_ctx* ctx);
/* A second context for the same scene on device `device` (may equal the source's): the scene streams are copied device to device, nothing is
 * flattened or built again.  The clone has its own film, counters, stream and options (those of `src`, device replaced). */
mcpt_status mcpt_clone_to_device(mcpt_ctx* src, int32_t device, mcpt_ctx** out_ctx);
/* Host-only half of mcpt_create: validates `scene` (same error codes) and runs the same flatten + BVH build, without
 * touching a device.  Fills n_tris / n_lights / n_nodes / bvh_depth / max_leaf / width / height / bvh_build_ms. */
mcpt_status mcpt_check_scene(const mcpt_scene_desc* scene, mcpt_scene_info* out_info);
mcpt_status mcpt_get_scene_info(const mcpt_ctx* ctx, mcpt_scene_info* out);
const char* mcpt_last_error(void);   /* thread-local, valid until the next failing call on this thread */
uint32_t    mcpt_abi_version(void);

/* ---- the hot path ----------------------------------------------------------------------------------- */
/* Replaces `spp` consecutive calls of Render::render(Scene&) (Render.cpp:56-69): adds `spp` samples to EVERY
 * pixel of the device accumulator (sum rgb + sample count, NaN components zeroed first like Scene::set_Pixel,
 * Scene.cpp:12-21).  Samples are numbered first_sample .. first_sample+spp-1; a sample's random numbers depend
 * only on (seed, pixel, sample index), so any split of a sample range over calls, GPUs or ranks yields the
 * same image up to fp32 summation order.  Asynchronous on the context's stream. */
mcpt_status mcpt_render(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample);
/* The same for the pixels of ONE interleaved share of the image only: 8x8-pixel tiles are numbered row-major and this call renders the
 * tiles t with t % tile_mod == tile_rem (every other pixel of the film is left untouched).  GPU g of G renders (G, g): the
 * "pixel-tile shard" of BASELINE.json's bathroom2 configuration -- the films of the G shares are disjoint and their sum (the same RCCL
 * all-reduce as for sample sharding) is the full image.  (1, 0) = mcpt_render. */
mcpt_status mcpt_render_tiles(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample, uint32_t tile_mod, uint32_t tile_rem);
/* The same for an arbitrary set of tiles: `tiles` holds n_tiles distinct tile numbers (row-major over ceil(w/8) x ceil(h/8), as for
 * mcpt_render_tiles), in any order; every other pixel of the film is left untouched.  The list is validated before any device work (an
 * index out of range, a duplicate, or a NULL list with n_tiles > 0: MCPT_ERR_INVALID_ARG) and copied to the device in stream order, so the
 * caller may reuse it as soon as the call returns.  n_tiles = 0 does nothing.  Asynchronous on the context's stream. */
mcpt_status mcpt_render_tile_list(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample, const uint32_t* tiles, uint32_t n_tiles);
mcpt_status mcpt_sync(mcpt_ctx* ctx);

/* Film = Scene::m_Pixels (Scene.h:7-12,25): width*height records {r_sum, g_sum, b_sum, spp}, index y*width+x,
 * y = 0 at the image bottom (Render.cpp:63, Scene.cpp:14). */
mcpt_status mcpt_read_accum(mcpt_ctx* ctx, float* rgba_host);     /* synchronises, then D2H */
mcpt_status mcpt_write_accum(mcpt_ctx* ctx, const float* rgba_host);   /* resume / merge */
mcpt_status mcpt_clear_accum(mcpt_ctx* ctx);
/* Scene::getPixelsColor (Scene.cpp:23-33) on the device: mean -> clamp[0,1] -> pow(.,0.5) -> *255.99 -> u8.
 * flip_y != 0 additionally applies Scene::save_image's vertical flip (Scene.cpp:40-46).
 * The mean is sum / count in fp32: a NaN mean gives 0, +inf gives 255, negative and -inf give 0, count 0 with sum 0 gives 0 (0 / 0 is NaN). */
mcpt_status mcpt_tonemap(mcpt_ctx* ctx, uint8_t* rgb_host, int flip_y);
/* ABI 4: the same without the last host copy -- *out_rgb points at the context's own pinned host image (width * height * 3 bytes), valid until
 * the next tonemap call on this context or mcpt_destroy.  This is Scene::getPixelsColor's own contract (Scene.cpp:23-33 returns a pointer
 * into a vector the next call overwrites), and what the reference's loop calls after EVERY render(scene) (main.cpp:26-33). */
mcpt_status mcpt_tonemap_map(mcpt_ctx* ctx, int flip_y, const uint8_t** out_rgb);

/* mcpt_tonemap of any film of this context's size resident on its device (e.g. several devices' films summed into a scratch buffer). */
mcpt_status mcpt_tonemap_buffer(mcpt_ctx* ctx, const void* device_rgba, uint8_t* rgb_host, int flip_y);
mcpt_status mcpt_get_counters(mcpt_ctx* ctx, mcpt_counters* out);  /* synchronises */
mcpt_status mcpt_reset_counters(mcpt_ctx* ctx);

/* ---- denoised preview ---------------------------------------------------------------------------------- */
/* Edge-avoiding a-trous wavelet filter of a film, guided by first-hit feature buffers.  The features are rendered by
 * mcpt_render_features from the camera rays mcpt_render(ctx, ..., seed, first_sample = 0) traces for samples 0 .. spp-1: per pixel
 * 8 floats {albedo r, g, b, coverage f, normal x, y, z, depth z} (albedo = kd + ks of non-emissive first hits summed / spp, f = their
 * share of the spp, normal = sum of camera-facing shading normals / max(hits, 1), z = mean hit distance, 0 without hits).  They depend
 * on the scene, the camera, spp and seed only: clearing or writing the film keeps them; a clone starts without them.
 * mcpt_denoise filters a film of {sum rgb, count} records (NULL = the context film, which it never writes) into the context's
 * denoised film {r, g, b, 1} (count 0: {0, 0, 0, 0}) -- a mean, so mcpt_tonemap_buffer displays it as it is.
 *
 * Two opt-in flags (flags = 0 is the filter as it always was):
 *  - MCPT_DENOISE_SPLIT_EMISSION keeps emitted light apart from reflected light.  The emission buffer E holds per pixel {sum of the radiance
 *    of the first hits on emitters / spp, their share of the spp}, from the camera rays of the features the context holds (same spp, same
 *    seed).  A valid pixel's mean c becomes max(c - E.rgb, 0) per channel before it is divided by the albedo; the filter works on that
 *    reflected part and adds E.rgb back when it writes the pixel.  The subtraction is exact up to rounding when the film holds the feature
 *    samples (same seed, samples 0 .. spp-1); otherwise E estimates the same expectation and the clamp at 0 absorbs the rest.
 *    The first call with this flag allocates E (16 B per pixel, counted in device_bytes) and renders it for the features held; afterwards
 *    every feature render of the context fills it in the same pass.  E is dropped with the features; a clone starts without the buffer.
 *  - MCPT_DENOISE_CLAMP_FIREFLIES scales a valid pixel whose demodulated luminance l exceeds k times m, the largest unclamped l among the
 *    valid pixels of its 3x3 neighbourhood, by k m / l before the filter (k = firefly_clamp); the variance that steers the luminance term
 *    is taken over the clamped values.  A pixel without a valid neighbour is never clamped. */
#define MCPT_DENOISE_SPLIT_EMISSION  0x1u
#define MCPT_DENOISE_CLAMP_FIREFLIES 0x2u
#define MCPT_DENOISE_DEFAULT_FIREFLY_CLAMP 4.0f
typedef struct mcpt_denoise_opts {
    uint32_t struct_size;                           /* = sizeof(mcpt_denoise_opts) */
    uint32_t iterations;                            /* a-trous levels, 0 = default 5, max 10 */
    float sigma_color, sigma_normal, sigma_depth;   /* 0 = default (4, 128, 4) */
    uint32_t flags;                                 /* MCPT_DENOISE_*; an unknown bit is MCPT_ERR_INVALID_ARG */
    float firefly_clamp;                            /* k of the clamp: 0 = default (MCPT_DENOISE_DEFAULT_FIREFLY_CLAMP), else finite and >= 1 */
    uint32_t reserved[1];
} mcpt_denoise_opts;
mcpt_status mcpt_render_features(mcpt_ctx* ctx, uint32_t spp, uint64_t seed);          /* 1 <= spp <= 64, asynchronous */
mcpt_status mcpt_read_features(mcpt_ctx* ctx, float* out8);                            /* synchronises, then D2H: width*height*8 floats */
mcpt_status mcpt_denoise(mcpt_ctx* ctx, const void* device_rgba, const mcpt_denoise_opts* opts);  /* NULL film = ctx film; NULL opts = defaults; asynchronous */
mcpt_status mcpt_read_denoised(mcpt_ctx* ctx, float* rgba_host);                       /* synchronises, then D2H: width*height*4 floats */
mcpt_status mcpt_denoised_device_ptr(mcpt_ctx* ctx, void** out_device_rgba);           /* the denoised film on the device (after a first mcpt_denoise) */
mcpt_status mcpt_read_emission(mcpt_ctx* ctx, float* out4);                            /* synchronises, then D2H: width*height*4 floats; MCPT_ERR_INVALID_ARG when no emission is held */
/* The filter alone on caller data of this context's film size: a film of width * height {sum rgb, count} records, features as
 * mcpt_read_features returns them, and -- with MCPT_DENOISE_SPLIT_EMISSION, and only then -- an emission buffer as mcpt_read_emission returns
 * it (NULL otherwise).  The options are checked as mcpt_denoise checks them (NULL = defaults); the depth term's pixel angle is that of the
 * context's camera.  out gets what mcpt_read_denoised would return.  Synchronous; works in scratch buffers: the context's features, emission,
 * denoised film and device_bytes are neither read nor written.
 * PRECONDITION: every feature depth z >= 0.  The filter marks an invalid pixel for its later passes by a negative depth, so a valid pixel
 * with z < 0 would be filtered as valid by the first pass and skipped as invalid by the others (mcpt_render_features never writes one:
 * z is a mean of hit distances >= 1e-4, or 0).  A depth < 0, a non-finite feature or emission value, a null film, features or output, an
 * emission buffer without the flag or the flag without one: MCPT_ERR_INVALID_ARG, and out is not written. */
mcpt_status mcpt_probe_denoise(mcpt_ctx* ctx, const float* film_rgba_host, const float* feat8_host, const float* emis4_host,
                               const mcpt_denoise_opts* opts, float* out_rgba_host);

/* ---- adaptive sampling ------------------------------------------------------------------------------------------- */
/* Samples go where the image is still noisy, per 8x8 tile.  During a call the samples go into two internal half films H and O (the first and
 * the second half of every pass's sample range).  Per in-image pixel e_p = sum over rgb of |sqrt(clamp(H/nH, 0, 1)) - sqrt(clamp(O/nO, 0, 1))|
 * -- how different the two halves look after mcpt_tonemap -- and per tile E_t = max e_p, c_t = nH + nO.  A tile is active while
 * E_t >= threshold && c_t < max_spp.  Pass 0 gives every tile min_spp samples; each later pass doubles the active tiles' count (the last one
 * stops at max_spp).  At the end H + O is added to the bound film, whatever it held before.  Every tile t ends with samples
 * first_sample .. first_sample + N_t - 1, N_t in {min_spp * 2^k} and {max_spp}: the same image as mcpt_render_tile_list of N_t samples, up to
 * fp32 summation order.  One small read-back and one synchronisation per pass; the call returns when the merge has been enqueued.
 * The counters account the call's rays and paths as usual; it counts as ONE launch, and its kernel_ms is the device time from its first to
 * its last operation, the per-pass host round trips included. */
typedef struct mcpt_adaptive_opts {
    uint32_t struct_size;   /* = sizeof(mcpt_adaptive_opts) */
    uint32_t min_spp;       /* samples every tile gets in pass 0; even, >= 2; 0 = default 16 */
    uint32_t max_spp;       /* cap per tile, >= min_spp; 0 = default 1024 */
    float    threshold;     /* finite, > 0; 0 = default (MCPT_ADAPTIVE_DEFAULT_THRESHOLD) */
    uint32_t reserved[4];
} mcpt_adaptive_opts;
typedef struct mcpt_adaptive_stats {
    uint32_t struct_size, passes;           /* passes: render passes, pass 0 included */
    uint64_t pixel_samples;                 /* samples added to in-image pixels by this call */
    uint32_t tiles_converged, tiles_capped; /* E_t < threshold / E_t >= threshold at max_spp */
    uint32_t reserved[4];
} mcpt_adaptive_stats;
#define MCPT_ADAPTIVE_DEFAULT_THRESHOLD 0.25f
/* opts NULL = all defaults; out_stats may be NULL.  Invalid options return MCPT_ERR_INVALID_ARG before any device work, as does
 * first_sample + max_spp > 2^32. */
mcpt_status mcpt_render_adaptive(mcpt_ctx* ctx, uint64_t seed, uint32_t first_sample, const mcpt_adaptive_opts* opts, mcpt_adaptive_stats* out_stats);
/* Synchronises, then D2H: tiles_y * tiles_x floats, E_t of the last pass of the last mcpt_render_adaptive call. */
mcpt_status mcpt_read_tile_error(mcpt_ctx* ctx, float* out);
/* The error and compaction kernels on caller films of this context's size (width * height {sum rgb, count} each): out_err gets E_t of every
 * tile, out_list (room for tiles_y * tiles_x entries) the active tiles in ascending order, *out_n their number.  Synchronous. */
mcpt_status mcpt_probe_tile_error(mcpt_ctx* ctx, const float* h_rgba_host, const float* o_rgba_host, float threshold, uint32_t max_spp,
                                  float* out_err, uint32_t* out_list, uint32_t* out_n);

/* ---- live scenes: camera moves and vertex updates --------------------------------------------------------------------- */
/* Both calls below are ordered like any other call on the context: renders enqueued before them see the old scene, renders enqueued after
 * them the new one (their device work runs on the context's stream, which every sub-pipeline forks from and joins).  Neither touches the film
 * or the counters: the caller clears the film (mcpt_clear_accum) when the old samples no longer belong to the picture.  The first-hit feature
 * buffers and the tile error of the last adaptive call describe the old scene: after either call the context is without them, as a clone is
 * (mcpt_denoise / mcpt_read_features / mcpt_read_tile_error answer as on a context that never had them). */

/* New camera for the same film size.  camera->width / height must equal the context's (else MCPT_ERR_INVALID_ARG, nothing changed);
 * eye == lookat, a non-finite field, or an `up` whose cross(front, up) is zero or not finite (parallel to the view direction, or zero; see
 * mcpt_create): MCPT_ERR_INVALID_ARG, nothing changed.  Every other call that takes a camera for a live context refuses the same.  Works on
 * every context, MCPT_FLAG_DYNAMIC or not.  The constants are formed by the function mcpt_create uses: the same camera gives the same rays, bit
 * for bit, either way. */
mcpt_status mcpt_set_camera(mcpt_ctx* ctx, const mcpt_camera* camera);

/* New positions (and optionally new normals) for the SAME faces: n_vertex / n_normal must equal those of the mcpt_scene_desc the context was
 * created from; normal == NULL keeps the normals.  Rewrites the triangle streams and the light records and refits BOTH trees on the device.
 *  - `vertex` is validated on the host before any device work, by mcpt_create's rules (every vertex a face uses finite and |x| <= 1e18; the
 *    counts; NULL): MCPT_ERR_INVALID_ARG, context unchanged.  It is staged through pinned memory and copied in stream order, so the caller
 *    may reuse the arrays when the call returns.
 *  - Device coordinates stay relative to the CREATION-time centre; mcpt_scene_info::centre does not change.  Geometry that travels far from
 *    it loses fp32 precision (the absolute ray epsilon 1e-4 needs |coordinate| * 2^-24 << 1e-4): create a new context then.
 *  - Tie ranks, leaf order, lobe classes, materials, textures and the light list's membership and order are those of creation; with
 *    MCPT_FLAG_REFERENCE_TIE_ORDER the ranks are the creation geometry's.
 *  - Topology and octant slots are kept, so a large deformation makes traversal slower, never wrong; mcpt_update_info::wide_area_ratio tells
 *    the caller when mcpt_rebuild_trees (below) is due: new trees for the moved geometry in this context, everything else kept.
 *  - mcpt_clone_to_device of a dynamic context gives a dynamic context.  Works with either builder, with deep device-built binary trees and
 *    with both integrators. */
mcpt_status mcpt_update_vertices(mcpt_ctx* ctx, const double* vertex, uint32_t n_vertex, const double* normal, uint32_t n_normal);

typedef struct mcpt_update_info {
    uint32_t struct_size, updates;      /* mcpt_update_vertices / _transforms / _skin / _morph (+ _reproject) / _normals calls on this context so far */
    double   last_update_ms;            /* device time of the last one, first to last operation on the stream (HIP events) */
    double   wide_area_ratio;           /* sum of the child-box areas of the 8-wide tree now / when it was built, by mcpt_create or by the last
                                           mcpt_rebuild_trees (dequantised boxes; 1.0 before any update and right after a rebuild) */
    uint32_t reserved[4];
} mcpt_update_info;
mcpt_status mcpt_get_update_info(mcpt_ctx* ctx, mcpt_update_info* out);   /* synchronises */

/* Probe: downloads the context's CURRENT device streams and runs the host soundness walks on them: the 8-wide tree's (every triangle's fp32
 * test data inside every dequantised box on its root path, referenced once) and the same containment check on the binary tree.
 * MCPT_OK = sound; otherwise MCPT_ERR_INVALID_ARG with the walk's message in mcpt_last_error(). */
mcpt_status mcpt_probe_validate_trees(mcpt_ctx* ctx);

/* ---- temporal reprojection: the film carried across a camera move ------------------------------------------------------- */
/* mcpt_set_camera_reproject is mcpt_set_camera for a caller who wants to keep the film: per pixel of the NEW view the first-hit surface point
 * (feature depth along the pixel-centre ray) is projected into the OLD view, the old film is gathered bilinearly there -- a tap counts when it
 * is inside the image, holds samples, is a surface pixel (coverage >= 0.5) and passes a relative depth test and a normal test against the
 * old view's features; taps of zero weight never count -- and the bound film becomes {mean * n, n} with n = min(rint(weighted mean of the taps'
 * counts), max_history); {0, 0, 0, 0} where there is no history (background, emitters, disocclusions, less than a quarter of the bilinear
 * weight left, outside the old image, behind the old eye, or an old view whose front / right / up are linearly dependent).
 *  - The history cap is the point of the design: reprojected radiance is exact only for view-independent (diffuse) shading.  On glossy and
 *    mirror surfaces it lags behind the view; max_history bounds how long that stale radiance survives once new samples are added.  Lobes
 *    are not classified.
 *  - Asynchronous; all device work is on the context's stream, ordered like mcpt_set_camera.  A film bound with mcpt_bind_accum is the one
 *    rewritten.  If the context holds no features, those of the CURRENT camera are rendered first (feature_spp, feature_seed).  Afterwards the
 *    context HOLDS features -- those of the new view, mcpt_render_features(ctx, feature_spp, feature_seed) exactly -- so mcpt_denoise may
 *    follow at once; the denoised film and the last adaptive tile error are dropped as after mcpt_set_camera; the counters are untouched.
 *  - Refusals (the camera by mcpt_set_camera's rules, the options by the ranges below, MCPT_ERR_BVH_DEPTH where mcpt_render_features answers
 *    it) change nothing: not the camera, the film, or the features held.
 *  - The first call allocates 48 B per pixel (the old view's features and a copy of the old film), counted in device_bytes, plus the 32 B
 *    per pixel of the feature buffers if the context never had any.  A clone starts without them.
 *  - Which first_sample / seed to continue with is the caller's business: continuing with sample indices that are already in the history
 *    correlates the new samples with it (the same paths, seen from the new eye) -- continue past them, or change the seed.
 *  - A camera move only: the film is carried across a vertex update by mcpt_update_vertices_reproject below, which follows the surfaces. */
typedef struct mcpt_reproject_opts {
    uint32_t struct_size;       /* = sizeof(mcpt_reproject_opts) */
    uint32_t feature_spp;       /* features of the new view (and of the old one if the context holds none): 0 = default 4, max 64 */
    uint64_t feature_seed;
    float    max_history;       /* cap on the sample count carried over per pixel; 0 = default 32; finite, >= 1 */
    float    depth_tolerance;   /* relative; 0 = default 0.05; finite, in (0, 1] */
    float    normal_threshold;  /* minimum cosine; 0 = default 0.9; in (0, 1] */
    uint32_t reserved[3];
} mcpt_reproject_opts;
typedef struct mcpt_reproject_info {
    uint32_t struct_size, reprojections;   /* mcpt_set_camera_reproject + mcpt_update_{vertices,transforms,skin,morph}_reproject calls */
    uint64_t pixels_reused;                /* pixels of the last call written with a history of >= 1 sample */
    double   last_ms;                      /* device time of the last call, first to last operation on the stream (HIP events) */
    uint32_t reserved[4];
} mcpt_reproject_info;
mcpt_status mcpt_set_camera_reproject(mcpt_ctx* ctx, const mcpt_camera* camera, const mcpt_reproject_opts* opts);   /* NULL opts = defaults */
mcpt_status mcpt_get_reproject_info(mcpt_ctx* ctx, mcpt_reproject_info* out);   /* synchronises */
/* Probe: the reprojection kernel alone on caller data of the context's film size -- the old film (width * height {sum rgb, count}), the old and
 * the new view's features (width * height * 8 floats each, mcpt_read_features' layout) and both cameras (mcpt_set_camera's rules).  Touches
 * neither the context's camera nor its film nor its features.  Synchronous. */
mcpt_status mcpt_probe_reproject(mcpt_ctx* ctx, const mcpt_camera* old_cam, const mcpt_camera* new_cam, const float* old_film_host,
                                 const float* old_feat8_host, const float* new_feat8_host, const mcpt_reproject_opts* opts, float* out_film_host,
                                 uint64_t* out_reused);

/* ---- motion-vector reprojection: the film carried across a vertex update ------------------------------------------------ */
/* mcpt_update_vertices_reproject is mcpt_update_vertices for a caller who wants to keep the film (needs MCPT_FLAG_DYNAMIC), optionally with a
 * camera move in the same call (camera NULL = keep).  Per pixel of the NEW view the first hit of the pixel-centre ray in the NEW scene names a
 * triangle and barycentrics; the vertices the scene had BEFORE the call say where that surface point was, the normals it had before say which
 * way it faced (turned towards the old eye), and from there on it is mcpt_set_camera_reproject's projection, bilinear gather and tap rules --
 * except that a tap's normal is compared with that OLD shading normal of the point, not with the new view's normal, so a rotating object keeps
 * its history.  No history where mcpt_set_camera_reproject has none, nor where the centre ray misses or meets an emitter.
 *  - Validation, in this order and all before any device work: the vertices by mcpt_update_vertices' rules, the camera (when given) by
 *    mcpt_set_camera's, the options by the ranges above, MCPT_ERR_BVH_DEPTH where mcpt_render_features answers it.  A refusal changes nothing: not
 *    the geometry, the camera, the film or the features held.
 *  - Asynchronous; all device work is on the context's stream, ordered like mcpt_update_vertices: features of the current scene if none are
 *    held, the old features / film / vertices / normals set aside, the update exactly as mcpt_update_vertices does it, the camera, the new
 *    features, the first hits, the gather into the bound film.  Afterwards the context holds the features of the new scene and view
 *    (mcpt_denoise may follow at once); the denoised film and the adaptive tile error are dropped; the counters are untouched.
 *  - mcpt_get_update_info and mcpt_get_reproject_info count the call as one update and one reprojection; pixels_reused and last_ms describe it
 *    (last_ms spans the whole call, last_update_ms its refit).
 *  - The first call allocates 16 B per pixel (the first hits) and 24 B x (n_vertex + n_normal) (the old arrays) on top of
 *    mcpt_set_camera_reproject's 48 B per pixel (+ 32 B per pixel if the context never had features), all counted in device_bytes.  A clone
 *    starts without them.
 *  - The radiance carried over is the old scene's: shadows and indirect light of what moved lag behind like glossy radiance behind the view,
 *    and max_history bounds for how long. */
mcpt_status mcpt_update_vertices_reproject(mcpt_ctx* ctx, const double* vertex, uint32_t n_vertex, const double* normal, uint32_t n_normal,
                                           const mcpt_camera* camera /* NULL = keep */, const mcpt_reproject_opts* opts /* NULL = defaults */);
/* Probes, both synchronous; neither touches the context's film, features, camera or geometry.
 * mcpt_probe_first_hits: the first-hit kernel on the current scene and camera -- per pixel the face (Model::face order, -1 = miss) and
 * {u, v, t} of the closest hit of the pixel-centre ray (0, 0, 0 for a miss); MCPT_ERR_BVH_DEPTH where mcpt_render_features answers it.
 * mcpt_probe_reproject_motion: the motion kernel alone on caller data of the context's film size (a MCPT_FLAG_DYNAMIC context: the faces' vertex
 * and normal indices and materials are the context's).  old_vertex / old_normal: n_vertex / n_normal records of the scene description, NULL =
 * the context's current ones.  hit_face / hit_uv2: per pixel of the new view a face (Model::face order, -1 = miss) and its {u, v}, the way
 * mcpt_probe_hit_shade takes hits; a face outside [-1, n_face) or a non-finite u or v is refused on the host.  The rest as mcpt_probe_reproject. */
mcpt_status mcpt_probe_first_hits(mcpt_ctx* ctx, int32_t* out_face, float* out_uvt3);
mcpt_status mcpt_probe_reproject_motion(mcpt_ctx* ctx, const mcpt_camera* old_cam, const mcpt_camera* new_cam, const double* old_vertex,
                                        const double* old_normal, const float* old_film_host, const float* old_feat8_host, const float* new_feat8_host,
                                        const int32_t* hit_face_host, const float* hit_uv2_host, const mcpt_reproject_opts* opts,
                                        float* out_film_host, uint64_t* out_reused);

/* ---- material, light and texture edits of a live context -------------------------------------------------------------------- */
/* What a surface looks like, edited without rebuilding anything: ks, ns, radiance and map_kd of every material (mcpt_update_materials) and the
 * texels of one texture (mcpt_update_texture).  Both work on every context (MCPT_FLAG_DYNAMIC or not, either builder, both integrators) and are
 * ordered like mcpt_update_vertices: asynchronous, all device work on the context's stream, so renders enqueued before the call see the old look
 * and renders after it the new one.  Host data is staged through pinned memory and copied in stream order: the caller may reuse its arrays when
 * the call returns.  Neither touches the film or the counters (the caller clears the film); the feature buffers, the denoised film and the
 * adaptive tile error are dropped as after mcpt_set_camera.  A clone taken afterwards is a clone of the edited state, and a later
 * mcpt_update_vertices works on the new light list.
 *
 * mcpt_update_materials: n_materials must equal creation's, and every map_kd must name one of the textures the context was created with
 * (re-pointing a material at another of them is allowed).  Validated on the host before any device work; a refusal changes nothing:
 * MCPT_ERR_INVALID_ARG for NULL, a wrong count, a map_kd out of range or a non-finite ks / ns / radiance; MCPT_ERR_NO_LIGHTS when no face would
 * be left with |radiance| > 0.01.  The material records are formed by the function mcpt_create uses; the lobe class of every triangle and the
 * light list -- membership by |radiance| > 0.01, in Model::face order -- are rebuilt on the device, bit for bit what mcpt_create of the edited
 * scene uploads.  mcpt_scene_info::n_lights and device_bytes follow.  The first call allocates 4 B per face of scratch; the light buffers grow
 * when the list outgrows them (one stream synchronisation then) and never shrink.
 *
 * mcpt_update_texture: new texels for texture `index`; width and height must equal creation's (else MCPT_ERR_INVALID_ARG).  A 1x1 texture is a
 * constant Kd colour: its new value also reaches every material that maps it.  The light list is not touched. */
mcpt_status mcpt_update_materials(mcpt_ctx* ctx, const mcpt_material* materials, uint32_t n_materials);
mcpt_status mcpt_update_texture(mcpt_ctx* ctx, uint32_t index, const mcpt_texture* tex);
typedef struct mcpt_material_info {
    uint32_t struct_size, updates;      /* mcpt_update_materials calls on this context so far */
    uint32_t n_lights, reserved0;       /* entries of the light list now */
    double   last_ms;                   /* device time of the last mcpt_update_materials, first to last operation on the stream (HIP events) */
    uint32_t reserved[4];
} mcpt_material_info;
mcpt_status mcpt_get_material_info(mcpt_ctx* ctx, mcpt_material_info* out);   /* synchronises */
/* Probes, synchronous, touch nothing; both work on any context, so an edited context can be compared with a fresh one record for record.
 * mcpt_probe_lights: per light in list order its face (Model::face order), out13 = {area, radiance[3], n0[3], n1[3], n2[3]} and the nine fp64
 * corner coordinates the device samples it from (relative to mcpt_scene_info::centre).  *out_n = n_lights; capacity < n_lights is
 * MCPT_ERR_INVALID_ARG with *out_n set.  mcpt_probe_face_classes: per face (n_face, Model::face order) the lobe set its hits are shaded with:
 * 0 diffuse, 1 Blinn-Phong + diffuse, 2 mirror + diffuse. */
mcpt_status mcpt_probe_lights(mcpt_ctx* ctx, uint32_t capacity, int32_t* out_face, float* out13, double* out_pos9, uint32_t* out_n);
mcpt_status mcpt_probe_face_classes(mcpt_ctx* ctx, uint8_t* out_class);

/* ---- rigid parts moved by per-group transforms on the device ----------------------------------------------------------------- */
/* The usual animation moves a few rigid parts.  Instead of computing every vertex on the host and sending all of them (mcpt_update_vertices), the
 * caller names a group per vertex and per normal once and then sends one 3x4 matrix per group and frame: the device keeps a REST POSE and writes
 * the current vertices and normals from it.  All three calls need MCPT_FLAG_DYNAMIC (else MCPT_ERR_UNSUPPORTED).
 *
 * mcpt_set_vertex_groups: set-up, synchronous.  n_vertex / n_normal must equal the scene's, 1 <= n_groups <= n_vertex + n_normal, every id
 * < n_groups (normal_group may be NULL when n_normal is 0); a violation is MCPT_ERR_INVALID_ARG with nothing changed.  Groups are per vertex and
 * per normal, not per face (the context keeps no host copy of the faces): a vertex or normal shared by two parts is the caller's to duplicate.
 * The context's CURRENT vertices and normals become the rest pose (copied device to device), the ids are uploaded, and per group R_g -- the
 * largest |coordinate| among its vertices that a face uses, 0 without any -- is kept for the validation below (one read-back of the vertices).
 * Calling it again replaces the groups and takes the rest pose anew.  Allocates, counted in device_bytes, 24 B x (n_vertex + n_normal) for the
 * rest pose, 4 B x (n_vertex + n_normal) for the ids and 168 B x n_groups for the table (per group the 12 doubles of its matrix and the 9 of its
 * cofactor matrix), plus a pinned stage of the table's size.  mcpt_clone_to_device carries the groups, the rest pose and R_g.
 *
 * mcpt_update_transforms: m3x4 holds n_groups row-major 3x4 matrices [A | t] in world space.  Every vertex becomes A rest + t of its group -- per
 * row ((a0 x + a1 y) + a2 z) + t in fp64, in that association -- and every normal cof(A) rest_normal, normalised (cof(A) = det(A) A^-T, so
 * nothing is divided by the determinant; a result of length 0 or not finite is left as it is).
 *  - MIRRORING (det A < 0): cof(A) carries a normal the way it carries the cross product of a triangle's edges, so the normals of a mirrored
 *    part come out on the side its stored winding faces -- for a closed part that is INTO the object.  This renderer orients a surface by its
 *    vertex normals alone (front = dot(normal, direction) < 0; an emitter radiates to its normals' side), never by the winding: a mirrored
 *    sphere is shaded as seen from inside and a mirrored lamp radiates to its other side.  A caller who mirrors a part and wants it to look
 *    mirrored, not turned inside out, negates that part's normals as well: mcpt_update_vertices with the normals negated BEFORE
 *    mcpt_set_vertex_groups, so that the rest pose holds them.
 * From there on the call IS mcpt_update_vertices after its upload: the same refit, ordering, bookkeeping (mcpt_get_update_info counts it, and
 * last_update_ms spans the transform kernels and the refit) and what it leaves untouched (film, counters) or drops (features, denoised film,
 * tile error).
 *  - Transforms apply to the rest pose and never accumulate: the same matrices twice give the same scene, identities give the rest pose back.  A
 *    later mcpt_update_vertices moves the scene and leaves the rest pose alone; the next mcpt_update_transforms overwrites what it wrote.
 *  - Validated on the host before any device work, a refusal changes nothing; in this order: MCPT_ERR_UNSUPPORTED without MCPT_FLAG_DYNAMIC;
 *    MCPT_ERR_INVALID_ARG when no groups are set, for NULL or another n_groups, for an entry that is not finite, for det A zero or not finite,
 *    and when for some row (|a0| + |a1| + |a2|) R_g + |t| exceeds 1e18 or is not finite.  That row bound is CONSERVATIVE: it may refuse a
 *    transform whose vertices mcpt_update_vertices would accept just under 1e18; in exchange validation needs no device round trip.
 *  - Asynchronous on the context's stream.  The matrices are staged through pinned memory and copied in stream order: the caller may reuse its
 *    array when the call returns, and back-to-back calls cannot overtake each other.
 *
 * mcpt_update_transforms_reproject is mcpt_update_vertices_reproject with the transform in place of the upload; validation order: the matrices,
 * the camera (when given), the options, MCPT_ERR_BVH_DEPTH. */
mcpt_status mcpt_set_vertex_groups(mcpt_ctx* ctx, const uint32_t* vertex_group, uint32_t n_vertex, const uint32_t* normal_group, uint32_t n_normal,
                                   uint32_t n_groups);
mcpt_status mcpt_update_transforms(mcpt_ctx* ctx, const double* m3x4, uint32_t n_groups);
mcpt_status mcpt_update_transforms_reproject(mcpt_ctx* ctx, const double* m3x4, uint32_t n_groups, const mcpt_camera* camera /* NULL = keep */,
                                             const mcpt_reproject_opts* opts /* NULL = defaults */);
typedef struct mcpt_transform_info {
    uint32_t struct_size, n_groups;     /* groups set now (0 = none) */
    uint32_t updates, reserved0;        /* mcpt_update_transforms (+ _reproject) calls on this context so far */
    double   last_ms;                   /* device time of the last one's transform part: the table's copy and the two kernels (HIP events) */
    uint32_t reserved[4];
} mcpt_transform_info;
mcpt_status mcpt_get_transform_info(mcpt_ctx* ctx, mcpt_transform_info* out);   /* synchronises */

/* ---- deforming parts: linear-blend skinning on the device --------------------------------------------------------------------- */
/* A bending arm, a swaying plant or a character has vertices that follow several bones with weights: mcpt_update_transforms cannot express it (a
 * vertex belongs to one group).  The caller names MCPT_SKIN_INFLUENCES bone ids and weights per vertex and per normal once and then sends one 3x4
 * matrix per bone and frame: the device keeps the skin's REST POSE and writes the current vertices and normals from it.  All calls need
 * MCPT_FLAG_DYNAMIC (else MCPT_ERR_UNSUPPORTED).
 *
 * mcpt_set_vertex_skin: set-up, synchronous, the twin of mcpt_set_vertex_groups.  vertex_bone / vertex_weight hold 4 ids / 4 doubles per vertex,
 * normal_bone / normal_weight 4 per normal (both may be NULL only when n_normal is 0).  The context's CURRENT vertices and normals become the skin's
 * OWN rest pose (copied device to device) -- independent of the groups' rest pose; both features may be set on one context.  Per bone R_b -- the
 * largest |coordinate| among the vertices that a face uses and that give the bone a weight > 0, 0 without any -- is kept for the validation below
 * (one read-back of the vertices).  Calling it again replaces the skin and takes the rest pose anew.  Allocates, counted in device_bytes, 24 B
 * (rest pose) + 16 B (ids) + 32 B (weights) per vertex and per normal and 96 B per bone (the table), plus a pinned stage of the table's size.
 * mcpt_clone_to_device carries skin, rest pose and R_b; mcpt_rebuild_trees keeps them (they are per vertex, not per leaf: nothing is permuted).
 *  - Refused with nothing changed, MCPT_ERR_INVALID_ARG: counts that differ from the scene's; a NULL array; n_bones outside
 *    [1, 4 (n_vertex + n_normal)]; an id >= n_bones in ANY slot, zero-weight slots included; a weight that is not finite or is outside [0, 1]; a
 *    record whose sum S = ((w0 + w1) + w2) + w3 has |S - 1| > 1e-6.
 *  - Weights are USED AS GIVEN and never renormalised: what the caller sends is what every frame is blended with.  (fp32 weights normalised by the
 *    caller sum to 1 within about 1e-7 and pass.)
 *
 * mcpt_update_skin: m3x4 holds n_bones row-major 3x4 matrices [A | t] in world space.  Per record the blended matrix is, entrywise,
 * B = ((w0 M0 + w1 M1) + w2 M2) + w3 M3 -- all four slots in that order, none skipped because its weight is 0.  A vertex becomes per row
 * ((B0 x + B1 y) + B2 z) + B3; a normal, with its own influences, cof(A_B) rest_normal per row (C0 x + C1 y) + C2 z, divided by its length when
 * that is finite and > 0 and left as it is otherwise (mcpt_update_transforms' rule).  Everything in fp64, one rounding per operation.
 *  - Blends that come out (nearly) SINGULAR give meaningless normals: two opposed rotations blended half and half are the classic case (the
 *    "candy wrapper").  Only the bones themselves are validated, not their blends.
 * From there on the call IS mcpt_update_vertices after its upload: the same refit, ordering, bookkeeping (mcpt_get_update_info counts it, and
 * last_update_ms spans the table's copy, the two kernels and the refit) and what it leaves untouched (film, counters) or drops (features, denoised
 * film, tile error).
 *  - Bones apply to the skin's rest pose and never accumulate.  A later mcpt_update_vertices or mcpt_update_transforms overwrites what the call
 *    wrote and leaves the skin's rest pose alone; the next mcpt_update_skin overwrites what they wrote and leaves the groups' rest pose alone.
 *  - Validated on the host before any device work, a refusal changes nothing; in this order: MCPT_ERR_UNSUPPORTED without MCPT_FLAG_DYNAMIC;
 *    MCPT_ERR_INVALID_ARG when no skin is set, for NULL or another n_bones, for an entry that is not finite, for a bone whose det A is zero or not
 *    finite, and when for some bone and row (1 + 2^-16) ((|a0| + |a1| + |a2|) R_b + |t|) exceeds 1e18 or is not finite.  That row bound is
 *    CONSERVATIVE: a vertex's result is bounded by S times the largest reach of its bones, and the factor covers S <= 1 + 1e-6 and the rounding;
 *    it may refuse bones whose vertices mcpt_update_vertices would accept just under 1e18; in exchange validation needs no device round trip.
 *  - Asynchronous on the context's stream.  The matrices are staged through pinned memory and copied in stream order: the caller may reuse its
 *    array when the call returns, and back-to-back calls cannot overtake each other.
 *
 * mcpt_update_skin_reproject is mcpt_update_vertices_reproject with the bones in place of the upload; validation order: the matrices, the camera
 * (when given), the options, MCPT_ERR_BVH_DEPTH. */
#define MCPT_SKIN_INFLUENCES 4
mcpt_status mcpt_set_vertex_skin(mcpt_ctx* ctx, const uint32_t* vertex_bone /* 4 per vertex */, const double* vertex_weight /* 4 per vertex */,
                                 uint32_t n_vertex, const uint32_t* normal_bone, const double* normal_weight, uint32_t n_normal, uint32_t n_bones);
mcpt_status mcpt_update_skin(mcpt_ctx* ctx, const double* m3x4, uint32_t n_bones);
mcpt_status mcpt_update_skin_reproject(mcpt_ctx* ctx, const double* m3x4, uint32_t n_bones, const mcpt_camera* camera /* NULL = keep */,
                                       const mcpt_reproject_opts* opts /* NULL = defaults */);
typedef struct mcpt_skin_info {
    uint32_t struct_size, n_bones;      /* bones of the skin set now (0 = none) */
    uint32_t updates, reserved0;        /* mcpt_update_skin (+ _reproject) calls on this context so far */
    double   last_ms;                   /* device time of the last one's skinning part: the table's copy and the two kernels (HIP events) */
    uint32_t reserved[4];
} mcpt_skin_info;
mcpt_status mcpt_get_skin_info(mcpt_ctx* ctx, mcpt_skin_info* out);   /* synchronises */

/* ---- deforming parts: dual-quaternion skinning -------------------------------------------------------------------------------- */
/* Blending the bones' MATRICES shrinks a twisted part: two bones that differ by a rotation of 170 degrees, blended half and half, leave a ring of
 * vertices at 0.087 of its radius, and at 180 degrees the surface collapses onto the axis (the "candy wrapper" above).  The second skinning mode
 * blends the bones as unit DUAL QUATERNIONS (Kavan et al. 2008): the blend of rigid motions is again a rigid motion, the ring keeps its radius and
 * turns by half the angle.
 *
 * mcpt_set_skin_mode: MCPT_SKIN_LINEAR (the default: everything above, bit for bit) or MCPT_SKIN_DUAL_QUATERNION.  A sticky property of the
 * context: it may be set before or after mcpt_set_vertex_skin, survives another mcpt_set_vertex_skin, travels with mcpt_clone_to_device and is
 * kept by mcpt_rebuild_trees.  Synchronous.  MCPT_ERR_UNSUPPORTED without MCPT_FLAG_DYNAMIC; MCPT_ERR_INVALID_ARG for an unknown mode, with nothing
 * changed.  While the mode is MCPT_SKIN_DUAL_QUATERNION and a skin is set the context holds a second table of 8 doubles per bone (64 B x n_bones,
 * counted in device_bytes) and a pinned stage of that size; both are released when the mode goes back to MCPT_SKIN_LINEAR.
 *
 * Every call that takes bones -- mcpt_update_skin, mcpt_update_skin_reproject, mcpt_update_morph and mcpt_update_morph_reproject with bones --
 * follows the mode.  The bones are given as before, one row-major 3x4 matrix [A | t] each.  In MCPT_SKIN_DUAL_QUATERNION mode:
 *  - Every bone must be RIGID: det A > 0 and |(A^T A)ij - delta_ij| <= 1e-6 for every entry, each entry computed as (a0i a0j + a1i a1j) + a2i a2j
 *    (rotations built in fp32 pass).  A scaled, sheared or mirrored bone is MCPT_ERR_INVALID_ARG: such bones need MCPT_SKIN_LINEAR.  The checks run
 *    in mcpt_update_skin's order, after its own matrix checks; the reach bound (1 + 2^-16) (2 R_b + 16 ((|tx| + |ty|) + |tz|)) <= 1e18 per bone
 *    replaces the row bound (with a morph in the same call its reach E stands for every R_b).  It is conservative too: a rotation carries
 *    |p|inf <= R_b to at most sqrt(3) R_b, and the blended translation is at most 16 S times the longest of the blended bones' translations.
 *  - The host turns each bone into the unit dual quaternion {w, x, y, z, dw, dx, dy, dz}: the rotation by Shepperd's method (the largest of
 *    trace, a00, a11, a22 decides the branch, the first wins a tie), divided by its length, negated when w < 0; the dual part is 1/2 (0, t) q.
 *    Only these 8 doubles per bone cross the bus.
 *  - Per record SLOT 0 IS THE PIVOT, whatever its weight (put the main bone first): slot k = 1..3 enters with the sign s_k = -1 when the dot
 *    product of its rotation quaternion with slot 0's is < 0, else +1 -- q and -q are the same rotation, and the blend goes the short way round.
 *    All eight components are blended as ((w0 q0 + (w1 s1) q1) + (w2 s2) q2) + (w3 s3) q3, all four slots in that order.  With n2 the squared
 *    length of the blended rotation part: when !(n2 >= 2^-8 && n2 < inf) the blend is DEGENERATE and the record keeps its rest pose, bit for bit
 *    (this needs three or four wildly opposed bones: two bones in slots 0 and 1 give n2 >= 1/2).  Otherwise both parts are divided by sqrt(n2), R is the rotation
 *    matrix of the real part r, t = 2 (r.w d_v - d.w r_v + r_v x d_v), and a vertex becomes per row ((R0 x + R1 y) + R2 z) + t.
 *  - A normal, with its own influences, blends the rotation parts only, by the same signs and the same degenerate rule (a degenerate normal is
 *    copied as it is, not normalised); otherwise R rest_normal per row (R0 x + R1 y) + R2 z, divided by its length when that is finite and > 0.
 *  - Everything in fp64, one rounding per operation; DESIGN.md §21 fixes the association of every expression.
 * Refit, automatic normals, ordering, bookkeeping (mcpt_skin_info, mcpt_update_info) and the reprojection are the same in both modes. */
#define MCPT_SKIN_LINEAR          0u   /* blend the bones' matrices (the default) */
#define MCPT_SKIN_DUAL_QUATERNION 1u   /* blend the bones as unit dual quaternions: rigid bones only */
mcpt_status mcpt_set_skin_mode(mcpt_ctx* ctx, uint32_t mode);
mcpt_status mcpt_get_skin_mode(mcpt_ctx* ctx, uint32_t* out_mode);

/* ---- baked vertex animation: device-resident keyframes played by time --------------------------------------------------------- */
/* Cloth, a fluid meshed per frame with fixed topology, a destruction sequence, a point cache, an OBJ sequence: per-vertex motion that no bone and
 * no sparse target expresses.  The caller uploads the keyframes ONCE -- whole vertex arrays (and, optionally, normal arrays), uniformly spaced in
 * time -- and then sends ONE DOUBLE, THE TIME, per frame: the device writes the current vertices and normals by interpolating the keyframes.
 * All four calls need MCPT_FLAG_DYNAMIC (else MCPT_ERR_UNSUPPORTED).
 *
 * mcpt_set_vertex_keyframes: set-up, synchronous, the twin of mcpt_set_vertex_morph.  vertex_frames holds n_frames arrays of 3 n_vertex doubles,
 * frame after frame; normal_frames (NULL, or n_frames arrays of 3 n_normal doubles) the normals of every frame, used AS GIVEN (not normalised
 * here).  Frame k lies at start_time + k * frame_time.  opts == NULL: MCPT_KEYFRAMES_LINEAR, MCPT_KEYFRAMES_CLAMP, start_time 0, frame_time 1.
 * Without normal_frames the context's CURRENT normals are captured (device to device) as the keyframes' own rest normals, and every update writes
 * them, as mcpt_update_morph does without normal targets.  The set is independent of groups, skin and morph: all of them may be set on one
 * context; a call of any route overwrites what the previous route wrote and touches no other route's rest pose.  Calling it again replaces
 * frames and options.  On the device a frame's stride is its 3 n doubles rounded up to an EVEN number (3 n is odd when n is odd; the padding is
 * 0 and never read), so that every frame, like the output arrays, starts 16-byte aligned.  Allocates, counted in device_bytes and reported in
 * mcpt_keyframe_info::device_bytes: 8 B x n_frames x stride(n_vertex), the same for the normals when normal_frames is given, and 24 B per
 * vertex and per normal for the pose captured at set-up (of which only the normals are read, and only without normal_frames).  Freed with the
 * context; mcpt_clone_to_device carries all of it; mcpt_rebuild_trees leaves it alone (it is per vertex, not per leaf).
 *  - Refused with nothing changed, MCPT_ERR_INVALID_ARG, in this order: a NULL context or NULL vertex_frames; n_vertex / n_normal that differ
 *    from the scene's; a wrong struct_size; an unknown interpolation; an unknown wrap; n_frames outside [2, MCPT_KEYFRAMES_MAX]; start_time not
 *    finite; frame_time not finite or <= 0; a coordinate of a vertex that a face uses that is not finite or has |x| > 1e18; a normal component
 *    that is not finite; a reach E that is not <= 1e18, with E = (1 + 2^-16) (c R), R the largest |coordinate| of a used vertex over all
 *    frames, c = 1 (linear) or 1.25 (Catmull-Rom: the largest sum of |weights|, reached at u = 1/2).  MCPT_ERR_HIP when an allocation fails.
 *    Because of these checks an update validates only its time: no device round trip.
 *
 * Time to segment, on the host, fp64, one correctly rounded operation each, K = n_frames: x = (time - start_time) / frame_time.
 *  - MCPT_KEYFRAMES_CLAMP: x <= 0: k = 0, u = 0; x >= K - 1: k = K - 1, u = 0; otherwise k = floor(x), u = x - k.
 *  - MCPT_KEYFRAMES_LOOP: the period is K frames (frame K - 1 blends into frame 0): x = fmod(x, K); if x < 0: x = x + K; if then !(x < K):
 *    x = 0; k = floor(x), u = x - k.
 *  - Taps: (k, k + 1) linear, (k - 1, k, k + 1, k + 2) Catmull-Rom; indices clamped to [0, K - 1] under CLAMP, taken modulo K under LOOP.
 * Weights (never renormalised): linear (1 - u, u); Catmull-Rom, with u2 = u u and u3 = u2 u: w0 = 0.5 ((2 u2 - u3) - u),
 * w1 = 0.5 ((3 u3 - 5 u2) + 2), w2 = 0.5 ((4 u2 - 3 u3) + u), w3 = 0.5 (u3 - u2).
 *
 * mcpt_update_keyframes: MCPT_ERR_INVALID_ARG for a time that is not finite, then when no keyframes are set.  u == 0: the vertices become frame k
 * COPIED device to device, bit for bit (negative zeros included), the normals frame k's as given (not normalised) -- or the rest normals.
 * Otherwise per component, fp64, one rounding per operation: linear out = w0 a + w1 b; Catmull-Rom out = ((w0 a + w1 b) + w2 c) + w3 d; normals
 * get the same sum and are then divided by sqrt((x x + y y) + z z) when that is finite and > 0, and are otherwise left as they are
 * (mcpt_update_transforms' rule); without normal_frames they are the rest normals.  Every record is written on every call.  From there on the
 * call IS mcpt_update_vertices after its upload: the auto-normals pass when it is set, the same refit, ordering and bookkeeping
 * (mcpt_get_update_info counts it), and what it leaves untouched (film, counters) or drops (features, denoised film, tile error).
 *  - Asynchronous on the context's stream.  The weights and tap indices travel as kernel arguments: nothing is staged, and back-to-back calls
 *    cannot overtake each other.
 *
 * mcpt_update_keyframes_reproject is mcpt_update_vertices_reproject with the time in place of the upload; validation order: the above, the camera
 * (when given), the options, MCPT_ERR_BVH_DEPTH. */
#define MCPT_KEYFRAMES_LINEAR      0u
#define MCPT_KEYFRAMES_CATMULL_ROM 1u   /* uniform Catmull-Rom spline through the frames: C1 motion, may overshoot by at most 1/4 */
#define MCPT_KEYFRAMES_CLAMP       0u   /* before the first frame: the first; after the last: the last */
#define MCPT_KEYFRAMES_LOOP        1u   /* periodic, period n_frames * frame_time */
#define MCPT_KEYFRAMES_MAX         65536
typedef struct mcpt_keyframe_opts {
    uint32_t struct_size;
    uint32_t interpolation;             /* MCPT_KEYFRAMES_LINEAR / _CATMULL_ROM */
    uint32_t wrap;                      /* MCPT_KEYFRAMES_CLAMP / _LOOP */
    uint32_t reserved0;
    double   start_time, frame_time;    /* frame k lies at start_time + k * frame_time; frame_time > 0 */
    uint32_t reserved[4];
} mcpt_keyframe_opts;
typedef struct mcpt_keyframe_info {
    uint32_t struct_size, n_frames;     /* frames of the set now (0 = none) */
    uint32_t interpolation, wrap;       /* of the set now */
    uint32_t updates, last_frame;       /* mcpt_update_keyframes (+ _reproject) calls on this context so far; k of the last one */
    double   last_u, last_time;         /* u and the time of the last one */
    double   last_ms;                   /* device time of the last one's deforming part: the copies or the two kernels */
    uint64_t device_bytes;              /* what the set holds on the device now */
    uint32_t reserved[4];
} mcpt_keyframe_info;
mcpt_status mcpt_set_vertex_keyframes(mcpt_ctx* ctx, const double* vertex_frames /* n_frames * 3 n_vertex */, uint32_t n_vertex,
                                      const double* normal_frames /* NULL, or n_frames * 3 n_normal */, uint32_t n_normal,
                                      uint32_t n_frames, const mcpt_keyframe_opts* opts /* NULL: linear, clamp, start 0, frame_time 1 */);
mcpt_status mcpt_update_keyframes(mcpt_ctx* ctx, double time);
mcpt_status mcpt_update_keyframes_reproject(mcpt_ctx* ctx, double time, const mcpt_camera* camera /* NULL = keep */, const mcpt_reproject_opts* opts /* NULL = defaults */);
mcpt_status mcpt_get_keyframe_info(mcpt_ctx* ctx, mcpt_keyframe_info* out);   /* synchronises */

/* ---- live scenes: each part driven by its own deformer in one update call ----------------------------------------------------- */
/* mcpt_update_transforms, _skin, _morph and _keyframes each write EVERY record of the scene, so a later call of another route overwrites what the
 * previous one wrote: a skinned figure, a spinning rigid fan and a keyframed cloth in one scene cannot be animated by them.  Here every vertex
 * record and every normal record names the ONE route that writes it, and one call runs several routes, lets each write only its own records,
 * runs the automatic-normals pass once and refits once.  All calls need MCPT_FLAG_DYNAMIC (else MCPT_ERR_UNSUPPORTED).
 *
 *     id  owner                  written by
 *     0   MCPT_OWNER_NONE        no route of a parts update: the record keeps what it holds
 *     1   MCPT_OWNER_GROUPS      mcpt_update_transforms' arithmetic
 *     2   MCPT_OWNER_SKIN        mcpt_update_skin's, in the context's skinning mode
 *     3   MCPT_OWNER_MORPH       mcpt_update_morph's; with MCPT_PARTS_MORPH_THEN_SKIN morph, then skin
 *     4   MCPT_OWNER_KEYFRAMES   mcpt_update_keyframes'
 * The route bit is MCPT_ROUTE_x = 1u << MCPT_OWNER_x.
 *
 * mcpt_set_vertex_owners: set-up, synchronous: one owner id per vertex and per normal.  The two arrays are independent; pairing them sensibly is
 * the caller's business.  No route has to be set up yet.  Calling it again replaces the owners.  vertex_owner == NULL drops them and frees what
 * they hold (device_bytes is what it was before the first call).  Allocates, counted in device_bytes and reported in
 * mcpt_parts_info::device_bytes: 1 B per vertex and per normal for the owners, and one scratch pair of 24 B per vertex and per normal that the
 * routes of a parts update write.  Freed with the context; mcpt_clone_to_device carries the owners; mcpt_rebuild_trees keeps them (they are per
 * record, not per leaf).
 *  - Refused with nothing changed, MCPT_ERR_INVALID_ARG, in this order: n_vertex / n_normal that differ from the scene's; a NULL normal_owner
 *    with n_normal > 0; an id > 4 (the message names the record; vertices are judged first).  MCPT_ERR_HIP when an allocation fails.
 *
 * mcpt_update_parts runs the routes named in `routes`, in ascending id order, each with the payload of its own call.  Afterwards
 *  - a record whose owner's route ran holds, bit for bit, what that route's own call -- mcpt_update_transforms, mcpt_update_skin,
 *    mcpt_update_morph (with the bones iff MCPT_PARTS_MORPH_THEN_SKIN) or mcpt_update_keyframes, with the same payload, on this context -- would
 *    have written to that record;
 *  - every other record (owner NONE, or an owner whose route did not run in this call) holds the bits it held before.
 * A route that runs and owns no record writes nothing; it still advances its own info (mcpt_transform_info::updates ...) as its own call does.
 * From there on the call IS mcpt_update_vertices after its upload, as for every other route: the auto-normals pass, when set, runs once on the
 * combined arrays and overrides the records it has entries for; one refit follows, ordered on the context's stream; mcpt_get_update_info counts
 * one update; film and counters are untouched; features, the denoised film and the tile error are dropped.  Asynchronous.
 *  - Everything is validated on the host before any device work, and a refusal changes nothing (no stage, no table, no counter).  In this order:
 *    MCPT_ERR_UNSUPPORTED without MCPT_FLAG_DYNAMIC; then MCPT_ERR_INVALID_ARG for a NULL update; a wrong struct_size; no owners set; routes == 0,
 *    an unknown route bit or an unknown flag bit; MCPT_PARTS_MORPH_THEN_SKIN without MCPT_ROUTE_MORPH; then per route that runs, in id order,
 *    that route's own rules for its payload (a route that was never set up, a NULL payload, a wrong count, its value checks).
 * mcpt_update_parts_reproject is mcpt_update_vertices_reproject with the parts update in place of the upload; validation order: the above, the
 * camera (when given), the options, MCPT_ERR_BVH_DEPTH.
 *
 * The existing calls do not look at the owners: mcpt_update_transforms, _skin, _morph, _keyframes, _vertices and their _reproject forms write
 * every record, as before. */
#define MCPT_OWNER_NONE      0u
#define MCPT_OWNER_GROUPS    1u
#define MCPT_OWNER_SKIN      2u
#define MCPT_OWNER_MORPH     3u
#define MCPT_OWNER_KEYFRAMES 4u
#define MCPT_ROUTE_GROUPS    (1u << MCPT_OWNER_GROUPS)
#define MCPT_ROUTE_SKIN      (1u << MCPT_OWNER_SKIN)
#define MCPT_ROUTE_MORPH     (1u << MCPT_OWNER_MORPH)
#define MCPT_ROUTE_KEYFRAMES (1u << MCPT_OWNER_KEYFRAMES)
#define MCPT_PARTS_MORPH_THEN_SKIN 0x1u   /* mcpt_scene_update::flags: the morph route's records are morphed, then skinned by bone_m3x4 */
typedef struct mcpt_scene_update {
    uint32_t struct_size;
    uint32_t routes;                    /* MCPT_ROUTE_*: the routes that run */
    uint32_t flags;                     /* MCPT_PARTS_MORPH_THEN_SKIN */
    uint32_t reserved0;
    const double* group_m3x4;           /* MCPT_ROUTE_GROUPS: mcpt_update_transforms' arguments */
    uint32_t n_groups, reserved1;
    const double* bone_m3x4;            /* MCPT_ROUTE_SKIN and / or MCPT_PARTS_MORPH_THEN_SKIN: mcpt_update_skin's */
    uint32_t n_bones, reserved2;
    const double* morph_weight;         /* MCPT_ROUTE_MORPH: mcpt_update_morph's weights */
    uint32_t n_targets, reserved3;
    double   time;                      /* MCPT_ROUTE_KEYFRAMES: mcpt_update_keyframes' */
    uint32_t reserved[4];
} mcpt_scene_update;
typedef struct mcpt_parts_info {
    uint32_t struct_size, set;          /* 1: owners are set now */
    uint32_t updates, last_routes;      /* mcpt_update_parts (+ _reproject) calls on this context so far; `routes` of the last one */
    uint32_t vertex_records[5];         /* records per owner id, of the owners set now */
    uint32_t normal_records[5];
    double   last_ms;                   /* device time of the last call's deforming part: all its routes and their selects */
    uint64_t device_bytes;              /* what the owners and the scratch pair hold on the device now */
    uint32_t reserved[4];
} mcpt_parts_info;
mcpt_status mcpt_set_vertex_owners(mcpt_ctx* ctx, const uint8_t* vertex_owner /* NULL: drop the owners */, uint32_t n_vertex,
                                   const uint8_t* normal_owner, uint32_t n_normal);
mcpt_status mcpt_update_parts(mcpt_ctx* ctx, const mcpt_scene_update* update);
mcpt_status mcpt_update_parts_reproject(mcpt_ctx* ctx, const mcpt_scene_update* update, const mcpt_camera* camera /* NULL = keep */,
                                        const mcpt_reproject_opts* opts /* NULL = defaults */);
mcpt_status mcpt_get_parts_info(mcpt_ctx* ctx, mcpt_parts_info* out);   /* synchronises */

/* ---- deforming parts: morph targets (blend shapes) on the device -------------------------------------------------------------- */
/* A facial expression, a bulging muscle or a breathing chest is a weighted sum of per-vertex displacement sets, not a matrix per bone.  The caller
 * names the targets once -- each a sparse list of records and their displacements -- and then sends ONE WEIGHT PER TARGET and frame: the device
 * keeps the morph's REST POSE and writes the current vertices and normals from it.  All calls need MCPT_FLAG_DYNAMIC (else MCPT_ERR_UNSUPPORTED).
 *
 * mcpt_set_vertex_morph: set-up, synchronous, the twin of mcpt_set_vertex_skin.  `vertex` holds the targets over the vertices, `normal` (NULL =
 * normals are not morphed: every call writes the rest pose's normals) the targets over the normals; normal->n_targets must equal
 * vertex->n_targets, one weight drives both.  A target may have no entries, and so may all of them.  The context's CURRENT vertices and normals
 * become the morph's OWN rest pose (copied device to device) -- independent of the groups' and the skin's; all three may be set on one context.
 * The host turns the per-target lists into one list per record (a counting sort; inside a record the entries are ordered by ascending target id)
 * and keeps R, the largest |coordinate| among the rest-pose vertices that a face uses (one read-back of the vertices), and per target D_k, the
 * largest |delta component| among its vertex entries whose vertex a face uses (0 without any).  Calling it again replaces the targets and takes
 * the rest pose anew.  Allocates, counted in device_bytes: 24 B per vertex and per normal (rest pose), 4 B (n_vertex + 1) + 4 B (n_normal + 1)
 * (list offsets), 32 B per entry and 8 B per target (the weights), plus a pinned stage of the weights' size.  mcpt_clone_to_device carries all of
 * it with R and D_k; mcpt_rebuild_trees keeps it (it is per vertex, not per leaf: nothing is permuted).
 *  - Refused with nothing changed, MCPT_ERR_INVALID_ARG: counts that differ from the scene's; NULL `vertex`; a wrong struct_size; n_targets
 *    outside [1, 65536]; NULL target_offset, or NULL index / delta where entries exist; offsets that decrease or do not start at 0; an index >=
 *    the record count; indices not STRICTLY ascending inside a target (so no record twice in one target); a delta component that is not finite
 *    or has |d| > 1e18.
 *
 * mcpt_update_morph: `weight` holds n_targets doubles; they may be negative or exceed 1 (extrapolation) and are never renormalised.  Everything
 * in fp64, one correctly rounded operation each.  A vertex with >= 1 entry: p = rest, then per entry in stored order (ascending target) and per
 * component p = p + weight[target] * d -- EVERY entry, one whose weight is 0 included (skipping it could change the sign of a zero).  A vertex
 * without entries: the rest pose's, bit for bit.  A normal with >= 1 entry: the same sum, then divided by its length sqrt((x x + y y) + z z)
 * when that is finite and > 0 and left as it is otherwise (mcpt_update_transforms' rule).  A normal without entries: copied, NOT normalised.
 * Every record is written on every call.
 *  - bones_m3x4 == NULL: the morphed arrays ARE the context's new vertices and normals.
 *  - bones_m3x4 != NULL: MORPH, THEN SKIN, the order glTF prescribes.  Needs mcpt_set_vertex_skin on this context; m3x4 and n_bones are
 *    mcpt_update_skin's.  The morphed arrays go to two scratch arrays (24 B per vertex and per normal, allocated by the first such call, counted
 *    in device_bytes, carried by a clone) and mcpt_update_skin's kernels, with the skin's influences, read THEM as their rest pose: in this call
 *    the skin's own rest pose is not read (and not changed) -- the morph's rest pose is the base.  mcpt_skin_info::updates advances too (its
 *    last_ms does not: this call's time is mcpt_morph_info::last_ms).
 * From there on the call IS mcpt_update_vertices after its upload: the same refit, ordering, bookkeeping (mcpt_get_update_info counts it, and
 * last_update_ms spans the weights' copy, the kernels and the refit) and what it leaves untouched (film, counters) or drops (features, denoised
 * film, tile error).
 *  - Morphs apply to the morph's rest pose and never accumulate.  A later mcpt_update_vertices / _transforms / _skin overwrites what the call
 *    wrote and leaves the morph's rest pose alone; the next mcpt_update_morph overwrites what they wrote and leaves their rest poses alone.
 *  - Validated on the host before any device work, a refusal changes nothing; in this order: MCPT_ERR_UNSUPPORTED without MCPT_FLAG_DYNAMIC;
 *    MCPT_ERR_INVALID_ARG when no morph is set, for NULL weights or another n_targets, for a weight that is not finite or has |w| > 1e18; when the
 *    reach E = (1 + 2^-16) (R + sum_k |w_k| D_k) (summed in the order of k, starting from R) exceeds 1e18 or is not finite; with bones: when no
 *    skin is set or for another n_bones, then mcpt_update_skin's matrix checks (finite entries, det A finite and non-zero), then its row bound
 *    with E in place of EVERY bone's R_b.  Both bounds are CONSERVATIVE; the second may refuse a far-away bone without members that
 *    mcpt_update_skin accepts; in exchange validation needs no device round trip.
 *  - Asynchronous on the context's stream.  Weights (and bones) are staged through pinned memory and copied in stream order: the caller may reuse
 *    its arrays when the call returns, and back-to-back calls cannot overtake each other.
 *
 * mcpt_update_morph_reproject is mcpt_update_vertices_reproject with the weights (and bones) in place of the upload; validation order: the above,
 * the camera (when given), the options, MCPT_ERR_BVH_DEPTH.
 *
 * mcpt_probe_vertices (for tests and debugging; synchronous, needs MCPT_FLAG_DYNAMIC): the context's current vertices and normals as the device
 * holds them now, whatever call wrote them.  Either output may be NULL.  Touches nothing. */
typedef struct mcpt_morph_targets {      /* one set of sparse targets over an array of records (vertices, or normals) */
    uint32_t        struct_size;
    uint32_t        n_targets;
    const uint32_t* target_offset;       /* n_targets + 1 entries, non-decreasing, [0] = 0: target k owns entries [off[k], off[k+1]) */
    const uint32_t* index;               /* per entry the record it displaces; STRICTLY ascending inside a target (so: no duplicates) */
    const double*   delta;               /* 3 doubles per entry */
    uint32_t        reserved[4];
} mcpt_morph_targets;
mcpt_status mcpt_set_vertex_morph(mcpt_ctx* ctx, const mcpt_morph_targets* vertex, uint32_t n_vertex,
                                  const mcpt_morph_targets* normal /* NULL = normals are not morphed */, uint32_t n_normal);
mcpt_status mcpt_update_morph(mcpt_ctx* ctx, const double* weight, uint32_t n_targets, const double* bones_m3x4 /* NULL = no skinning */, uint32_t n_bones);
mcpt_status mcpt_update_morph_reproject(mcpt_ctx* ctx, const double* weight, uint32_t n_targets, const double* bones_m3x4, uint32_t n_bones,
                                        const mcpt_camera* camera /* NULL = keep */, const mcpt_reproject_opts* opts /* NULL = defaults */);
typedef struct mcpt_morph_info {
    uint32_t struct_size, n_targets;    /* targets of the morph set now (0 = none) */
    uint32_t updates, reserved0;        /* mcpt_update_morph (+ _reproject) calls on this context so far */
    uint64_t vertex_entries, normal_entries;   /* entries of the per-record lists */
    double   last_ms;                   /* device time of the last one's deforming part: the weights' (and bones') copy and the morph (and skin) kernels */
    uint32_t reserved[4];
} mcpt_morph_info;
mcpt_status mcpt_get_morph_info(mcpt_ctx* ctx, mcpt_morph_info* out);   /* synchronises */
mcpt_status mcpt_probe_vertices(mcpt_ctx* ctx, double* out_vertex /* 3 n_vertex, may be NULL */, double* out_normal /* 3 n_normal, may be NULL */);

/* ---- live scenes: smooth normals recomputed on the device after every update -------------------------------------------------- */
/* None of the update routes yields normals of the DEFORMED surface: mcpt_update_vertices(normal = NULL) keeps the old ones, mcpt_update_morph
 * without normal targets writes the rest pose's, mcpt_update_skin pushes rest normals through a blended matrix.  The tracer orients a surface by
 * its vertex normals alone, so stale normals also give wrong front/back decisions and emission sides.  With auto normals on, every scene update
 * -- mcpt_update_vertices / _transforms / _skin / _morph / _keyframes and their _reproject forms -- runs one extra kernel after the route has written the
 * vertices and normals and in front of the refit: each chosen normal record becomes the normalised sum of the area-weighted normals of the faces
 * that use it, computed from the vertices as they are now.  All calls need MCPT_FLAG_DYNAMIC (else MCPT_ERR_UNSUPPORTED).
 *
 * mcpt_set_auto_normals: set-up, synchronous, the twin of mcpt_set_vertex_morph.  normal_mask: n_normal bytes, != 0 = recompute this record,
 * NULL = all.  It reads back the faces and the context's CURRENT vertices and normals, the REFERENCE POSE, and builds on the host, per normal
 * record, the list of the faces that name the record in any corner: one entry per face (also when two or three corners name it), ordered by
 * ascending face index of the description (never by leaf order: mcpt_rebuild_trees keeps the lists untouched, mcpt_clone_to_device carries them).
 * An entry is 16 bytes: the face's three vertex indices in corner order and `flip`.  With g = cross(v1 - v0, v2 - v0) at the reference pose and
 * n the record's reference normal, flip = ((g.x n.x + g.y n.y) + g.z n.z) < 0 (a zero or NaN dot: 0): a face whose winding disagrees with its
 * normal record at the reference pose goes on disagreeing, so the renderer's orientation rule holds.  Hard edges keep working: they are
 * separate normal records, and each record gathers only its own faces.  A record that is masked out or that no face uses has no entries and is
 * never written by the pass.  Allocates, counted in device_bytes: 4 B (n_normal + 1) (list offsets) + 16 B per entry (at most 3 per face).
 * Calling it again replaces the lists and takes the reference pose anew; mode MCPT_NORMALS_OFF frees them, and every update is again exactly
 * what it is without this section.
 *  - Refused with nothing changed: MCPT_ERR_INVALID_ARG for a NULL context, n_normal that differs from the scene's, a wrong struct_size, an
 *    unknown mode; MCPT_ERR_HIP when an allocation fails.
 *
 * The pass, per record with >= 1 entry, everything in fp64 and one correctly rounded operation each: s = +0; per entry in stored order
 * a = V[v1] - V[v0], b = V[v2] - V[v0], c = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), s = s + sigma c (sigma = -1 when flip,
 * else +1); len = sqrt((s.x s.x + s.y s.y) + s.z s.z); the record becomes s / len when len is finite and > 0 and is otherwise NOT written (it
 * keeps what the route wrote).  Area weighting is the only weighting: angle weighting needs acos, which is not correctly rounded.
 *  - For the records that have entries the pass OVERRIDES what the route wrote -- normals that the caller handed to mcpt_update_vertices
 *    included.  Mask out what the caller wants to supply itself.
 *  - The refit is handed the context's normals on every update, also after mcpt_update_vertices(normal = NULL).
 *  - mcpt_update_info::last_update_ms spans the pass; mcpt_normals_info::last_ms is the pass alone.
 *
 * mcpt_update_normals: the same update with no source -- nothing is staged, no vertex moves; the pass, then the usual refit (which reproduces
 * the trees: the call is idempotent).  Counted as one update; asynchronous on the context's stream; drops what mcpt_update_vertices drops.
 * MCPT_ERR_INVALID_ARG when auto normals are not set. */
#define MCPT_NORMALS_OFF  0u
#define MCPT_NORMALS_AREA 1u           /* area-weighted face normals, the only weighting */
typedef struct mcpt_normals_opts {
    uint32_t struct_size, mode;         /* MCPT_NORMALS_* */
    uint32_t reserved[4];
} mcpt_normals_opts;
mcpt_status mcpt_set_auto_normals(mcpt_ctx* ctx, const uint8_t* normal_mask /* n_normal bytes, != 0 = recompute; NULL = all */, uint32_t n_normal,
                                  const mcpt_normals_opts* opts /* NULL = MCPT_NORMALS_AREA */);
mcpt_status mcpt_update_normals(mcpt_ctx* ctx);   /* recompute now; nothing moves */
typedef struct mcpt_normals_info {
    uint32_t struct_size, mode;         /* MCPT_NORMALS_* in force now */
    uint32_t records, max_valence;      /* normal records with >= 1 entry; the largest number of entries of one record */
    uint64_t entries;                   /* entries of the per-record lists */
    uint32_t updates, reserved0;        /* passes run on this context so far: one per scene update while the mode was on */
    double   last_ms;                   /* device time of the last pass (HIP events) */
    uint32_t reserved[4];
} mcpt_normals_info;
mcpt_status mcpt_get_normals_info(mcpt_ctx* ctx, mcpt_normals_info* out);   /* synchronises */

/* ---- live scenes: new trees for the geometry as it is now -------------------------------------------------------------- */
/* mcpt_update_vertices and mcpt_update_transforms refit: after a large deformation the trees are sound and slow.  mcpt_rebuild_trees builds BOTH
 * trees (binary and 8-wide) anew for the context's current vertices -- whatever the last update or transform wrote -- and keeps everything else.
 *  - Needs MCPT_FLAG_DYNAMIC (else MCPT_ERR_UNSUPPORTED).  Works with both integrators and with MCPT_PIPELINE=mega.  `builder` chooses the host
 *    binned-SAH builder or the device PLOC builder; the device builder has mcpt_create's fallbacks (gave up, or too deep for the context's
 *    kernels: the host builder's tree, bvh_builder = 2) and mcpt_create's depth rule: a wavefront-only context may keep a deep device tree.
 *  - SYNCHRONOUS, and ordered like every call: it drains the context first, so renders enqueued before it walked the old trees; when it returns
 *    the new ones are in place.
 *  - Coordinates stay relative to the CREATION-time centre: mcpt_scene_info::centre and the camera constants do not change.  The builders see
 *    the faces in Model::face order with the bounds mcpt_create would form for them, so whenever a fresh mcpt_create of the same geometry would
 *    choose the same centre the rebuilt context IS that fresh context: wide_tree_hash, the leaf order, every triangle stream bit for bit, the
 *    deterministic film.
 *  - A triangle's tie rank becomes its new leaf position, as mcpt_create gives it; with MCPT_FLAG_REFERENCE_TIE_ORDER every triangle keeps the
 *    rank it has (the creation geometry's, as mcpt_update_vertices documents).
 *  - KEPT, because the scene looks the same from every pixel: the film or a bound accumulator, the counters, the stream binding, the camera, the
 *    feature buffers and the denoised film, the adaptive tile error, the reprojection buffers, the vertex groups with their rest pose and R_g,
 *    the skin with its rest pose and R_b, the morph targets with their rest pose, R and D_k (and the morph-then-skin scratch), the keyframes with their options and captured pose (§22), the owners of the parts update (§23: per record, not per leaf), the auto-normals lists (§20: they are per face of the description, not per leaf), the visibility mask (§24: per face too; the builders see a hidden face with the bounds of its vertices, the permuted streams keep it hidden, the next update tightens the boxes again), the materials, the textures, and the light list's membership and order (only the lights' leaf-order
 *    triangle index is renumbered).
 *  - Afterwards mcpt_update_info::wide_area_ratio is 1.0 (its base is the new tree) and `updates` is unchanged; mcpt_scene_info follows the new
 *    trees: n_nodes, bvh_depth, max_leaf, wide_nodes, wide_depth, traversal_bytes, wide_tree_hash, bvh_builder, and device_bytes counts what is
 *    allocated now; bvh_build_ms and upload_ms stay creation's.
 *  - A refusal changes NOTHING, not a buffer and not a field of an info: MCPT_ERR_INVALID_ARG for a NULL context, a struct_size that is not this
 *    library's or an unknown builder; MCPT_ERR_BVH_DEPTH where mcpt_create would answer it for the new tree (binary depth; the 512-MB cap of the
 *    traversal stack's overflow area, which is sized from the new wide_depth before anything walks the tree); MCPT_ERR_HIP for an allocation or
 *    builder failure.  Needs room for a second copy of the triangle streams while it runs.
 *  - A clone taken afterwards is a clone of the rebuilt context; clones taken earlier keep their own trees. */
#define MCPT_REBUILD_SAME   0u   /* the builder the context was created with (MCPT_FLAG_GPU_BVH_BUILD or not) */
#define MCPT_REBUILD_HOST   1u   /* host binned-SAH builder */
#define MCPT_REBUILD_DEVICE 2u   /* device PLOC builder, with create's fallbacks (gave up / too deep -> host, bvh_builder = 2) */
typedef struct mcpt_rebuild_opts { uint32_t struct_size, builder; uint32_t reserved[4]; } mcpt_rebuild_opts;
typedef struct mcpt_rebuild_info {
    uint32_t struct_size, rebuilds;     /* successful mcpt_rebuild_trees calls on this context */
    double   last_ms;                   /* wall time of the last call, entry to return */
    double   last_build_ms;             /* its tree construction (what bvh_build_ms is for mcpt_create) */
    double   last_device_ms;            /* HIP events: the bounds kernel + the permutation and light kernels */
    double   area_ratio_before;         /* wide_area_ratio just before the last call */
    uint32_t reserved[4];
} mcpt_rebuild_info;
mcpt_status mcpt_rebuild_trees(mcpt_ctx* ctx, const mcpt_rebuild_opts* opts /* NULL = defaults */);
mcpt_status mcpt_get_rebuild_info(mcpt_ctx* ctx, mcpt_rebuild_info* out);

/* ---- live scenes: faces shown and hidden on the device ------------------------------------------------------------------------ */
/* The face list of a context is fixed at mcpt_create; which of those faces EXIST for the rays is not.  A context holds one visibility byte per
 * face of the description, in Model::face order (!= 0 = visible).  A door taken away, a prop that pops in on frame 40, a lamp switched off as
 * geometry: one call, no new upload, no new trees, the film kept.  All calls need MCPT_FLAG_DYNAMIC (else MCPT_ERR_UNSUPPORTED).
 *
 * The mask is STICKY: every later scene update, by any route (mcpt_update_vertices, _transforms, _skin, _morph, _keyframes, _parts, _normals and
 * their _reproject forms), applies it again.  With no mask set every call enqueues exactly the kernels it enqueues without this section.  After
 * any update on a context with a mask, for every triangle whose face is hidden: record 0 of its intersection stream (first corner, lobe class,
 * tie rank) is what the update wrote; both edge records are {+0, +0, +0, 0}, so the determinant of the one triangle test every kernel shares is
 * exactly +-0 for every ray and NO kernel of the library -- wavefront trace, binary cross-check, first hit, features -- can accept it; its refit
 * box is the point of its first corner, so it no longer inflates its ancestors' boxes and mcpt_probe_validate_trees stays sound; its shading
 * records and fp64 corners stay as the update wrote them.  Visible triangles hold, bit for bit, what they hold without a mask.
 *
 * The light list's membership becomes |radiance| > 0.01 AND visible, still in face order; it is rebuilt on the device whenever the mask changes,
 * and mcpt_update_materials on a context with a mask applies the same rule.  A call -- of either kind -- that would leave no visible light is
 * refused with MCPT_ERR_NO_LIGHTS and changes nothing.  mcpt_scene_info::n_lights and mcpt_material_info::n_lights follow the list.
 *
 * mcpt_set_face_visibility: `visible` = n_face bytes, or NULL = every face visible and the mask freed (device_bytes is what it was before the
 * first call, but for the 4 B per face + 4 B per 256 faces of scan scratch that mcpt_update_materials also allocates on first use and that stay).
 * The bytes are copied before the call returns (staged in pinned memory, sent in stream order).  The call IS a scene update without a source: no
 * vertex moves; the triangle streams are rewritten from the vertices as they are, the hidden faces hidden, the light list rebuilt, both trees
 * refitted -- on the context's stream, ordered like mcpt_update_vertices, asynchronous.  mcpt_get_update_info counts one update; film and
 * counters are untouched; features, the denoised film and the tile error are dropped.  Allocates 1 B per face, counted in device_bytes.
 *  - Validated on the host before any device work; a refusal changes nothing.  In this order: MCPT_ERR_UNSUPPORTED without MCPT_FLAG_DYNAMIC;
 *    MCPT_ERR_INVALID_ARG for n_face that differs from the scene's (also with a NULL mask); MCPT_ERR_NO_LIGHTS when no emissive face under the
 *    current materials would stay visible.
 * mcpt_set_face_visibility_reproject is mcpt_update_vertices_reproject with the mask in place of the upload; validation order: the above, the
 * camera (when given), the options, MCPT_ERR_BVH_DEPTH.
 *
 * mcpt_clone_to_device carries the mask and the records as they are.  mcpt_rebuild_trees keeps the mask (it is per face, not per leaf): the
 * builders see a hidden face with the bounds of its vertices, as if it were visible, and the streams are permuted as they are, so hidden stays
 * hidden; the next update tightens the boxes again.  (A builder that skips hidden faces does not exist.)
 *
 * mcpt_probe_triangles: per face, in Model::face order, the nine floats {first corner, edge 1, edge 2} of its intersection records and the six
 * {lo, hi} of its refit box, as the device holds them; either output may be NULL.  The boxes are scratch of the scene update: asking for them
 * before the first update after creation or after mcpt_rebuild_trees is MCPT_ERR_INVALID_ARG.  Synchronous; touches nothing. */
typedef struct mcpt_visibility_info {
    uint32_t struct_size, set;          /* 1: a mask is in force now */
    uint32_t n_hidden;                  /* faces it hides */
    uint32_t n_hidden_emitters;         /* ... of those, faces whose material emits (|radiance| > 0.01) under the current materials */
    uint32_t updates, reserved0;        /* mcpt_set_face_visibility (+ _reproject) calls that shaped this context so far */
    double   last_ms;                   /* device time of the last update's hide pass and, where the mask changed, its light rebuild */
    uint64_t device_bytes;              /* what the mask holds on the device now */
    uint32_t reserved[4];
} mcpt_visibility_info;
mcpt_status mcpt_set_face_visibility(mcpt_ctx* ctx, const uint8_t* visible /* n_face bytes, != 0 = visible; NULL = all visible, frees the mask */, uint32_t n_face);
mcpt_status mcpt_set_face_visibility_reproject(mcpt_ctx* ctx, const uint8_t* visible, uint32_t n_face, const mcpt_camera* camera /* NULL = keep */,
                                               const mcpt_reproject_opts* opts /* NULL = defaults */);
mcpt_status mcpt_get_visibility_info(mcpt_ctx* ctx, mcpt_visibility_info* out);   /* synchronises */
mcpt_status mcpt_probe_triangles(mcpt_ctx* ctx, float* out_v0e1e2 /* 9 per face */, float* out_box6 /* 6 per face */);   /* face order; either may be NULL */

/* ---- camera models ---------------------------------------------------------------------------------------------------------- */
/* A ray-generation stage in front of the unchanged render kernels: mcpt_render_camera writes one primary ray per pixel for the model set here
 * (a HIP kernel, csrc/camera.hip) and hands the rays to the wavefront pipeline through the hook mcpt_probe_paths uses, once per sample.  A path
 * of pixel p and sample s draws exactly the random numbers mcpt_render draws for (p, s); the lens sample comes from the camera block's two spare
 * numbers.  With MCPT_CAMERA_PINHOLE the stage reproduces mcpt_render's film bit for bit.
 *
 * The models, with the camera frame of mcpt_set_camera (front, right, `up` as given, h = 2 tan(fovy / 2)), (u, v) the pinhole's image-plane
 * coordinates of the jittered pixel point and (u0, v0) in [-1/2, 1/2) its position on the film:
 *   PINHOLE       origin eye, direction normalize(front + u right + v up): mcpt_render's camera.
 *   THIN_LENS     D = front + u right + v up; the ray leaves the lens point eye + lens_radius (lx right + ly lup), lup = cross(right, front), towards
 *                 eye + focus_distance D.  What the pinhole sees at distance focus_distance along `front` is sharp; lens_radius 0 is the pinhole.
 *                 (lx, ly): uniform on the unit disk (blades 0) or on the regular polygon of `blades` corners, the first at angle blade_rotation.
 *                 An `up` that is not orthogonal to `front` shears the image exactly as it shears the pinhole's: the plane in focus is the pinhole
 *                 image of that camera.  Documented, not corrected.
 *   ORTHOGRAPHIC  origin eye + (u0 ortho_height width / height) right + (v0 ortho_height) up, direction front.  fovy is ignored.
 *   EQUIRECT      origin eye, direction cos(phi) (cos(lambda) front + sin(lambda) right) + sin(phi) lup with lambda = 2 pi u0, phi = pi v0: the whole
 *                 sphere, the view direction in the film's centre.  fovy is ignored; any film shape is accepted.
 *
 * mcpt_set_camera_model: validated on the host, a refusal changes nothing: MCPT_ERR_INVALID_ARG for a struct_size that is not this library's, an
 * unknown model, or a field of the CHOSEN model outside its range below (fields of other models are ignored).  NULL = PINHOLE.  Works on every
 * context; free.  mcpt_set_camera keeps the model (its parameters are relative to the camera frame); mcpt_clone_to_device carries the model
 * and not the ray buffers.
 *
 * ONLY mcpt_render_camera and mcpt_probe_camera_rays look at the model.  mcpt_render, mcpt_render_tiles, mcpt_render_tile_list,
 * mcpt_render_adaptive, mcpt_render_features, mcpt_probe_first_hits, the reprojection calls and mcpt_denoise's guide describe the PINHOLE view
 * whatever model is set: a denoised, reprojected or adaptively sampled film of another model is guided by features that do not belong to it.
 * Carrying the models into those kernels is follow-up work.
 *
 * mcpt_render_camera: adds `spp` samples (first_sample .. first_sample + spp - 1 of `seed`) of the set model to every pixel of the bound film; on
 * the context's stream, ordered like mcpt_render.  One pass per sample: the ray kernel, then the wavefront pipeline over width * height
 * one-sample items -- a many-sample still pays the per-pass overhead that mcpt_render's batching avoids (DESIGN.md §25 has the numbers).  Counted as
 * ONE launch in mcpt_counters, its paths and rays like mcpt_render's.  The two ray buffers (48 B per pixel together) are allocated by the first
 * call and counted in mcpt_scene_info::device_bytes.  spp == 0 does nothing.  MCPT_ERR_UNSUPPORTED without the wavefront pipeline
 * (MCPT_INTEGRATOR_RECURSIVE_NEE, MCPT_PIPELINE=mega); MCPT_ERR_INVALID_ARG when first_sample + spp > 2^32 or the film has more than
 * 67 108 863 pixels (what one mcpt_probe_paths call takes).
 *
 * mcpt_autofocus: the focus_distance that makes pixel (px, py) sharp: t dot(d, front) for the pixel-centre pinhole ray's direction d and its
 * first hit at t (the kernel behind mcpt_probe_first_hits).  MCPT_ERR_INVALID_ARG for a pixel outside the film or a ray that hits nothing;
 * MCPT_ERR_BVH_DEPTH where mcpt_probe_first_hits answers it.  Synchronous; touches nothing (the model included: pass the value on).
 *
 * mcpt_probe_camera_rays: the stage's device function for n pixels (xy: 2 ints each, inside the film) of sample `sample`: per ray the origin in
 * DEVICE coordinates (world less mcpt_scene_info::centre) and the direction (fp32 values), 3 doubles each.  Synchronous; touches nothing. */
#define MCPT_CAMERA_PINHOLE      0u
#define MCPT_CAMERA_THIN_LENS    1u
#define MCPT_CAMERA_ORTHOGRAPHIC 2u
#define MCPT_CAMERA_EQUIRECT     3u
#define MCPT_CAMERA_MAX_BLADES   16u
typedef struct mcpt_camera_model {
    uint32_t struct_size, model;          /* MCPT_CAMERA_* */
    double   lens_radius, focus_distance; /* THIN_LENS: radius finite and >= 0, focus finite and > 0 */
    uint32_t blades, reserved0;           /* THIN_LENS: 0 = disk, 3..16 = polygon */
    double   blade_rotation;              /* radians, finite */
    double   ortho_height;                /* ORTHOGRAPHIC: finite, > 0 */
    uint32_t reserved[4];
} mcpt_camera_model;
typedef struct mcpt_camera_model_info {
    uint32_t struct_size, model;          /* the model in force */
    uint32_t renders, reserved0;          /* mcpt_render_camera calls that enqueued work on this context */
    uint64_t passes;                      /* ... and their samples: one ray kernel each */
    double   last_stage_ms;               /* HIP events: the ray kernels of the last call, summed */
    uint64_t device_bytes;                /* what the ray buffers hold on the device now */
    uint32_t reserved[4];
} mcpt_camera_model_info;
mcpt_status mcpt_set_camera_model(mcpt_ctx* ctx, const mcpt_camera_model* model /* NULL = PINHOLE */);
mcpt_status mcpt_get_camera_model(mcpt_ctx* ctx, mcpt_camera_model* out, mcpt_camera_model_info* out_info /* may be NULL; not NULL: synchronises */);
mcpt_status mcpt_render_camera(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample);
mcpt_status mcpt_autofocus(mcpt_ctx* ctx, int32_t px, int32_t py, double* out_focus_distance);
mcpt_status mcpt_probe_camera_rays(mcpt_ctx* ctx, uint32_t n, const int32_t* xy, uint32_t sample, uint64_t seed,
                                   double* out_origin3 /* device coordinates */, double* out_dir3);

/* ---- surface baking ---------------------------------------------------------------------------------------------------------- */
/* Lighting seen from the surface instead of from a camera: lightmaps and per-vertex baked lighting (irradiance probes, points in free space
 * without a surface, are the next section's: mcpt_set_sh_probes).  A second ray-generation
 * stage (HIP kernels, csrc/bake.hip) starts one cosine-weighted ray per BAKE POINT on the scene's surfaces and hands the rays to the unchanged
 * wavefront pipeline through the hook mcpt_probe_paths and mcpt_render_camera use; the finished samples land in a film of the context's own
 * with one {sum L, count} record per point, never in the bound film.
 *
 * A bake point is {face, u, v, flags}: a face in Model::face order, barycentrics (the point is v0 + u (v1 - v0) + v (v2 - v0)) and
 * MCPT_BAKE_BACK_SIDE for the side the interpolated vertex normal points away from.  The stage reads the context's CURRENT corners and vertex
 * normals, so a bake after mcpt_update_* sees the scene as it is now.  A point whose interpolated normal AND geometric normal both have length 0
 * (or not finite) is DEAD: it is traced from its position along +z so that the pipeline sees a proper ray, and resolves to {0, 0, 0, 0}.
 * Item i of a pass is point i; its direction comes from random-number block 0 of (pixel = i, sample, seed) -- the camera's block -- and its path
 * draws blocks 1, 2, ... as every path does.
 *
 * DIRECT LIGHT (mcpt_set_bake_direct).  MCPT_BAKE_DIRECT_OFF, the default: direct light reaches a point only through cosine-sampled rays that hit
 * an emitter, which is noisy under small lamps; from the first hit on, paths sample the lights as always.  MCPT_BAKE_DIRECT_MIS adds next-event
 * estimation at the bake point itself, combined with the cosine ray by the power heuristic.  The record keeps its meaning (the mean of L over
 * cosine-weighted directions).  Per live item a kernel that takes the first-hit kernel's place (below) forms, in fp32:
 *   sub -- for the cosine ray's first hit: Le for an emitter met from behind (the rule below); (1 - w_b) Le for a LIGHT (|radiance| > 0.01) met from
 *          its front, with p_b = max(d.n, 0) / pi, p_l = t^2 / (cos_l n_lights area) (the pdf a later bounce uses) and w_b = p_b^2 / (p_b^2 + p_l^2);
 *          0 otherwise -- a faint emitter (0.0001 < |radiance| <= 0.01) is in no light list and keeps its full radiance;
 *   add -- one light sample from random-number block 0xFFFFFFFF of the item (a path would need 2^31 bounces to draw it): it counts if its pdf is finite
 *          and > 0 (a light seen from behind gives nothing), its distance exceeds 1e-4, cos_p = wo.n > 0 and the segment to it is free; then
 *          p_bl = cos_p / pi, p_lf = pdf / n_lights, w_l = p_lf^2 / (p_lf^2 + p_bl^2), add = w_l Le p_bl / p_lf.
 * and adds (add - sub) to the item's record before the pass.  The bake's own vertex ignores the light sample's self-occlusion verdict and always
 * behaves as MCPT_FLAG_CORRECT_SHADOW_T2 does: that quirk exists for parity with a reference that has no baker.  Everything from the first hit on
 * is the pipeline's, unchanged.  The stage's two traversals are not counted in mcpt_counters.
 *
 * mcpt_set_bake_direct: an unknown mode is MCPT_ERR_INVALID_ARG with nothing changed.  Works with or without points; the mode survives
 * mcpt_set_bake_points, mcpt_clear_bake and mcpt_rebuild_trees; a clone starts with OFF.  It holds for the passes enqueued after it and drains
 * nothing.  Costs no device memory.  mcpt_bake_info::direct_mode reports it.
 *
 * mcpt_probe_bake_direct: the kernel's device function for points first .. first + n - 1 and sample `sample`, whatever the mode, touching no film;
 * synchronous; either array may be NULL.  out12 per point: sub[3], add[3], w_b, w_l, p_b, p_l, p_bl, p_lf (terms not reached are 0: w_b, p_b, p_l
 * belong to a light met from its front; w_l, p_bl, p_lf to the states OCCLUDED and COUNTED).  out4 per point: the first-hit face in Model::face
 * order (-1 for a miss), whether it was met from its front (0 / 1), the sampled light's face, and MCPT_BAKE_DIRECT_STATE_*: DEAD (a dead point:
 * faces -1, all else 0), NO_PDF (pdf not positive or not finite, or distance <= 1e-4), BELOW (under the point's horizon), OCCLUDED, COUNTED.
 * MCPT_ERR_BVH_DEPTH where mcpt_bake answers it.
 *
 * EMITTERS ARE ONE-SIDED FOR A BAKE POINT.  A point's ray enters the pipeline as a path's PRIMARY ray, whose hit on an emitter adds its radiance
 * whatever side it is hit from (a camera sees a lamp's back lit); later bounces see emitters from their front only, and a surface point's ray is
 * morally one of those.  So before each pass a first-hit kernel (the binary tree; about 0.4 ms per pass for 640 000 points) finds the rays that
 * first meet an emitter from behind and takes that radiance out of their records: such a sample contributes what its path gathers after that hit.
 * (With MCPT_BAKE_DIRECT_MIS the direct-light kernel does this in the same traversal.)
 * MCPT_ERR_BVH_DEPTH from mcpt_bake where mcpt_probe_first_hits answers it (a device-built binary tree deeper than the kernel's stack).
 *
 * mcpt_set_bake_points: synchronous set-up.  Validated on the host before any device work, a refusal changes nothing: MCPT_ERR_INVALID_ARG for a
 * NULL list with n > 0, a face outside [0, n_face), u or v not finite, u < 0, v < 0 or double(u) + double(v) > 1, an unknown flag bit, or
 * n > 67 108 863.  n = 0 drops the points and frees everything.  The context holds 16 B (the point) + 1 B (dead) + 16 B (bake film) per point
 * from this call on and 48 B per point more (the two ray arrays) from the first mcpt_bake on, all counted in mcpt_scene_info::device_bytes.
 * Setting points zeroes the bake film.  mcpt_rebuild_trees keeps points and bake film; mcpt_clone_to_device's clone starts without points.
 * Points on faces hidden by mcpt_set_face_visibility stay alive (hiding removes a face from what rays can hit, not its corners or normals):
 * they bake what the surface would receive with the hidden faces gone.
 *
 * mcpt_bake: adds `spp` samples (first_sample .. first_sample + spp - 1 of `seed`) to every point's bake-film record; on the context's stream,
 * asynchronous, one pass per sample like mcpt_render_camera, ONE launch in mcpt_counters, its paths and rays counted like mcpt_render's.  The
 * context's flags (MCPT_FLAG_CORRECT_SHADOW_T2, MCPT_FLAG_DETERMINISTIC ...) apply as they do there; a bake of one-sample items is reproducible
 * bit for bit with or without MCPT_FLAG_DETERMINISTIC.  Consecutive calls are ordered: a pass's ray kernel runs after the pass before it has
 * read its rays.  MCPT_ERR_UNSUPPORTED without the wavefront pipeline; MCPT_ERR_INVALID_ARG without points or when first_sample + spp > 2^32;
 * spp == 0 does nothing.  Touches neither the bound film nor the features, the denoised film, the tile error or the camera model.
 *
 * mcpt_clear_bake: zeroes the bake film (asynchronous).  mcpt_read_bake: 4 floats per point, synchronous -- with m = sum L / float(count) in fp32,
 * MCPT_BAKE_IRRADIANCE gives {float(pi) m, count} (for cosine-weighted directions E = pi mean L) and MCPT_BAKE_DIFFUSE {kd * m, count}, the
 * radiance a diffuse texel of that surface sends out, kd the point's Map_Kd colour at its interpolated uv; a dead point or a count of 0 gives
 * {0, 0, 0, 0}.  mcpt_read_bake_film: the raw {sum L, count}.
 *
 * mcpt_probe_bake_rays: the stage's device function for points first .. first + n - 1 of the set list and sample `sample`: per point the origin
 * in DEVICE coordinates, the direction (fp32 values), the unit normal the direction was sampled about (3 doubles each; any may be NULL) and the
 * dead byte.  Synchronous; touches nothing.
 *
 * mcpt_lightmap_points: HOST ONLY, no device: the texel-to-surface map of a width x height lightmap over the description's texcoords.  Texel
 * (i, j) has the centre ((i + 0.5) / width, (j + 0.5) / height); the faces are tested in Model::face order with fp64 edge functions and a texel
 * belongs to the LOWEST face whose three barycentrics are all >= 0.  A face whose uv area is 0 or not finite is skipped; uv is not wrapped.
 * Output in texel order: the point (barycentrics rounded to fp32, then clamped so that mcpt_set_bake_points accepts them, flags 0) and the texel
 * j * width + i.  *out_n is always set; capacity < *out_n is MCPT_ERR_INVALID_ARG with nothing written, as for mcpt_probe_lights. */
#define MCPT_BAKE_BACK_SIDE   1u          /* mcpt_bake_point::flags */
#define MCPT_BAKE_IRRADIANCE  0u          /* mcpt_read_bake's mode */
#define MCPT_BAKE_DIFFUSE     1u
#define MCPT_BAKE_DIRECT_OFF  0u          /* mcpt_set_bake_direct's mode */
#define MCPT_BAKE_DIRECT_MIS  1u
#define MCPT_BAKE_DIRECT_STATE_DEAD     0 /* mcpt_probe_bake_direct's out4[3] */
#define MCPT_BAKE_DIRECT_STATE_NO_PDF   1
#define MCPT_BAKE_DIRECT_STATE_BELOW    2
#define MCPT_BAKE_DIRECT_STATE_OCCLUDED 3
#define MCPT_BAKE_DIRECT_STATE_COUNTED  4
typedef struct mcpt_bake_point {
    uint32_t face;                        /* Model::face order */
    float    u, v;                        /* barycentrics of corners 1 and 2 */
    uint32_t flags;                       /* MCPT_BAKE_BACK_SIDE */
} mcpt_bake_point;
typedef struct mcpt_bake_info {
    uint32_t struct_size, n_points;
    uint32_t n_dead, bakes;               /* dead points as of the last mcpt_bake; mcpt_bake calls that enqueued work on this context */
    uint64_t passes;                      /* ... and their samples: one ray kernel each */
    double   last_stage_ms;               /* HIP events: the ray kernels of the last call, summed */
    uint64_t device_bytes;                /* points + dead bytes + bake film + ray arrays, as held now */
    union {                               /* (anonymous: C11, C++ and every C99 compiler in use) */
        uint32_t direct_mode;             /* MCPT_BAKE_DIRECT_*: reserved[0]'s word, which was always 0, so 0 keeps its meaning */
        uint32_t reserved[4];             /* [1] .. [3] stay reserved */
    };
} mcpt_bake_info;
mcpt_status mcpt_set_bake_points(mcpt_ctx* ctx, const mcpt_bake_point* points, uint32_t n);
mcpt_status mcpt_bake(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample);
mcpt_status mcpt_clear_bake(mcpt_ctx* ctx);
mcpt_status mcpt_read_bake(mcpt_ctx* ctx, uint32_t mode /* MCPT_BAKE_IRRADIANCE / _DIFFUSE */, float* out4 /* 4 per point */);
mcpt_status mcpt_read_bake_film(mcpt_ctx* ctx, float* out4 /* 4 per point */);
mcpt_status mcpt_get_bake_info(mcpt_ctx* ctx, mcpt_bake_info* out);                 /* synchronises */
mcpt_status mcpt_probe_bake_rays(mcpt_ctx* ctx, uint32_t sample, uint64_t seed, uint32_t first, uint32_t n, double* out_origin3 /* device coordinates */,
                                 double* out_dir3, double* out_normal3, uint8_t* out_dead);
mcpt_status mcpt_set_bake_direct(mcpt_ctx* ctx, uint32_t mode /* MCPT_BAKE_DIRECT_* */);
mcpt_status mcpt_probe_bake_direct(mcpt_ctx* ctx, uint32_t sample, uint64_t seed, uint32_t first, uint32_t n, float* out12 /* 12 per point */,
                                   int32_t* out4 /* 4 per point */);
mcpt_status mcpt_lightmap_points(const mcpt_scene_desc* scene, uint32_t width, uint32_t height, uint32_t capacity, mcpt_bake_point* out_points,
                                 uint32_t* out_texel, uint32_t* out_n);

/* ---- light probes: L2 spherical harmonics at free-space points ---------------------------------------------------------------- */
/* What an object that moves through a baked scene is lit by.  A LIGHT PROBE is a point in free space, no surface and no normal; it stores the
 * radiance arriving from all around it as 9 real spherical-harmonic coefficients per colour channel (bands l = 0, 1, 2; k = l (l + 1) + m):
 *   Y0 = 0.282095   Y1 = 0.488603 y   Y2 = 0.488603 z   Y3 = 0.488603 x   Y4 = 1.092548 x y   Y5 = 1.092548 y z
 *   Y6 = 0.315392 (3 z^2 - 1)   Y7 = 1.092548 x z   Y8 = 0.546274 (x^2 - y^2)
 * A third ray-generation stage (HIP kernels, csrc/shprobe.hip) starts 64 rays per probe and PASS, one wave64 per probe: item i of a pass is
 * probe i >> 6 and direction slot j = i & 63 of an 8 x 8 stratification of the sphere -- with (xi0, xi1) from random-number block 0 of
 * (pixel = i, sample, seed), u = ((j & 7) + xi0) / 8, v = ((j >> 3) + xi1) / 8: z = 1 - 2 u, r = 2 sqrt(u (1 - u)), phi = 2 pi v,
 * d = (r cos phi, r sin phi, z), fp64 rounded to fp32.  The rays go through the unchanged wavefront pipeline (the hook of mcpt_probe_paths,
 * mcpt_render_camera and mcpt_bake) into a scratch film of one record per item; a projection kernel then forms per item the 27 products
 * L_c Y_k(d) in fp32 (a component of L that is not finite counts as 0), sums the wave's 64 items in ONE fixed tree -- s[j] + s[j + 32], then
 * + 16, ... + 1; no atomics, so a bake is reproducible bit for bit and tests/shprobe_ref.py restates it to the bit -- and adds the sums to the
 * probe's 27 fp32 accumulators, 64 to its ray count and the pass's hits from behind and misses to two more counts.
 *
 * EMITTERS ARE ONE-SIDED FOR A PROBE, as for a bake point: before each pass a first-hit kernel (the binary tree) takes the radiance of an
 * emitter first met from BEHIND out of the item's record, and writes the item's class byte: 0 a miss, 1 a hit from the front, 2 a hit from
 * behind.  A probe whose share of back hits (counts[1] / counts[0]) is large sits inside geometry.
 *
 * mcpt_set_sh_probes: synchronous set-up; positions in WORLD coordinates, 3 doubles per probe.  Validated on the host before any device work, a
 * refusal changes nothing: MCPT_ERR_INVALID_ARG for a NULL list with n > 0, a coordinate that is not finite (the message names the first bad
 * probe) or n > 1 048 575 (a pass is one probe job of 64 n items).  n = 0 drops the probes and frees everything.  The context holds 24 B (the
 * position in device coordinates) + 108 B (accumulators) + 12 B (counts) per probe from this call on and, from the first mcpt_bake_sh on,
 * 64 x (48 B ray arrays + 16 B scratch film + 1 B class) per probe more, all counted in mcpt_scene_info::device_bytes.  Setting probes zeroes
 * accumulators and counts.  The context keeps the world positions: mcpt_rebuild_trees derives the device coordinates anew and keeps probes and
 * accumulators; mcpt_clone_to_device's clone starts without probes.
 *
 * mcpt_bake_sh: adds `passes` passes (samples first_sample .. first_sample + passes - 1 of `seed`) of 64 rays to every probe; mcpt_bake's
 * contract: on the context's stream, asynchronous, ONE launch in mcpt_counters, the context's flags apply, it reads the context's CURRENT scene
 * (after mcpt_update_* or mcpt_set_face_visibility: the scene as it is now).  MCPT_ERR_UNSUPPORTED without the wavefront pipeline;
 * MCPT_ERR_INVALID_ARG without probes or when first_sample + passes > 2^32; MCPT_ERR_BVH_DEPTH where mcpt_bake answers it; passes == 0 does
 * nothing.  Touches neither the bound film nor the bake film, the bake points, the features or the camera model.  (The ray count is a uint32:
 * it wraps after 2^26 passes without mcpt_clear_sh.)
 *
 * mcpt_clear_sh: zeroes accumulators and counts (asynchronous).  mcpt_read_sh: 27 floats per probe, channel-major (out[27 p + 9 c + k]),
 * synchronous: MCPT_SH_RADIANCE gives c[k] = (float(4 pi) / float(rays)) acc[k], the coefficients of the incident radiance, and
 * MCPT_SH_IRRADIANCE those times float(pi), float(2 pi / 3), float(pi / 4) for l = 0, 1, 2 (the cosine lobe's convolution), so that
 * mcpt_sh_eval gives the irradiance for a normal; all 0 where rays == 0.  mcpt_read_sh_film: the raw accumulators (27 per probe) and
 * {rays, hits from behind, misses} (3 uint32 per probe); either may be NULL.
 *
 * mcpt_probe_sh_rays: the stage's device function for items first_item .. first_item + n_items - 1 (item numbers included) of sample `sample`:
 * the origin in DEVICE coordinates and the direction (fp32 values), 3 doubles each; either may be NULL.  Synchronous; touches nothing.
 * mcpt_read_sh_pass: the scratch film (4 floats per item: the item's L and count 1) and the class bytes as the LAST pass left them; either may
 * be NULL; synchronises; MCPT_ERR_INVALID_ARG before the first pass of the set list.
 *
 * HOST ONLY, no device and no context: mcpt_sh_grid -- the cell centres of the box [lo, hi] cut into nx x ny x nz cells, x fastest, cell i at
 * lo + ((i + 0.5) / n) (hi - lo) per axis; *out_n is always set, capacity < *out_n is MCPT_ERR_INVALID_ARG with nothing written
 * (mcpt_lightmap_points' protocol); refused: a NULL bound, no cells or more than 1 048 575, a bound that is not finite, lo > hi.
 * mcpt_sh_eval -- out[c] = sum_k coeffs[9 c + k] Y_k(normal / |normal|) in fp64, k ascending; {0, 0, 0} for a normal of length 0. */
#define MCPT_SH_RADIANCE    0u            /* mcpt_read_sh's mode */
#define MCPT_SH_IRRADIANCE  1u
#define MCPT_SH_DIRECTIONS  64u           /* rays per probe and pass */
#define MCPT_SH_MAX_PROBES  1048575u
typedef struct mcpt_sh_info {
    uint32_t struct_size, n_probes;
    uint32_t bakes, reserved0;            /* mcpt_bake_sh calls that enqueued work on this context */
    uint64_t passes;                      /* ... and their passes: one ray, first-hit and projection kernel each */
    double   last_stage_ms;               /* HIP events: the ray and first-hit kernels (with the scratch film's fill) of the last call, summed */
    uint64_t device_bytes;               /* positions + accumulators + counts + ray arrays + scratch film + class bytes, as held now */
    uint32_t reserved[4];
} mcpt_sh_info;
mcpt_status mcpt_set_sh_probes(mcpt_ctx* ctx, const double* world_xyz /* 3 per probe */, uint32_t n);
mcpt_status mcpt_bake_sh(mcpt_ctx* ctx, uint32_t passes, uint64_t seed, uint32_t first_sample);
mcpt_status mcpt_clear_sh(mcpt_ctx* ctx);
mcpt_status mcpt_read_sh(mcpt_ctx* ctx, uint32_t mode /* MCPT_SH_RADIANCE / _IRRADIANCE */, float* out27 /* 27 per probe */);
mcpt_status mcpt_read_sh_film(mcpt_ctx* ctx, float* out27 /* 27 per probe */, uint32_t* out_counts3 /* 3 per probe */);
mcpt_status mcpt_get_sh_info(mcpt_ctx* ctx, mcpt_sh_info* out);                     /* synchronises */
mcpt_status mcpt_probe_sh_rays(mcpt_ctx* ctx, uint32_t sample, uint64_t seed, uint32_t first_item, uint32_t n_items, double* out_origin3 /* device coordinates */,
                               double* out_dir3);
mcpt_status mcpt_read_sh_pass(mcpt_ctx* ctx, float* out_film4 /* 4 per item */, uint8_t* out_class /* 1 per item */);
mcpt_status mcpt_sh_grid(const double* lo3, const double* hi3, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t capacity, double* out_xyz /* 3 per probe */,
                         uint32_t* out_n);
mcpt_status mcpt_sh_eval(const float* coeffs27, const double* normal3, double* out_rgb3);

/* ---- plumbing for multi-GPU hosts (one context per GPU / rank) ---------------------------------------- */
/* Use a caller-owned device buffer of width*height*4 floats as the accumulator (e.g. a torch tensor that
 * torch.distributed / RCCL all-reduces in place).  NULL re-binds the internal buffer. */
mcpt_status mcpt_bind_accum(mcpt_ctx* ctx, void* device_rgba);
mcpt_status mcpt_accum_device_ptr(mcpt_ctx* ctx, void** out_device_rgba);
/* Launch on a caller-owned hipStream_t.  NULL = back to the context's own (non-blocking) stream -- NOT the device's legacy
 * default stream, whose handle is also 0: a caller that wants its work ordered with the default stream (e.g. torch's
 * default stream, `cuda_stream == 0`) says so with mcpt_set_null_stream(). */
mcpt_status mcpt_set_stream(mcpt_ctx* ctx, void* hip_stream);
mcpt_status mcpt_set_null_stream(mcpt_ctx* ctx);

/* ---- function-level probes (what the parity tests call; each maps to one reference function) ---------- */
/* BVH::hit (BVH.cpp:90-113) / BVH::has_hit (BVH.cpp:115-136) for n host rays.  origin/dir: 3 doubles per ray.
 * t1,t2: per-ray interval.  Outputs (closest): t (fp32), triangle index in face order (-1 = miss), barycentric
 * u,v.  any_hit != 0: out_tri[i] = 1/0 only.  This is the binary-tree cross-check traversal: among triangles at EXACTLY the same distance
 * the first one in ITS traversal order wins (neither of the production kernel's tie rules: on coincident geometry it may name another face
 * than mcpt_probe_trace4 at the same t). */
mcpt_status mcpt_probe_trace(mcpt_ctx* ctx, uint32_t n, const double* origin, const double* dir,
                             const double* t1, const double* t2, int any_hit,
                             float* out_t, int32_t* out_tri, float* out_u, float* out_v);
/* The same two reference functions through the PRODUCTION traversal kernel (wf_trace8_kernel over the 8-wide compressed tree:
 * LDS top levels, LDS + global overflow group stack, chunked ray list): the rays are placed in a path pool the way the shade kernel
 * leaves them, the trace kernel runs once, results come back from the pool.  t1 is the kernel's fixed 1e-4 (Render.h:30);
 * closest-hit rays are unbounded (t2 = DBL_MAX like cast_Ray / BSDF rays), any-hit rays use t2[i] (Render.cpp:219-221).
 * Same outputs as mcpt_probe_trace. */
mcpt_status mcpt_probe_trace4(mcpt_ctx* ctx, uint32_t n, const double* origin, const double* dir, const double* t2, int any_hit,
                              float* out_t, int32_t* out_tri, float* out_u, float* out_v);
/* Render::cast_Ray (Render.cpp:71-80) for n (x,y) pixels with the xi the caller supplies (2 per ray). */
/* Triangle::hit's shading record (Triangle.cpp:68-76: interplote_Normal, normalize, interplote_uv, front = dot(n, d) < 0) for hits the
 * caller got from mcpt_probe_trace4: `face` = Model::face index, (u, v) = the hit's barycentrics, dir = the ray's direction.
 * out6 per hit = normal xyz | uv | front (1 / 0). */
mcpt_status mcpt_probe_hit_shade(mcpt_ctx* ctx, uint32_t n, const int32_t* face, const float* u, const float* v, const double* dir, float* out6);
mcpt_status mcpt_probe_cast_ray(mcpt_ctx* ctx, uint32_t n, const int32_t* xy, const float* xi, float* out_origin_dir6);
/* BSDF (BSDF.cpp:87-202) on synthetic hits: per item normal[3], wi[3], kd[3], ks[3], ns, wo[3] (world) and 3 xi
 * {lobe, xi1, xi2}.  out per item: Fx(wo)[3], Pdf(wo), sample.wo[3], sample.f[3], sample.pdf, isMirror = 12 floats */
mcpt_status mcpt_probe_bsdf(mcpt_ctx* ctx, uint32_t n, const float* normal, const float* wi, const float* kd,
                            const float* ks, const float* ns, const float* wo, const float* xi, float* out12);
/* Render::sample (Render.cpp:202-223) from n shading points (3 doubles each) with 3 xi each.
 * out per item: wo[3], radiance[3], pdf, t2, light triangle index (as float), self_hit (0/1; the fp64 predicate
 * of SURVEY A-9 evaluated on the sampled triangle only) = 10 floats */
mcpt_status mcpt_probe_sample_light(mcpt_ctx* ctx, uint32_t n, const double* point, const float* xi, float* out10);
/* One full path per item through the shipping integrator from a given ray, random numbers from the counter-based
 * generator keyed (seed, pixel = item, sample = 0).  out: L[3].  Runs the production wavefront pipeline (wf_shade_kernel +
 * wf_trace8_kernel over a path pool, item = entry of an n x 1 film); the cross-check megakernel only under MCPT_PIPELINE=mega. */
mcpt_status mcpt_probe_paths(mcpt_ctx* ctx, uint32_t n, const double* origin, const double* dir, uint64_t seed, float* out_L3);
/* Texture::get_color (model.cpp:30-41) of material `material`'s Map_Kd for n (u, v) pairs (fp32, as the device interpolates them):
 * nearest texel, fract + clamp01's 0.999 cap, no v flip; a 1x1 texture returns its constant colour.  A uv that is not finite is refused on the
 * host (MCPT_ERR_INVALID_ARG, nothing enqueued): no scene mcpt_create accepts can produce one. */
mcpt_status mcpt_probe_texture(mcpt_ctx* ctx, uint32_t material, uint32_t n, const float* uv2, float* out_rgb3);
/* The generator itself: n*4 uniforms for (pixel, sample, block) triples -- pins oracle and device to one stream. */
mcpt_status mcpt_probe_rng(mcpt_ctx* ctx, uint32_t n, const uint32_t* pixel_sample_block3, uint64_t seed, float* out4);

#ifdef __cplusplus
}
#endif
#endif /* MCPT_H */
