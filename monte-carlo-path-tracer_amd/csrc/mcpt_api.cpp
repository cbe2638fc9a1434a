// C ABI of libmcpt_hip.so (include/mcpt.h): context management, HBM upload, kernel launches.
// No CPU path exists in this file: every compute entry point launches a gfx950 kernel or fails.
#include "../../include/mcpt.h"
#include "kernels.h"
#include "scene_build.h"
#include "bvh_gpu.h"
#include "wavefront.h"
#include "wf_plan.h"
#include "denoise.h"
#include "adaptive.h"
#include "refit.h"
#include "rebuild.h"
#include "rebuild_plan.h"
#include "transform.h"
#include "skin.h"
#include "morph.h"
#include "keyframes.h"
#include "parts.h"
#include "normals.h"
#include "reproject.h"
#include "materials.h"
#include "visibility.h"
#include "visibility_plan.h"
#include "camera.h"
#include "bake.h"
#include "bake_plan.h"
#include "shprobe.h"
#include "shprobe_plan.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

namespace {

thread_local std::string g_err;

// Owners of what a context holds on the device: move-only, each gives its handle back when it dies, so `delete` of a context frees all of it.
template <class H, auto Free> struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Owned() { if (h) (void)Free(h); }
    operator H() const { return h; }
    H* out() { return &h; }            // for the hip*Create / hipHostMalloc call that fills an empty owner
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
template <class T> using Pinned = Owned<T*, hipHostFree>;

// The duration of the last refit / reprojection call: an event pair around its stream work, read once -- by the next begin() or by whoever asks
// for last_ms after settle() -- and kept.  (The render calls' ring, mcpt_ctx::ev0 / ev1, is a different thing: many calls outstanding.)
struct Stopwatch {
    Event ev0, ev1; bool timed = false; double last_ms = 0.0;
    hipError_t create() { const hipError_t e = hipEventCreate(ev0.out()); return e != hipSuccess ? e : hipEventCreate(ev1.out()); }
    hipError_t settle() {                                // waits for the bracketed work
        if (!timed) return hipSuccess;
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(ev1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
        if (e == hipSuccess) { last_ms = ms; timed = false; }
        return e;
    }
    hipError_t begin(hipStream_t s) { const hipError_t e = settle(); return e != hipSuccess ? e : hipEventRecord(ev0, s); }   // (the last duration is read before the events are recorded again)
    hipError_t end(hipStream_t s) { const hipError_t e = hipEventRecord(ev1, s); timed = e == hipSuccess; return e; }
};

// A pinned host buffer that is filled by the host, copied to the device in stream order and filled again by the next call.  `copied`: the last
// copy out of it has been made, it may be written again.
template <class T> struct Staging {
    Pinned<T> host; size_t cap = 0; Event copied; bool pending = false;
    hipError_t wait() {                                  // until the buffer may be written
        const hipError_t e = pending ? hipEventSynchronize(copied) : hipSuccess;
        if (e == hipSuccess) pending = false;
        return e;
    }
    // elements [at, at + n) to `dev` on `s`; `last`: no further copy of this filling follows -- the event is recorded
    hipError_t send(T* dev, size_t at, size_t n, hipStream_t s, bool last = true) {
        hipError_t e = hipMemcpyAsync(dev, host + at, n * sizeof(T), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && last) { e = hipEventRecord(copied, s); pending = e == hipSuccess; }
        return e;
    }
    hipError_t grow(size_t n) {                          // to n elements, after wait(); the contents are not kept, and nothing changes on failure
        if (n <= cap) return hipSuccess;
        Pinned<T> h;
        hipError_t e = hipHostMalloc(h.out(), n * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess && !copied) e = hipEventCreateWithFlags(copied.out(), hipEventDisableTiming);
        if (e == hipSuccess) { host = std::move(h); cap = n; }
        return e;
    }
};

// A device buffer of `T`s.  `tally` (the context's mcpt_scene_info::device_bytes, or null for a buffer that is not counted) follows the allocation:
// it grows by `bytes` when the buffer is allocated and shrinks when it is released, regrown or destroyed.
template <class T> struct DevBuf {
    T* p = nullptr; size_t bytes = 0; uint64_t* tally = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), tally(o.tally) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(tally, o.tally); return *this; }
    ~DevBuf() { release(); }
    size_t count() const { return bytes / sizeof(T); }
    void release() { if (p) { (void)hipFree(p); if (tally) *tally -= bytes; } p = nullptr; bytes = 0; }
    hipError_t alloc(size_t n, uint64_t* counted = nullptr) {             // n elements
        release();
        const hipError_t e = hipMalloc(&p, n ? n * sizeof(T) : 16);
        if (e == hipSuccess) { bytes = n * sizeof(T); tally = counted; if (tally) *tally += bytes; } else p = nullptr;
        return e;
    }
};
using DevBytes = DevBuf<unsigned char>;                // the rows of ensure_pool's table: element sizes differ from row to row

// "Allocate a group into locals, commit all or none": every wanted owner (`on`) is allocated afresh, in the order given, and only when all of
// them are there do they replace their destinations.  On a failure the fresh ones die and the context is as it was, its tally included.
template <class O> struct Want {
    O& dst; size_t n; uint64_t* tally; bool on;
    Want(O& d, size_t n_ = 1, uint64_t* t = nullptr, bool on_ = true) : dst(d), n(n_), tally(t), on(on_) {}
};
template <class T> hipError_t alloc_fresh(DevBuf<T>& b, size_t n, uint64_t* tally) { return b.alloc(n, tally); }
template <class T> hipError_t alloc_fresh(Pinned<T>& h, size_t n, uint64_t*) { return hipHostMalloc(h.out(), n ? n * sizeof(T) : 16, hipHostMallocDefault); }
template <class T> hipError_t alloc_fresh(Staging<T>& s, size_t n, uint64_t*) { return s.grow(n); }
inline hipError_t alloc_fresh(Stopwatch& w, size_t, uint64_t*) { return w.create(); }
template <class... O> hipError_t alloc_all(Want<O>... w) {
    std::tuple<O...> fresh;
    hipError_t e = hipSuccess;
    std::apply([&](O&... f) { ((e = e != hipSuccess || !w.on ? e : alloc_fresh(f, w.n, w.tally)), ...); }, fresh);
    if (e == hipSuccess) std::apply([&](O&... f) { ((w.on ? void(w.dst = std::move(f)) : void()), ...); }, fresh);
    return e;
}

mcpt_status fail(mcpt_status s, const std::string& msg) { g_err = msg; return s; }
mcpt_status hip_fail(hipError_t e, const char* what) { g_err = std::string(what) + ": " + hipGetErrorString(e); return MCPT_ERR_HIP; }
#define HIP_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(e_, #call); } while (0)

}  // namespace

struct mcpt_ctx {
    int device = 0;
    mcpt_opts opts{};
    DevScene dev{};
    DevBuf<float4> nodes, nodes8, tri_isect, tri_shade, texels, accum_own;
    DevBuf<double> tri_pos64, light_pos64;
    DevBuf<int32_t> tri_face; DevBuf<DevMaterial> mats; DevBuf<DevLight> lights; DevBuf<DevCounters> counters;   // (counters: WF_COUNTER_REPLICAS of them)
    float4* accum = nullptr;           // bound accumulator (own or external)
    Stream own_stream; hipStream_t stream = nullptr;   // the stream in use: own_stream, the caller's (mcpt_set_stream) or the default stream
    // HIP-event brackets of the render calls whose duration has not been read yet: a ring, so that a call does not have to wait for the one
    // before it (the reference's loop issues a call per sample); resolve_timing() reads the finished ones, oldest first
    static constexpr uint32_t TIMED = 16;
    Event ev0[TIMED], ev1[TIMED];
    uint32_t timed_head = 0, timed_tail = 0;      // calls [timed_tail, timed_head) are outstanding
    double last_kernel_ms = 0.0, total_kernel_ms = 0.0;
    uint64_t launches = 0;
    mcpt_scene_info info{};
    int width = 0, height = 0;
    // ---- wavefront pipeline (the default for MCPT_INTEGRATOR_MIS)
    bool use_wavefront = true;
    // Sub-pipelines ("lanes"): each owns a path pool, a control block and a stream and runs its own [shade, trace] loop on its
    // share of the sample range.  Two of them in flight let the issue-bound shade kernel of one overlap the memory-bound trace
    // kernel of the other on the same CUs (measured +15 % on MI355X).
    struct WfLane {
        PathPool pool{};
        CompactBufs compact{};             // scratch of the end-of-job drain compaction (wavefront.h); capacity 0 = none (small pools)
        std::vector<DevBytes> pool_bufs;
        DevBuf<IterCtl> ctl_buf; DevBuf<int> ovf_buf;
        Pinned<IterCtl> h_ctl;             // pinned ring of control-block snapshots (termination check)
        std::vector<Event> chk_ev;
        std::vector<Event> k_ev;           // per-kernel event chain (only with detailed timing)
        Stream stream;
        Event done_ev;
        Event shade_ev;                    // recorded after each shade launch of a gated sub-pipeline: what the next one's shade launch waits for (wf_plan.h: wf_shade_wait)
        uint64_t last_iterations = 0, last_timed = 0;
        // Known-length jobs (every item has its own slot and one sample, depth-limited: wf_plan_call) are enqueued whole and NOT waited for:
        // the control-block snapshot taken after their last iteration is looked at later -- by the next call that drains the stream, or when the
        // ring of snapshots is full -- so consecutive one-sample calls (the reference's loop, main.cpp:26-33) cost the host only their launches.
        struct Verdict { uint32_t ring_slot, it, n_shared; };
        std::vector<Verdict> verdicts;     // oldest first; at most RING - 2 outstanding
        uint32_t ring_next = 0;            // next h_ctl / chk_ev slot this lane uses (jobs of either kind take them in turn)
    };
    std::vector<WfLane> lanes;
    Event fork_ev;
    WaveTuning tune{};
    uint32_t trace_grid = 0;
    WfKnobs knobs{};                    // the scheduler's environment knobs, read by finish_ctx and by nobody after it (wf_plan.h)
    int n_cus = 0;
    double last_trace_ms = 0.0, total_trace_ms = 0.0, last_shade_ms = 0.0, total_shade_ms = 0.0;
    uint64_t total_iterations = 0;
    bool binary_ok = true;                // the binary cross-check tree fits its kernels' stack (false: a deep device-built tree)
    uint32_t wide_depth = 0;              // depth of the 8-wide tree the wavefront trace kernel walks
    std::vector<int32_t> h_tri_face;      // leaf order -> face index, fetched on first use by mcpt_probe_trace4
    // Scene::getPixelsColor every frame (main.cpp:26-33): the tonemapped film's device buffer and its pinned host image live as long as the
    // context (allocated by the first tonemap call) -- nothing is allocated, cleared or released per frame
    DevBuf<uint8_t> tone_dev; Pinned<uint8_t> tone_host;
    // Denoised preview (denoise.hip): first-hit features (2 float4 / pixel), allocated by the first mcpt_render_features; the filter's guide,
    // two ping-pong {irr, var} buffers and the denoised film (1 float4 / pixel each), allocated by the first mcpt_denoise
    DevBuf<float4> dn_feat, dn_guide, dn_iv0, dn_iv1, dn_out;
    bool dn_have_features = false, dn_have_out = false;
    // The emission buffer of MCPT_DENOISE_SPLIT_EMISSION (1 float4 / pixel), allocated by the first mcpt_denoise that asks for the split; from
    // then on every feature render fills it in the same traversal.  dn_feat_spp / dn_feat_seed: what the features held were rendered with.
    DevBuf<float4> dn_emis;
    bool dn_have_emis = false;
    uint32_t dn_feat_spp = 0; uint64_t dn_feat_seed = 0;
    // mcpt_render_tile_list: the caller's list, staged in pinned memory and copied to the device in stream order; both grow to the longest list seen
    DevBuf<uint32_t> tl_dev; Staging<uint32_t> tl_stage;
    // Adaptive sampling (adaptive.hip), allocated by the first mcpt_render_adaptive: the half films H and O (1 float4 / pixel each), per tile
    // E_t, the active list and its flags, per error block counts and offsets, the totals and their pinned read-back
    DevBuf<float4> ad_h, ad_o; DevBuf<float> ad_err; DevBuf<uint32_t> ad_list, ad_flags, ad_offs; DevBuf<uint4> ad_counts; DevBuf<AdTotals> ad_tot;
    Pinned<AdTotals> ad_host;
    bool ad_have_err = false;
    // Live scenes (refit.hip).  MCPT_FLAG_DYNAMIC only: per triangle its vertex and normal indices (leaf order), the device copy of
    // the caller's vertices / normals and its pinned staging, per triangle and per 8-wide node an fp32 box (refit scratch), the binary nodes sorted
    // by height and the level boundaries of both trees (one launch per level), the per-block partial sums of the wide tree's box areas.
    // rf_vtx / rf_nrm hold the scene's CURRENT vertices and normals from creation on (§14 reads them as "the scene before this update").
    bool dynamic = false;
    uint32_t rf_n_vertex = 0, rf_n_normal = 0;
    DevBuf<int32_t> rf_idx; DevBuf<double> rf_vtx, rf_nrm, rf_area; DevBuf<float> rf_tri_box, rf_node_box; DevBuf<uint32_t> rf_bin_order;
    std::vector<uint32_t> rf_bin_level, rf_wide_level;      // [k], [k + 1]: the nodes of height k in rf_bin_order / the records of depth k in nodes8
    std::vector<uint8_t> rf_used_vertex;                    // a face uses this vertex: it is validated
    Staging<double> rf_stage;                               // the vertices, then the normals
    Stopwatch rf_watch;
    uint32_t rf_updates = 0; double rf_area0 = 0.0;
    // Tree rebuilds (rebuild.hip): what mcpt_get_rebuild_info reports.  The call owns its temporaries; nothing of it stays allocated.
    uint32_t rb_rebuilds = 0; double rb_last_ms = 0.0, rb_last_build_ms = 0.0, rb_last_device_ms = 0.0, rb_area_before = 1.0;
    // One record per deformer that feeds the refit (Groups, Skin, Morph) and one for the normals pass: its device buffers (counted in device_bytes),
    // pinned stage, host radii, the Stopwatch of its stream work and its `updates` counter.  alloc(): the buffers afresh, all or none -- a context
    // that had the record keeps it when an allocation fails.  clone_from(): what travels with mcpt_clone_to_device, each buffer named once.
    struct RestPose { DevBuf<double> vtx, nrm; };             // the scene as the record's set call found it: rf_vtx's and rf_nrm's sizes
    // Rigid parts (transform.hip), allocated by mcpt_set_vertex_groups: the rest pose, a group id per vertex and per normal, the
    // table of XF_RECORD doubles per group and its pinned staging.  On the host per group R_g, the largest |coordinate| among its vertices that a
    // face uses (what mcpt_update_transforms validates against).
    struct Groups {
        RestPose rest; DevBuf<double> table; DevBuf<uint32_t> vgroup, ngroup;
        Staging<double> stage; std::vector<double> radius; Stopwatch watch; uint32_t n_groups = 0, updates = 0;
        mcpt_status alloc(mcpt_ctx* c, uint32_t n) {
            uint64_t* tally = &c->info.device_bytes; const size_t nt = size_t(n) * XF_RECORD;
            HIP_TRY(alloc_all(Want(rest.vtx, c->rf_vtx.count(), tally), Want(rest.nrm, c->rf_nrm.count(), tally), Want(vgroup, c->rf_n_vertex, tally),
                              Want(ngroup, c->rf_n_normal, tally), Want(table, nt, tally), Want(stage, nt), Want(watch, 1, nullptr, !watch.ev0)));
            n_groups = n; radius.assign(n, 0.0);
            return MCPT_OK;
        }
        template <class Copy> mcpt_status clone_from(mcpt_ctx* c, const Groups& src, Copy copy) {       // the groups, the rest pose and R_g
            if (!src.n_groups) return MCPT_OK;
            const mcpt_status st = alloc(c, src.n_groups); if (st != MCPT_OK) return st;
            radius = src.radius;
            HIP_TRY(copy(rest.vtx, src.rest.vtx)); HIP_TRY(copy(rest.nrm, src.rest.nrm)); HIP_TRY(copy(vgroup, src.vgroup)); HIP_TRY(copy(ngroup, src.ngroup));
            return MCPT_OK;
        }
    } xf;
    // Linear-blend skinning (skin.hip), allocated by mcpt_set_vertex_skin: the skin's OWN rest pose (independent of the groups'),
    // SK_INFLUENCES bone ids and weights per vertex and per normal, the table of SK_RECORD doubles per bone and its pinned staging.  On the host
    // per bone R_b, the largest |coordinate| among the vertices that a face uses and that give the bone a weight > 0 (what mcpt_update_skin
    // validates against).  Dual-quaternion mode: the mode is sticky and lives as long as the context; the table of SK_DQ_RECORD
    // doubles per bone (counted in device_bytes) and its pinned staging exist exactly while the mode is MCPT_SKIN_DUAL_QUATERNION AND a skin is set.
    struct Skin {
        RestPose rest; DevBuf<double> table, vweight, nweight, dq_table; DevBuf<uint32_t> vbone, nbone;
        Staging<double> stage, dq_stage; std::vector<double> radius; Stopwatch watch; uint32_t n_bones = 0, updates = 0, mode = MCPT_SKIN_LINEAR;
        bool dq() const { return mode == MCPT_SKIN_DUAL_QUATERNION; }
        Staging<double>& bone_stage() { return dq() ? dq_stage : stage; }         // the pinned stage and the table that the mode in force uses
        DevBuf<double>& bone_table() { return dq() ? dq_table : table; }
        mcpt_status alloc(mcpt_ctx* c, uint32_t n) {
            uint64_t* tally = &c->info.device_bytes;
            const size_t nt = size_t(n) * SK_RECORD, nv = size_t(c->rf_n_vertex) * SK_INFLUENCES, nn = size_t(c->rf_n_normal) * SK_INFLUENCES;
            const size_t nq = size_t(n) * SK_DQ_RECORD;                          // §21: the second table follows n_bones
            HIP_TRY(alloc_all(Want(rest.vtx, c->rf_vtx.count(), tally), Want(rest.nrm, c->rf_nrm.count(), tally), Want(vbone, nv, tally), Want(nbone, nn, tally),
                              Want(vweight, nv, tally), Want(nweight, nn, tally), Want(table, nt, tally), Want(stage, nt), Want(watch, 1, nullptr, !watch.ev0),
                              Want(dq_table, nq, tally, dq()), Want(dq_stage, nq, nullptr, dq())));
            n_bones = n; radius.assign(n, 0.0);
            return MCPT_OK;
        }
        template <class Copy> mcpt_status clone_from(mcpt_ctx* c, const Skin& src, Copy copy) {         // the skin, its rest pose and R_b
            mode = src.mode;                                                     // the skinning mode travels too, with or without a skin (§21)
            if (!src.n_bones) return MCPT_OK;
            const mcpt_status st = alloc(c, src.n_bones); if (st != MCPT_OK) return st;
            radius = src.radius;
            HIP_TRY(copy(rest.vtx, src.rest.vtx)); HIP_TRY(copy(rest.nrm, src.rest.nrm)); HIP_TRY(copy(vbone, src.vbone)); HIP_TRY(copy(nbone, src.nbone));
            HIP_TRY(copy(vweight, src.vweight)); HIP_TRY(copy(nweight, src.nweight)); HIP_TRY(copy(dq_table, src.dq_table));   // (§21: empty in MCPT_SKIN_LINEAR mode)
            return MCPT_OK;
        }
    } sk;
    // Morph targets (morph.hip), allocated by mcpt_set_vertex_morph: the morph's OWN rest pose (independent of the groups' and the
    // skin's), per array of records its n + 1 list offsets and its 32-byte entries, the table of one weight per target and its pinned staging.
    // `tmp` (rf_vtx's and rf_nrm's sizes, counted too) is allocated by the first mcpt_update_morph WITH bones: the morphed arrays that skin.hip's
    // kernels then read as their rest pose (those kernels' `rest` and `out` are __restrict__: they cannot work in place).  On the host R, the
    // largest |coordinate| among the rest-pose vertices that a face uses, and per target D_k, the largest |delta component| among its entries on
    // such vertices (what mcpt_update_morph validates against).
    struct Morph {
        RestPose rest, tmp; DevBuf<double> weight; DevBuf<uint32_t> voffset, noffset; DevBuf<MoEntry> ventry, nentry;
        Staging<double> stage; std::vector<double> delta; double radius = 0.0; Stopwatch watch; uint32_t n_targets = 0, updates = 0;
        mcpt_status alloc(mcpt_ctx* c, uint32_t n, size_t vertex_entries, size_t normal_entries) {
            uint64_t* tally = &c->info.device_bytes;
            HIP_TRY(alloc_all(Want(rest.vtx, c->rf_vtx.count(), tally), Want(rest.nrm, c->rf_nrm.count(), tally),
                              Want(voffset, size_t(c->rf_n_vertex) + 1, tally), Want(noffset, size_t(c->rf_n_normal) + 1, tally),
                              Want(ventry, vertex_entries, tally), Want(nentry, normal_entries, tally), Want(weight, n, tally),
                              Want(stage, n), Want(watch, 1, nullptr, !watch.ev0)));
            n_targets = n; delta.assign(n, 0.0); radius = 0.0;
            return MCPT_OK;
        }
        mcpt_status ensure_scratch(mcpt_ctx* c) {                                // the scratch arrays of "morph, then skin", allocated once
            if (tmp.vtx.p) return MCPT_OK;
            HIP_TRY(alloc_all(Want(tmp.vtx, c->rf_vtx.count(), &c->info.device_bytes), Want(tmp.nrm, c->rf_nrm.count(), &c->info.device_bytes)));
            return MCPT_OK;
        }
        template <class Copy> mcpt_status clone_from(mcpt_ctx* c, const Morph& src, Copy copy) {        // the morph, its rest pose, R and D_k
            if (!src.n_targets) return MCPT_OK;
            const mcpt_status st = alloc(c, src.n_targets, src.ventry.count(), src.nentry.count()); if (st != MCPT_OK) return st;
            delta = src.delta; radius = src.radius;
            HIP_TRY(copy(rest.vtx, src.rest.vtx)); HIP_TRY(copy(rest.nrm, src.rest.nrm)); HIP_TRY(copy(voffset, src.voffset)); HIP_TRY(copy(noffset, src.noffset));
            HIP_TRY(copy(ventry, src.ventry)); HIP_TRY(copy(nentry, src.nentry));
            return src.tmp.vtx.p ? ensure_scratch(c) : MCPT_OK;                   // (scratch: its contents are not carried)
        }
    } mo;
    // Keyframe playback (keyframes.hip), allocated by mcpt_set_vertex_keyframes: the vertex frames and, when the caller gave them,
    // the normal frames -- n_frames arrays of kf_stride() doubles each -- and the pose rf_capture_rest took at set-up, of which `rest.nrm` is what
    // every update writes when there are no normal frames.  Nothing is staged per update: the time becomes kernel arguments.  On the host the
    // options and what the last update played (mcpt_keyframe_info).
    struct Keyframes {
        RestPose rest; DevBuf<double> vframes, nframes; Stopwatch watch;
        uint32_t n_frames = 0, interpolation = 0, wrap = 0, updates = 0, last_frame = 0; double start_time = 0.0, frame_time = 1.0, last_u = 0.0, last_time = 0.0;
        bool normal_frames() const { return nframes.bytes != 0; }
        uint64_t device_bytes() const { return rest.vtx.bytes + rest.nrm.bytes + vframes.bytes + nframes.bytes; }
        mcpt_status alloc(mcpt_ctx* c, uint32_t n, bool normals) {
            uint64_t* tally = &c->info.device_bytes;
            DevBuf<double> none;                                                 // (a set without normal frames replaces one that had them)
            HIP_TRY(alloc_all(Want(rest.vtx, c->rf_vtx.count(), tally), Want(rest.nrm, c->rf_nrm.count(), tally), Want(vframes, n * kf_stride(c->rf_n_vertex), tally),
                              Want(nframes, n * kf_stride(c->rf_n_normal), tally, normals), Want(watch, 1, nullptr, !watch.ev0)));
            if (!normals) nframes = std::move(none);
            n_frames = n;
            return MCPT_OK;
        }
        template <class Copy> mcpt_status clone_from(mcpt_ctx* c, const Keyframes& src, Copy copy) {    // the frames, the rest normals and the options
            if (!src.n_frames) return MCPT_OK;
            const mcpt_status st = alloc(c, src.n_frames, src.normal_frames()); if (st != MCPT_OK) return st;
            interpolation = src.interpolation; wrap = src.wrap; start_time = src.start_time; frame_time = src.frame_time;
            HIP_TRY(copy(rest.vtx, src.rest.vtx)); HIP_TRY(copy(rest.nrm, src.rest.nrm)); HIP_TRY(copy(vframes, src.vframes)); HIP_TRY(copy(nframes, src.nframes));
            return MCPT_OK;
        }
    } kf;
    // Parts update (parts.hip), allocated by mcpt_set_vertex_owners: one owner id per vertex and per normal record, and the scratch
    // pair (rf_vtx's and rf_nrm's sizes) that the routes of mcpt_update_parts write and the select kernel reads.  On the host the records per
    // owner id and what the last parts update ran (mcpt_parts_info).
    struct Parts {
        DevBuf<uint8_t> vowner, nowner; RestPose tmp; Stopwatch watch; PtCounts counts{};
        bool set = false; uint32_t updates = 0, last_routes = 0;
        uint64_t device_bytes() const { return vowner.bytes + nowner.bytes + tmp.vtx.bytes + tmp.nrm.bytes; }
        mcpt_status alloc(mcpt_ctx* c) {
            uint64_t* tally = &c->info.device_bytes;
            HIP_TRY(alloc_all(Want(vowner, c->rf_n_vertex, tally), Want(nowner, c->rf_n_normal, tally), Want(tmp.vtx, c->rf_vtx.count(), tally),
                              Want(tmp.nrm, c->rf_nrm.count(), tally), Want(watch, 1, nullptr, !watch.ev0)));
            set = true;
            return MCPT_OK;
        }
        void drop() { vowner.release(); nowner.release(); tmp.vtx.release(); tmp.nrm.release(); counts = PtCounts{}; set = false; }
        template <class Copy> mcpt_status clone_from(mcpt_ctx* c, const Parts& src, Copy copy) {        // the owners and their counts (scratch: its contents are not carried)
            if (!src.set) return MCPT_OK;
            const mcpt_status st = alloc(c); if (st != MCPT_OK) return st;
            counts = src.counts;
            HIP_TRY(copy(vowner, src.vowner)); HIP_TRY(copy(nowner, src.nowner));
            return MCPT_OK;
        }
    } pt;
    // Automatic normals (normals.hip), allocated by mcpt_set_auto_normals: per normal record its list offset (rf_n_normal + 1) and
    // the 16-byte entries, one per face that names the record.  The lists follow the description's face order, not the leaf order: a rebuild
    // keeps them, a clone carries them.  mode == MCPT_NORMALS_OFF: nothing is allocated, no update runs the pass.
    struct Normals {
        DevBuf<uint32_t> offset; DevBuf<NrEntry> entry; Stopwatch watch; uint32_t mode = 0, updates = 0, records = 0, max_valence = 0;
        mcpt_status alloc(mcpt_ctx* c, size_t entries) {
            uint64_t* tally = &c->info.device_bytes;
            HIP_TRY(alloc_all(Want(offset, size_t(c->rf_n_normal) + 1, tally), Want(entry, entries, tally), Want(watch, 1, nullptr, !watch.ev0)));
            return MCPT_OK;
        }
        template <class Copy> mcpt_status clone_from(mcpt_ctx* c, const Normals& src, Copy copy) {      // the lists
            if (src.mode == MCPT_NORMALS_OFF) return MCPT_OK;
            const mcpt_status st = alloc(c, src.entry.count()); if (st != MCPT_OK) return st;
            mode = src.mode; records = src.records; max_valence = src.max_valence;
            HIP_TRY(copy(offset, src.offset)); HIP_TRY(copy(entry, src.entry));
            return MCPT_OK;
        }
    } nr;
    // Face visibility (visibility.hip), allocated by mcpt_set_face_visibility with a mask: one byte per face of the description on
    // the device (counted in device_bytes) and its pinned staging.  On the host the same bytes (normalised to 0 / 1), what they hide under the
    // current materials, and -- from creation on, dynamic contexts only -- every face's material (`face_material`: the light count of a mask is
    // known before any device work).  `set`: a mask is in force; the hide pass runs when it hides at least one face.  `box_valid`: rf_tri_box holds
    // the boxes of the streams as they are (an update has run since creation or the last rebuild), what mcpt_probe_triangles reads.
    struct Visibility {
        DevBuf<uint8_t> mask; Staging<uint8_t> stage; Stopwatch watch; std::vector<uint8_t> host; std::vector<uint32_t> face_material;
        bool set = false, box_valid = false; uint32_t n_hidden = 0, n_hidden_emitters = 0, updates = 0;
        const uint8_t* dev_mask() const { return set ? mask.p : nullptr; }       // what the light list's kernels take
        void drop() { mask.release(); host.clear(); set = false; n_hidden = 0; n_hidden_emitters = 0; }
        template <class Copy> mcpt_status clone_from(mcpt_ctx* c, const Visibility& src, Copy copy) {   // the mask and what it hides; the source's counter and duration
            face_material = src.face_material; updates = src.updates;
            if (src.watch.ev0) { HIP_TRY(watch.create()); watch.last_ms = src.watch.last_ms; }
            if (!src.set) return MCPT_OK;
            HIP_TRY(alloc_all(Want(mask, src.mask.count(), &c->info.device_bytes), Want(stage, src.mask.count())));
            host = src.host; set = true; n_hidden = src.n_hidden; n_hidden_emitters = src.n_hidden_emitters;
            HIP_TRY(copy(mask, src.mask));
            return MCPT_OK;
        }
    } vs;
    // Camera models (camera.hip).  From creation on, on the host: the model in force as the caller gave it (PINHOLE until
    // mcpt_set_camera_model) and as the ray kernel takes it.  Allocated by the first mcpt_render_camera and counted in device_bytes: the two ray
    // arrays wf_shade_kernel reads as probe_o / probe_d, 3 doubles per pixel each.  `watch` brackets one pass's ray kernel; stage_ms adds them up
    // over a call.
    struct Camera {
        mcpt_camera_model model{}; CmModel dev{}; DevBuf<double> ray_o, ray_d; Stopwatch watch; uint32_t renders = 0; uint64_t passes = 0; double stage_ms = 0.0;
        Camera() { model.struct_size = sizeof model; model.model = MCPT_CAMERA_PINHOLE; dev.model = MCPT_CAMERA_PINHOLE; }
        hipError_t take() {                                                  // the bracketed pass, once it has run, joins the call's sum
            const bool timed = watch.timed;
            const hipError_t e = watch.settle();
            if (e == hipSuccess && timed) stage_ms += watch.last_ms;
            return e;
        }
    } cm;
    // Surface baking (bake.hip), allocated by mcpt_set_bake_points and counted in device_bytes: the points with their leaf-order
    // triangle, a dead byte and a bake-film record {sum L, count} per point; by the first mcpt_bake the two ray arrays wf_shade_kernel reads as
    // probe_o / probe_d, 3 doubles per point each.  On the host the points in FACE terms: mcpt_rebuild_trees permutes the leaf order and derives
    // the device list anew from them.  `watch` brackets one pass's ray kernel; stage_ms adds them up over a call.  A clone starts without points.
    struct Bake {
        std::vector<mcpt_bake_point> host; DevBuf<BkPoint> pts; DevBuf<uint8_t> dead; DevBuf<float4> film; DevBuf<double> ray_o, ray_d;
        Stopwatch watch; uint32_t bakes = 0; uint64_t passes = 0; double stage_ms = 0.0;
        uint32_t direct = MCPT_BAKE_DIRECT_OFF;                              // mcpt_set_bake_direct's mode: no buffer hangs on it, drop() keeps it
        uint32_t n() const { return uint32_t(host.size()); }
        uint64_t device_bytes() const { return pts.bytes + dead.bytes + film.bytes + ray_o.bytes + ray_d.bytes; }
        void drop() { host.clear(); pts.release(); dead.release(); film.release(); ray_o.release(); ray_d.release(); }
        hipError_t take() {                                                  // the bracketed pass, once it has run, joins the call's sum
            const bool timed = watch.timed;
            const hipError_t e = watch.settle();
            if (e == hipSuccess && timed) stage_ms += watch.last_ms;
            return e;
        }
        // the device list for a leaf order: point i names leaf_of_face[its face]
        std::vector<BkPoint> in_leaf_terms(const std::vector<int32_t>& leaf_of_face) const {
            std::vector<BkPoint> v(host.size());
            for (size_t i = 0; i < host.size(); i++) v[i] = BkPoint{leaf_of_face[size_t(host[i].face)], host[i].u, host[i].v, host[i].flags};
            return v;
        }
    } bk;
    // Light probes (shprobe.hip), allocated by mcpt_set_sh_probes and counted in device_bytes: per probe its position in device
    // coordinates, 27 fp32 accumulators and the counts {rays, hits from behind, misses}; by the first mcpt_bake_sh, per ITEM (64 per probe) the two
    // ray arrays wf_shade_kernel reads as probe_o / probe_d, the scratch film of one pass and the class byte.  On the host the WORLD positions:
    // mcpt_rebuild_trees derives the device coordinates anew from them.  `watch` brackets one pass's ray and first-hit kernels; stage_ms adds them
    // up over a call.  `have_pass`: a pass of the set list has been enqueued (mcpt_read_sh_pass).  A clone starts without probes.
    struct ShProbes {
        std::vector<double> host; DevBuf<double> pos; DevBuf<float> acc; DevBuf<uint32_t> counts; DevBuf<double> ray_o, ray_d; DevBuf<float4> film; DevBuf<uint8_t> cls;
        Stopwatch watch; uint32_t bakes = 0; uint64_t passes = 0; double stage_ms = 0.0; bool have_pass = false;
        uint32_t n() const { return uint32_t(host.size() / 3); }
        uint32_t items() const { return n() * SH_DIRS; }
        uint64_t device_bytes() const { return pos.bytes + acc.bytes + counts.bytes + ray_o.bytes + ray_d.bytes + film.bytes + cls.bytes; }
        void drop_pass() { ray_o.release(); ray_d.release(); film.release(); cls.release(); have_pass = false; }
        void drop() { host.clear(); pos.release(); acc.release(); counts.release(); drop_pass(); }
        hipError_t take() {                                                  // the bracketed pass, once it has run, joins the call's sum
            const bool timed = watch.timed;
            const hipError_t e = watch.settle();
            if (e == hipSuccess && timed) stage_ms += watch.last_ms;
            return e;
        }
    } sh;
    // Temporal reprojection (reproject.hip), allocated by the first reprojection call: the old view's features (2 per pixel, swapped
    // with dn_feat per call), a copy of the old film and the reuse counter.
    // Motion-vector reprojection adds, on the first mcpt_update_vertices_reproject: the first hit of every pixel-centre ray and
    // the vertices and normals as they were before the update (rf_vtx's and rf_nrm's sizes).  All but the counter are counted in device_bytes.
    DevBuf<float4> rp_feat_old, rp_film_old, rp_hits; DevBuf<unsigned long long> rp_count; DevBuf<double> rp_vtx_old, rp_nrm_old;
    Stopwatch rp_watch;
    uint32_t rp_calls = 0;
    // Material edits (materials.hip).  From creation on, on the host: the description's materials as they are now, per texture its
    // place in `texels`, size and first texel, per material the faces that use it (the new light count is known before any device work).
    // Allocated by the first mcpt_update_materials and counted in device_bytes: one word per face (light flag, then its prefix sum) and one per
    // scan block.  `lights` / `light_pos64` only grow: their capacity is their buffers' count().
    std::vector<mcpt_material> mt_mats; std::vector<TexInfo> mt_tex; std::vector<uint32_t> mt_faces;
    DevBuf<uint32_t> mt_flag, mt_sums;
    Staging<DevMaterial> mt_stage; Staging<float4> mt_tex_stage;
    Stopwatch mt_watch; bool mt_have_watch = false;
    uint32_t mt_updates = 0;
};

static mcpt_status read_back(mcpt_ctx* ctx, void* host, const void* dev, size_t bytes, bool timing = true);
static mcpt_status resolve_timing(mcpt_ctx* c, bool block = true);

namespace {

template <class T, class H> hipError_t upload(DevBuf<T>& b, const std::vector<H>& v, uint64_t* tally) {
    static_assert(sizeof(H) == sizeof(T), "the host mirror of a device element has its size (f4h / float4)");
    const hipError_t e = b.alloc(v.size(), tally);
    return e != hipSuccess || v.empty() ? e : hipMemcpy(b.p, v.data(), b.bytes, hipMemcpyHostToDevice);
}

// The device must be current while the members give their handles back.
void destroy_ctx(mcpt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

mcpt_status use(mcpt_ctx* c) {
    if (!c) return fail(MCPT_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return MCPT_OK;
}

// Live scenes need what MCPT_FLAG_DYNAMIC keeps; `who` opens the message ("<entry point>: ").
mcpt_status require_dynamic(const mcpt_ctx* c, const std::string& who) { return c->dynamic ? MCPT_OK : fail(MCPT_ERR_UNSUPPORTED, who + "the context was created without MCPT_FLAG_DYNAMIC"); }

mcpt_status check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MCPT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(MCPT_ERR_NO_DEVICE, "device ordinal out of range");
    return MCPT_OK;
}

// The optional options struct of an entry point: absent = all defaults, present = exactly this library's layout.
template <class O> mcpt_status read_opts(const O* opts, O& o, const char* fn, const char* type) {
    std::memset(&o, 0, sizeof o); o.struct_size = sizeof o;
    if (opts && opts->struct_size != sizeof(O)) return fail(MCPT_ERR_INVALID_ARG, std::string(fn) + ": opts->struct_size != sizeof(" + type + ")");
    if (opts) o = *opts;
    return MCPT_OK;
}

uint64_t film_tiles(const mcpt_ctx* c) { return uint64_t((c->width + 7) / 8) * uint64_t((c->height + 7) / 8); }   // 8 x 8 pixel tiles

// leaf order -> face index on the host, fetched on first use (probes only)
mcpt_status fetch_tri_face(mcpt_ctx* c) {
    if (!c->h_tri_face.empty()) return MCPT_OK;
    std::vector<int32_t> f(size_t(c->dev.n_tris));
    const mcpt_status st = read_back(c, f.data(), c->dev.tri_face, f.size() * sizeof(int32_t), false);
    if (st == MCPT_OK) c->h_tri_face.swap(f);
    return st;
}

// What a control-block snapshot taken after iteration `it` says about a job with n_shared shared work items.
enum class JobState { Watchdog, Finished, NotFinished };
const char* const WATCHDOG_MSG = "trace kernel watchdog: a wave did not finish its ray list (internal error)";
JobState job_state(const IterCtl& s, uint32_t it, uint32_t n_shared) {
    if (s.pad[WF_CTL_WATCHDOG]) return JobState::Watchdog;
    for (uint32_t q = 0; q < WF_ITEM_SHARDS; q++) if (s.item_cursor[q].v < wf_shard_capacity(n_shared, q)) return JobState::NotFinished;
    return s.any_active[it & 3] != 0 ? JobState::NotFinished : JobState::Finished;
}

// Has `ev` happened?  `block`: wait for it.
hipError_t event_done(hipEvent_t ev, bool block, bool& done) {
    const hipError_t e = block ? hipEventSynchronize(ev) : hipEventQuery(ev);
    done = e == hipSuccess;
    return e == hipErrorNotReady ? hipSuccess : e;
}

uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* v = std::getenv(name);
    return (v && *v) ? uint32_t(std::strtoul(v, nullptr, 10)) : dflt;
}

// Probe entry points take and return WORLD coordinates; the device works relative to DevScene::centre.
std::vector<double> to_local(const mcpt_ctx* c, const double* p, size_t n) {
    std::vector<double> v(3 * n);
    for (size_t i = 0; i < n; i++) for (int a = 0; a < 3; a++) v[3 * i + a] = p[3 * i + a] - c->dev.centre[a];
    return v;
}

// Device scratch and host temporaries of one probe call.  The rule of this file: once a context has been handed out, every copy and fill is an
// ...Async call on a named stream (ctx->stream, or a sub-pipeline's L.stream for its pool) and is ordered with the kernels around it by that stream alone.
// Host memory an enqueued copy touches must outlive it: the destructor synchronises the stream before anything here is freed, on every return path.
struct Scratch {
    hipStream_t stream;
    std::vector<void*> ptrs;
    std::vector<std::shared_ptr<void>> held;
    explicit Scratch(hipStream_t s) : stream(s) {}
    Scratch(const Scratch&) = delete;
    ~Scratch() { (void)finish(); for (void* p : ptrs) (void)hipFree(p); }
    template <class T> T* keep(std::vector<T> v) {       // a host temporary that lives as long as the copies that use it
        auto h = std::make_shared<std::vector<T>>(std::move(v));
        held.push_back(h);
        return h->data();
    }
    template <class T> hipError_t alloc(size_t n, T** dev) {
        const hipError_t e = hipMalloc((void**)dev, (n ? n : 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*dev);
        return e;
    }
    // n counts elements of the host type
    template <class T> hipError_t put(void* dev, const T* host, size_t n) { return n ? hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, stream) : hipSuccess; }
    template <class T> hipError_t fetch(T* host, const void* dev, size_t n) { return n ? hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, stream) : hipSuccess; }
    hipError_t fill(void* dev, int byte, size_t bytes) { return hipMemsetAsync(dev, byte, bytes, stream); }
    template <class T> hipError_t in(const T* host, size_t n, T** dev) { const hipError_t e = alloc(n, dev); return e != hipSuccess ? e : put(*dev, host, n); }
    template <class T> hipError_t out(size_t n, T** dev) { const hipError_t e = alloc(n, dev); return e != hipSuccess ? e : fill(*dev, 0, (n ? n : 1) * sizeof(T)); }
    hipError_t finish() { return hipStreamSynchronize(stream); }
};

}  // namespace

// The traversal-stack overflow area one sub-pipeline needs under a wide tree of depth `wide_depth`, from the context's trace grid; host arithmetic
// only.  mcpt_create and mcpt_rebuild_trees size (and refuse) by it.
static mcpt_status overflow_bytes(const mcpt_ctx* c, uint32_t wide_depth, size_t& out) {
    out = size_t(c->trace_grid) * wf_trace_block_threads() * wf_trace_overflow_bytes_per_lane(wide_depth);
    if (out > (size_t(512) << 20)) return fail(MCPT_ERR_BVH_DEPTH, "wide BVH of depth " + std::to_string(wide_depth) + " needs a traversal-stack overflow area of " + std::to_string(out >> 20) + " MB per sub-pipeline: build the tree with the host builder (no MCPT_FLAG_GPU_BVH_BUILD)");
    return MCPT_OK;
}

// Everything of a context that is not the scene: streams, events, film, counters, the wavefront sub-pipelines, and the device pointers of
// c->dev (the scene streams c->nodes ... c->texels are on the device already: uploaded by mcpt_create or copied by mcpt_clone_to_device).
static mcpt_status finish_ctx(mcpt_ctx* c) {
    HIP_TRY(hipStreamCreateWithFlags(c->own_stream.out(), hipStreamNonBlocking));
    c->stream = c->own_stream;
    for (uint32_t i = 0; i < mcpt_ctx::TIMED; i++) { HIP_TRY(hipEventCreate(c->ev0[i].out())); HIP_TRY(hipEventCreate(c->ev1[i].out())); }
    HIP_TRY(c->accum_own.alloc(size_t(c->width) * c->height, &c->info.device_bytes));
    HIP_TRY(hipMemset(c->accum_own.p, 0, c->accum_own.bytes));
    HIP_TRY(c->counters.alloc(WF_COUNTER_REPLICAS));
    HIP_TRY(hipMemset(c->counters.p, 0, c->counters.bytes));
    {   // ---- wavefront pool.  Tunables are developer knobs (environment), not part of the ABI; every one of them is decided ONCE, here: no
        // render call reads the environment.
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, c->device));
        c->n_cus = prop.multiProcessorCount;
        c->knobs = wf_read_knobs(env_u32);
        c->tune.refill_at = env_u32("MCPT_WF_REFILL", 28); c->tune.leaf_at = env_u32("MCPT_WF_LEAF", 16);
        c->tune.inner_keep = env_u32("MCPT_WF_INNER", 24); c->tune.policy = env_u32("MCPT_WF_POLICY", 0); c->tune.pend_cap = 48;      // speculative traversal: refined below once the scene's size is known
        if (c->use_wavefront) {
            uint32_t n_lanes = env_u32("MCPT_WF_LANES", 2);
            if (n_lanes < 1) n_lanes = 1;
            if (c->opts.flags & MCPT_FLAG_DETERMINISTIC) n_lanes = 1;          // one owner per pixel, plain stores
            // Persistent trace grid: one 1024-thread block (16 waves, 78 VGPRs) per CU -- what the register file admits beside two shade
            // waves per SIMD (4 x 80 + 2 x 96 = 512).  Rounds 1-2 launched 3/4 and 7/8 of the CUs while the traversal data was
            // cache-resident (their 72-register kernel left room for a second block on some CUs); r03, 8-wide kernel, S-cornell 512 spp:
            // 214.6 / 217.5 / 211.6 / 213.4 / 208.5 ms at 192 / 208 / 224 / 240 / 256 blocks.  MCPT_WF_GRID overrides.
            const uint32_t per_cu = uint32_t(wf_trace_blocks_per_cu((c->opts.flags & MCPT_FLAG_COUNT_TRAVERSAL) != 0));
            c->trace_grid = uint32_t(c->n_cus) * per_cu;
            c->trace_grid = std::min(env_u32("MCPT_WF_GRID", c->trace_grid), uint32_t(c->n_cus) * per_cu);
            // speculative traversal: S-cornell 469 -> 450 ms; on the 4 M-triangle configuration, where the extra node visits are HBM
            // traffic, it is neutral within the noise (same box: 367 ms with, 371 ms without) -- on everywhere; MCPT_WF_PEND=0 turns it off
            c->tune.pend_cap = env_u32("MCPT_WF_PEND", 48u);
            HIP_TRY(hipEventCreateWithFlags(c->fork_ev.out(), hipEventDisableTiming));
            c->lanes.resize(n_lanes);
            for (auto& L : c->lanes) {
                L.pool.P = 0;                                             // allocated by ensure_pool() when the first job arrives
                HIP_TRY(L.ctl_buf.alloc(1));
                HIP_TRY(hipHostMalloc(L.h_ctl.out(), 8 * sizeof(IterCtl), hipHostMallocDefault));
                L.chk_ev.resize(8);
                for (auto& ev : L.chk_ev) HIP_TRY(hipEventCreateWithFlags(ev.out(), hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(L.done_ev.out(), hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(L.shade_ev.out(), hipEventDisableTiming));
                HIP_TRY(hipStreamCreateWithFlags(L.stream.out(), hipStreamNonBlocking));
                // the global overflow area of the traversal stack is sized from the wide tree's depth (2 x depth + 3 entries of 8 B per trace lane): a
                // pathologically deep device-built tree (depth in the hundreds) would ask for a GB per sub-pipeline -- refuse instead of allocating it
                size_t ovf_bytes = 0;
                const mcpt_status os = overflow_bytes(c, c->wide_depth, ovf_bytes); if (os != MCPT_OK) return os;
                HIP_TRY(L.ovf_buf.alloc(ovf_bytes / sizeof(int)));
            }
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    c->accum = c->accum_own.p;
    DevScene& d = c->dev;
    d.nodes = c->nodes.p; d.nodes8 = c->nodes8.p; d.tri_isect = c->tri_isect.p; d.tri_shade = c->tri_shade.p; d.tri_pos64 = c->tri_pos64.p;
    d.tri_face = c->tri_face.p; d.mats = c->mats.p; d.lights = c->lights.p; d.light_pos64 = c->light_pos64.p; d.texels = c->texels.p;
    return MCPT_OK;
}

// The wide tree's part of the info: hs.nodes8 and its depth, the leaf order `tri_face` (n_tris entries), the tri_isect stream's 3 n_tris + 3 records.
static void fill_tree_info(mcpt_scene_info& in, const HostScene& hs, const int32_t* tri_face, size_t n_tris) {
    in.wide_width = 8; in.wide_nodes = uint32_t(hs.nodes8.size() / 5);
    in.wide_depth = hs.bvh8_depth;
    in.traversal_bytes = (hs.nodes8.size() + 3 * n_tris + 3) * sizeof(f4h);
    uint64_t h = 1469598103934665603ull;                                  // FNV-1a, 4 bytes at a time
    auto mix = [&](const void* p, size_t bytes) { const uint32_t* w = static_cast<const uint32_t*>(p); for (size_t i = 0; i < bytes / 4; i++) { h ^= w[i]; h *= 1099511628211ull; } };
    mix(hs.nodes8.data(), hs.nodes8.size() * sizeof(f4h)); mix(tri_face, n_tris * 4);
    in.wide_tree_hash = h;
}
static void fill_wide_info(mcpt_scene_info& in, const HostScene& hs) {
    fill_tree_info(in, hs, hs.tri_face.data(), hs.tri_face.size());
    for (int a = 0; a < 3; a++) in.centre[a] = hs.centre[a];
}

// The device builders mcpt_create and mcpt_rebuild_trees hand to build_trees: PLOC on the current device (gave up: no tree, no error -- the host
// builder takes over, bvh_builder = 2) and the device collapse (MCPT_HOST_COLLAPSE=1: the host's).
static BvhBuildFn device_bvh_builder() {
    return [](const float* boxes, uint32_t n, std::vector<f4h>& nodes, std::vector<int>& order, uint32_t& depth, uint32_t& max_leaf, std::string& berr) {
        GpuBvh g;
        if (!gpu_build_ploc(boxes, n, g, berr)) {
            if (!g.gave_up) return false;
            if (std::getenv("MCPT_BUILD_DEBUG")) fprintf(stderr, "[build] %s: building on the host\n", berr.c_str());
            nodes.clear(); order.clear(); berr.clear();              // gave up: no tree, no error -- the host builder takes over (bvh_builder = 2)
            return true;
        }
        nodes.swap(g.nodes); order.assign(g.order.begin(), g.order.end()); depth = g.depth; max_leaf = g.max_leaf;
        return true;
    };
}
static Collapse8Fn device_collapse8() { return env_u32("MCPT_HOST_COLLAPSE", 0) ? Collapse8Fn(nullptr) : Collapse8Fn(gpu_collapse_bvh8); }


// ------------------------------------------------------------------------------------------------ live scenes: set-up
// The per-block partial sums the last launch_rf_wide_area left in rf_area, added up.  Synchronises.
static mcpt_status rf_read_area(mcpt_ctx* c, double& out) {
    std::vector<double> part(rf_area_blocks(uint32_t(c->dev.n_nodes8)));
    const mcpt_status st = read_back(c, part.data(), c->rf_area.p, part.size() * sizeof(double), false); if (st != MCPT_OK) return st;
    out = 0.0;
    for (double v : part) out += v;
    return MCPT_OK;
}
// Sum of the dequantised child-box areas of the context's 8-wide tree, as it is on the device when the stream reaches this point.  Synchronises.
static mcpt_status rf_wide_area(mcpt_ctx* c, double& out) {
    HIP_TRY(launch_rf_wide_area(c->dev.nodes8, uint32_t(c->dev.n_nodes8), c->rf_area.p, c->stream));
    return rf_read_area(c, out);
}
static mcpt_status rf_alloc(mcpt_ctx* c) {
    const size_t nt = size_t(c->dev.n_tris), n8 = size_t(c->dev.n_nodes8), n2 = size_t(c->dev.n_nodes);
    uint64_t* tally = &c->info.device_bytes;
    HIP_TRY(c->rf_idx.alloc(nt * 6, tally)); HIP_TRY(c->rf_vtx.alloc(size_t(c->rf_n_vertex) * 3, tally));
    HIP_TRY(c->rf_nrm.alloc(size_t(c->rf_n_normal) * 3, tally)); HIP_TRY(c->rf_tri_box.alloc(nt * 6, tally));
    HIP_TRY(c->rf_node_box.alloc(n8 * 6, tally)); HIP_TRY(c->rf_bin_order.alloc(n2, tally));
    HIP_TRY(c->rf_area.alloc(rf_area_blocks(uint32_t(n8)), tally));
    HIP_TRY(c->rf_stage.grow(c->rf_vtx.count() + c->rf_nrm.count() + 2));         // (+ 2: never empty)
    HIP_TRY(c->rf_watch.create());
    c->dynamic = true;
    return MCPT_OK;
}
static mcpt_status rf_setup(mcpt_ctx* c, const HostScene& hs, const mcpt_scene_desc* scene) {
    std::vector<uint32_t> bin_order; std::string err;
    if (!rf_levels(hs.nodes, hs.nodes8, bin_order, c->rf_bin_level, c->rf_wide_level, err)) return fail(MCPT_ERR_UNSUPPORTED, "MCPT_FLAG_DYNAMIC: " + err);
    c->rf_n_vertex = scene->n_vertex; c->rf_n_normal = scene->n_normal;
    c->rf_used_vertex.assign(scene->n_vertex, 0);
    for (size_t i = 0; i < hs.dyn_idx.size(); i += 6) for (int k = 0; k < 3; k++) c->rf_used_vertex[size_t(hs.dyn_idx[i + k])] = 1;
    mcpt_status st = rf_alloc(c); if (st != MCPT_OK) return st;
    Scratch s(c->stream);                                                 // the uploads and the kernel that follows are ordered by the context's stream
    HIP_TRY(s.put(c->rf_idx.p, hs.dyn_idx.data(), c->rf_idx.count())); HIP_TRY(s.put(c->rf_bin_order.p, bin_order.data(), c->rf_bin_order.count()));
    HIP_TRY(s.put(c->rf_vtx.p, scene->vertex, c->rf_vtx.count())); HIP_TRY(s.put(c->rf_nrm.p, scene->normal, c->rf_nrm.count()));
    return rf_wide_area(c, c->rf_area0);                                  // (synchronises: the caller's arrays have been read)
}
static mcpt_status rf_clone(mcpt_ctx* c, mcpt_ctx* src) {
    c->rf_n_vertex = src->rf_n_vertex; c->rf_n_normal = src->rf_n_normal; c->rf_used_vertex = src->rf_used_vertex;
    c->rf_bin_level = src->rf_bin_level; c->rf_wide_level = src->rf_wide_level; c->rf_area0 = src->rf_area0;
    mcpt_status st = rf_alloc(c); if (st != MCPT_OK) return st;
    auto copy = [&](auto& dst, const auto& from) { return from.bytes ? hipMemcpyPeer(dst.p, c->device, from.p, src->device, from.bytes) : hipSuccess; };
    HIP_TRY(copy(c->rf_idx, src->rf_idx)); HIP_TRY(copy(c->rf_bin_order, src->rf_bin_order)); HIP_TRY(copy(c->rf_vtx, src->rf_vtx)); HIP_TRY(copy(c->rf_nrm, src->rf_nrm));
    if ((st = c->xf.clone_from(c, src->xf, copy)) != MCPT_OK || (st = c->sk.clone_from(c, src->sk, copy)) != MCPT_OK ||
        (st = c->mo.clone_from(c, src->mo, copy)) != MCPT_OK || (st = c->kf.clone_from(c, src->kf, copy)) != MCPT_OK ||
        (st = c->pt.clone_from(c, src->pt, copy)) != MCPT_OK || (st = c->nr.clone_from(c, src->nr, copy)) != MCPT_OK) return st;
    HIP_TRY(hipSetDevice(src->device)); HIP_TRY(src->vs.watch.settle()); HIP_TRY(hipSetDevice(c->device));   // (the source's stream is drained: its last duration is there to read)
    if ((st = c->vs.clone_from(c, src->vs, copy)) != MCPT_OK) return st;             // §24: the scene streams were copied as they are, hidden records included
    HIP_TRY(hipDeviceSynchronize());
    return MCPT_OK;
}
// The first-hit features and the last adaptive call's tile error describe the scene as it was.
static void rf_forget_derived(mcpt_ctx* c) { c->dn_have_features = false; c->dn_have_emis = false; c->dn_have_out = false; c->ad_have_err = false; }

// What mcpt_set_vertex_groups / _skin / _morph do once their arguments are checked, in this order: the stream drained (rf_vtx / rf_nrm are final,
// and no copy out of the old stage is under way), the record's `alloc`, rf_vtx / rf_nrm copied into `rest` on the device, the caller's per-record
// arrays `put` through the same Scratch, the vertices fetched: `used(v, far)` sees each one that a face uses and its largest |coordinate|.
template <class Alloc, class Put, class Used> static mcpt_status rf_capture_rest(mcpt_ctx* ctx, mcpt_ctx::RestPose& rest, Alloc alloc, Put put, Used used) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    mcpt_status st = resolve_timing(ctx); if (st != MCPT_OK) return st;
    st = alloc(); if (st != MCPT_OK) return st;
    std::vector<double> vtx(ctx->rf_vtx.count());
    {   Scratch s(ctx->stream);
        if (ctx->rf_vtx.bytes) HIP_TRY(hipMemcpyAsync(rest.vtx.p, ctx->rf_vtx.p, ctx->rf_vtx.bytes, hipMemcpyDeviceToDevice, ctx->stream));
        if (ctx->rf_nrm.bytes) HIP_TRY(hipMemcpyAsync(rest.nrm.p, ctx->rf_nrm.p, ctx->rf_nrm.bytes, hipMemcpyDeviceToDevice, ctx->stream));
        st = put(s); if (st != MCPT_OK) return st;
        HIP_TRY(s.fetch(vtx.data(), ctx->rf_vtx.p, vtx.size())); HIP_TRY(s.finish()); }
    for (uint32_t v = 0; v < ctx->rf_n_vertex; v++) {
        const double* x = vtx.data() + 3 * size_t(v);
        if (ctx->rf_used_vertex[v]) used(v, std::max({std::fabs(x[0]), std::fabs(x[1]), std::fabs(x[2])}));
    }
    return MCPT_OK;
}
// The shared opening of the info getters; `watch` is the context's (null with a null context, which is refused before it is looked at).
template <class Info> static mcpt_status info_begin(mcpt_ctx* ctx, Info* out, Stopwatch* watch) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    st = resolve_timing(ctx); if (st != MCPT_OK) return st;
    HIP_TRY(watch->settle());
    std::memset(out, 0, sizeof *out); out->struct_size = sizeof *out;
    return MCPT_OK;
}

extern "C" {

uint32_t mcpt_abi_version(void) { return MCPT_ABI_VERSION; }
const char* mcpt_last_error(void) { return g_err.c_str(); }

mcpt_status mcpt_check_scene(const mcpt_scene_desc* scene, mcpt_scene_info* out_info) {
    if (!scene) return fail(MCPT_ERR_INVALID_ARG, "mcpt_check_scene: null argument");
    HostScene hs; std::string err;
    mcpt_status st = build_host_scene(scene, hs, err);
    if (st != MCPT_OK) return fail(st, err);
    const std::string bad = validate_wide_bvh(hs);
    if (!bad.empty()) return fail(MCPT_ERR_UNSUPPORTED, "internal: wide BVH failed its self-check: " + bad);
    if (out_info) {
        std::memset(out_info, 0, sizeof *out_info);
        out_info->n_tris = uint32_t(hs.tri_face.size()); out_info->n_lights = uint32_t(hs.lights.size()); out_info->n_nodes = uint32_t(hs.nodes.size() / 4);
        out_info->bvh_depth = hs.bvh_depth; out_info->max_leaf = hs.max_leaf; out_info->width = uint32_t(scene->camera.width); out_info->height = uint32_t(scene->camera.height);
        out_info->bvh_build_ms = hs.bvh_build_ms;
        fill_wide_info(*out_info, hs);
    }
    return MCPT_OK;
}

mcpt_status mcpt_create(const mcpt_scene_desc* scene, const mcpt_opts* opts, mcpt_ctx** out_ctx) {
    if (!scene || !out_ctx) return fail(MCPT_ERR_INVALID_ARG, "mcpt_create: null argument");
    *out_ctx = nullptr;
    mcpt_opts o; std::memset(&o, 0, sizeof o);
    if (opts) std::memcpy(&o, opts, std::min<size_t>(sizeof o, opts->struct_size ? opts->struct_size : sizeof o));
    if (o.integrator > MCPT_INTEGRATOR_RECURSIVE_NEE) return fail(MCPT_ERR_INVALID_ARG, "unknown integrator");

    HostScene hs; std::string err;
    hs.reference_tie_order = (o.flags & MCPT_FLAG_REFERENCE_TIE_ORDER) != 0;
    hs.keep_dynamic = (o.flags & MCPT_FLAG_DYNAMIC) != 0;
    // which pipeline this context runs is decided ONCE, here: it sets how deep a device-built binary tree may be (below) and which kernels
    // mcpt_render launches -- the two must agree, or a megakernel context could walk a tree deeper than its LDS stack
    const bool use_wavefront = [&]() { const char* pipe = std::getenv("MCPT_PIPELINE"); return !(pipe && std::string(pipe) == "mega") && o.integrator == MCPT_INTEGRATOR_MIS; }();
    if ((o.flags & MCPT_FLAG_REFERENCE_TIE_ORDER) && !use_wavefront)
        return fail(MCPT_ERR_UNSUPPORTED, "MCPT_FLAG_REFERENCE_TIE_ORDER needs the wavefront pipeline (MCPT_INTEGRATOR_MIS, no MCPT_PIPELINE=mega): the binary-tree kernels have no tie rule");
    mcpt_status st;
    if (o.flags & MCPT_FLAG_GPU_BVH_BUILD) {                              // the tree is built on the device the context will render on
        if ((st = check_device(o.device)) != MCPT_OK) return st;
        HIP_TRY(hipSetDevice(o.device));
        // An agglomerative (PLOC) tree over millions of triangles can be deeper than the binary-tree kernels' 64-entry stack.  Only the
        // cross-check kernels (megakernel, recursive integrator, mcpt_probe_trace) walk the binary tree; the wavefront pipeline walks
        // the wide collapse of it, whose stack is sized from its own depth -- so a wavefront-only context keeps the deep tree.
        hs.allow_deep_binary = use_wavefront;
        st = build_host_scene(scene, hs, err, device_bvh_builder(), device_collapse8());
        if (st != MCPT_OK) return fail(st, err);
        if (env_u32("MCPT_VALIDATE_BVH", 0)) { const std::string bad = validate_wide_bvh(hs); if (!bad.empty()) return fail(MCPT_ERR_HIP, "device-built BVH failed validation: " + bad); }
    } else {
        st = build_host_scene(scene, hs, err);
        if (st != MCPT_OK) return fail(st, err);
        if ((st = check_device(o.device)) != MCPT_OK) return st;
    }

    // the 8-wide trace kernel addresses node and triangle records with 32-bit byte offsets
    if ((hs.nodes8.size() * sizeof(f4h) >= (1ull << 32) || hs.tri_isect.size() * sizeof(f4h) >= (1ull << 32)))
        return fail(MCPT_ERR_UNSUPPORTED, "scene too large for the 8-wide traversal kernel (more than 89 M triangles)");
    std::unique_ptr<mcpt_ctx, void (*)(mcpt_ctx*)> guard(new mcpt_ctx(), destroy_ctx);   // a context that is not handed out is destroyed
    mcpt_ctx* c = guard.get();
    c->device = o.device; c->opts = o; c->width = scene->camera.width; c->height = scene->camera.height;
    c->wide_depth = hs.bvh8_depth; c->binary_ok = hs.binary_ok; c->use_wavefront = use_wavefront;
    HIP_TRY(hipSetDevice(c->device));
    auto t0 = std::chrono::steady_clock::now();
    uint64_t* tally = &c->info.device_bytes;
    HIP_TRY(upload(c->nodes, hs.nodes, tally)); HIP_TRY(upload(c->nodes8, hs.nodes8, tally)); HIP_TRY(upload(c->tri_isect, hs.tri_isect, tally));
    HIP_TRY(upload(c->tri_shade, hs.tri_shade, tally)); HIP_TRY(upload(c->tri_pos64, hs.tri_pos64, tally)); HIP_TRY(upload(c->tri_face, hs.tri_face, tally));
    HIP_TRY(upload(c->mats, hs.mats, tally)); HIP_TRY(upload(c->lights, hs.lights, tally)); HIP_TRY(upload(c->light_pos64, hs.light_pos64, tally));
    HIP_TRY(upload(c->texels, hs.texels, tally));
    DevScene& d = c->dev;
    d.n_nodes8 = int32_t(hs.nodes8.size() / 5);
    d.cam = hs.cam;
    for (int a = 0; a < 3; a++) d.centre[a] = hs.centre[a];
    d.n_tris = int32_t(hs.tri_face.size()); d.n_lights = int32_t(hs.lights.size()); d.n_nodes = int32_t(hs.nodes.size() / 4); d.n_mats = int32_t(hs.mats.size());
    mcpt_scene_info& in = c->info;
    in.n_tris = uint32_t(d.n_tris); in.n_lights = uint32_t(d.n_lights); in.n_nodes = uint32_t(d.n_nodes);
    in.bvh_depth = hs.bvh_depth; in.max_leaf = hs.max_leaf; in.width = uint32_t(c->width); in.height = uint32_t(c->height);
    in.bvh_build_ms = hs.bvh_build_ms; in.bvh_builder = hs.bvh_builder;
    fill_wide_info(in, hs);
    c->mt_mats.assign(scene->materials, scene->materials + scene->n_materials); c->mt_tex = hs.tex_info; c->mt_faces = hs.mat_faces;
    if ((st = finish_ctx(c)) != MCPT_OK) return st;
    if ((o.flags & MCPT_FLAG_DYNAMIC) && (st = rf_setup(c, hs, scene)) != MCPT_OK) return st;
    if (o.flags & MCPT_FLAG_DYNAMIC) {                                    // §24: the material of a face is corner 0's (build_host_scene checked its range)
        c->vs.face_material.resize(scene->n_face);
        for (uint32_t f = 0; f < scene->n_face; f++) c->vs.face_material[f] = uint32_t(scene->face[12 * size_t(f) + 3]);
    }
    in.upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out_ctx = guard.release();
    return MCPT_OK;
}

/* A second context for the SAME scene on another device (or the same one): every scene stream is copied device to device -- no flatten, no
 * BVH build, no host copy of the scene is kept around for it.  `mcpt_cli --gpus N` builds once and clones N - 1 times. */
mcpt_status mcpt_clone_to_device(mcpt_ctx* src, int32_t device, mcpt_ctx** out_ctx) {
    if (!src || !out_ctx) return fail(MCPT_ERR_INVALID_ARG, "mcpt_clone_to_device: null argument");
    *out_ctx = nullptr;
    mcpt_status st = check_device(device); if (st != MCPT_OK) return st;
    st = use(src); if (st != MCPT_OK) return st;
    HIP_TRY(hipStreamSynchronize(src->stream));
    std::unique_ptr<mcpt_ctx, void (*)(mcpt_ctx*)> guard(new mcpt_ctx(), destroy_ctx);
    mcpt_ctx* c = guard.get();
    c->device = device; c->opts = src->opts; c->opts.device = device; c->width = src->width; c->height = src->height;
    c->wide_depth = src->wide_depth; c->binary_ok = src->binary_ok; c->use_wavefront = src->use_wavefront;
    c->dev = src->dev; c->info = src->info; c->info.bvh_build_ms = 0.0; c->info.device_bytes = 0;   // (counts this context's own allocations)
    HIP_TRY(hipSetDevice(device));
    auto t0 = std::chrono::steady_clock::now();
    auto copy = [&](auto mcpt_ctx::* m) {                                  // one scene stream: the types of the two ends agree by construction
        const hipError_t e = (c->*m).alloc((src->*m).count(), &c->info.device_bytes);
        return e != hipSuccess || !(src->*m).bytes ? e : hipMemcpyPeer((c->*m).p, device, (src->*m).p, src->device, (src->*m).bytes);
    };
    HIP_TRY(copy(&mcpt_ctx::nodes)); HIP_TRY(copy(&mcpt_ctx::nodes8)); HIP_TRY(copy(&mcpt_ctx::tri_isect)); HIP_TRY(copy(&mcpt_ctx::tri_shade));
    HIP_TRY(copy(&mcpt_ctx::tri_pos64)); HIP_TRY(copy(&mcpt_ctx::tri_face)); HIP_TRY(copy(&mcpt_ctx::mats)); HIP_TRY(copy(&mcpt_ctx::lights));
    HIP_TRY(copy(&mcpt_ctx::light_pos64)); HIP_TRY(copy(&mcpt_ctx::texels));
    c->mt_mats = src->mt_mats; c->mt_tex = src->mt_tex; c->mt_faces = src->mt_faces;
    c->cm.model = src->cm.model; c->cm.dev = src->cm.dev;                   // §25: the camera model travels, the ray buffers do not
    if ((st = finish_ctx(c)) != MCPT_OK) return st;
    if (src->dynamic && (st = rf_clone(c, src)) != MCPT_OK) return st;
    c->info.upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out_ctx = guard.release();
    return MCPT_OK;
}

mcpt_status mcpt_destroy(mcpt_ctx* ctx) {
    if (!ctx) return MCPT_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    destroy_ctx(ctx);
    return MCPT_OK;
}

mcpt_status mcpt_get_scene_info(const mcpt_ctx* ctx, mcpt_scene_info* out) {
    if (!ctx || !out) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    *out = ctx->info;
    return MCPT_OK;
}

static mcpt_status check_pending_jobs(mcpt_ctx* ctx);
// Reads the durations of finished render calls (oldest first).  `block`: wait for all of them -- every entry point that drains the stream
// anyway, and a render call when per-kernel timing is on (its sampled kernel events are per call).  Otherwise only what has finished.
static mcpt_status resolve_timing(mcpt_ctx* c, bool block) {
    while (c->timed_tail != c->timed_head) {
        const uint32_t k = c->timed_tail % mcpt_ctx::TIMED;
        bool done; HIP_TRY(event_done(c->ev1[k], block, done));
        if (!done) break;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0[k], c->ev1[k]));
        c->last_kernel_ms = ms; c->total_kernel_ms += ms; c->timed_tail++;
        if (c->use_wavefront && c->knobs.time_kernels && c->timed_tail == c->timed_head) {   // (per-kernel timing: calls are resolved one at a time, see mcpt_render_tiles)
            double sh = 0.0, tr = 0.0;
            for (auto& L : c->lanes) {
                if (L.last_timed) {                                          // sampled iterations stand for all of them
                    double s_ = 0.0, t_ = 0.0;
                    for (uint64_t i = 0; i < L.last_timed; i++) {
                        float a_ = 0.f, b_ = 0.f;
                        HIP_TRY(hipEventElapsedTime(&a_, L.k_ev[3 * i], L.k_ev[3 * i + 1]));
                        HIP_TRY(hipEventElapsedTime(&b_, L.k_ev[3 * i + 1], L.k_ev[3 * i + 2]));
                        s_ += a_; t_ += b_;
                    }
                    const double scale = double(L.last_iterations) / double(L.last_timed);
                    sh += s_ * scale; tr += t_ * scale;
                }
                L.last_iterations = 0; L.last_timed = 0;
            }
            c->last_shade_ms = sh; c->last_trace_ms = tr; c->total_shade_ms += sh; c->total_trace_ms += tr;
        }
    }
    return block ? check_pending_jobs(c) : MCPT_OK;                        // (everything has finished: the known-length jobs' snapshots are in)
}

// A sub-pipeline's path pool, allocated on first use and grown (never shrunk) to the largest job seen: a 48 x 48 film gets a few hundred KB,
// the 1024-spp bench job its 2^23 slots (1.4 GB per sub-pipeline).  All slot state is dead between render calls, so growing loses nothing.
static mcpt_status ensure_pool(mcpt_ctx* ctx, mcpt_ctx::WfLane& L, uint32_t P) {
    if (L.pool.P >= P) return MCPT_OK;
    HIP_TRY(hipStreamSynchronize(L.stream)); HIP_TRY(hipStreamSynchronize(ctx->stream));
    L.pool_bufs.clear(); L.pool.P = 0;                                   // (the old buffers are freed before the new ones are asked for)
    // the drain compaction's scratch: half a pool of the seven records a live slot carries from one iteration to the next (+ 4096 slots of rounding)
    const bool want_compact = P >= 4 * WF_COMPACT_MIN_SLOTS && !(ctx->opts.flags & MCPT_FLAG_DETERMINISTIC) && ctx->knobs.compact;
    const uint32_t eighths = ctx->knobs.compact_eighths;                 // compact when at most this many eighths of the swept slots are alive
    const uint32_t ccap = want_compact ? uint32_t(uint64_t(P) * eighths / 8) + 4096 : 0, nb = P / WF_SHADE_BLOCK;
    L.compact = CompactBufs{}; L.compact.capacity = ccap; L.compact.eighths = eighths;
    PathPool& pl = L.pool; CompactBufs& cb = L.compact;
    // one row per buffer: the field it fills (whose type gives the element size) and its element count -- per slot, per shade block or per scratch slot
    struct Row { void** field; size_t elem; uint32_t count; };
    auto row = [](auto*& field, uint32_t count) { return Row{(void**)&field, sizeof(*field), count}; };
    const Row rows[] = {
        row(pl.ray_o, P), row(pl.ray_d, P), row(pl.hit, P), row(pl.sq_d, P), row(pl.nee, P), row(pl.L, P), row(pl.beta, P), row(pl.sum, P), row(pl.ids, P),
        row(pl.shadow_queue, P), row(pl.shadow_count, nb), row(pl.sq_o, P), row(pl.block_items, nb), row(pl.live_cnt, nb),
        row(cb.beta, ccap), row(cb.L, ccap), row(cb.ray_d, ccap), row(cb.ray_o, ccap), row(cb.hit, ccap), row(cb.nee, ccap), row(cb.ids, ccap), row(cb.dst_off, nb)};
    for (const Row& r : rows) {
        const size_t bytes = size_t(r.count) * r.elem;
        DevBytes b;
        HIP_TRY(b.alloc(bytes, &ctx->info.device_bytes));
        HIP_TRY(hipMemsetAsync(b.p, 0, bytes, L.stream));
        *r.field = b.p;
        L.pool_bufs.push_back(std::move(b));
    }
    HIP_TRY(hipStreamSynchronize(L.stream));                             // (a caller on ctx->stream, mcpt_probe_trace4, sees filled buffers too)
    L.pool.P = P;
    return MCPT_OK;
}

// Look at the snapshots known-length jobs left behind.  `block`: wait for every one of them (the caller has synchronised, or is about to
// synchronise, the stream anyway); otherwise only those that have arrived.  A job that did not finish inside its bound, or whose trace kernel
// raised the watchdog flag, is an internal error and is reported by whichever call gets here first.
static mcpt_status check_lane_verdicts(mcpt_ctx::WfLane& L, bool block) {
    while (!L.verdicts.empty()) {
        const mcpt_ctx::WfLane::Verdict v = L.verdicts.front();
        bool done; HIP_TRY(event_done(L.chk_ev[v.ring_slot], block, done));
        if (!done) break;
        L.verdicts.erase(L.verdicts.begin());
        const JobState js = job_state(L.h_ctl[v.ring_slot], v.it, v.n_shared);
        if (js == JobState::Watchdog) return fail(MCPT_ERR_HIP, WATCHDOG_MSG);
        if (js != JobState::Finished) return fail(MCPT_ERR_HIP, "a known-length job did not finish within its iteration bound (internal error)");
    }
    return MCPT_OK;
}
static mcpt_status check_pending_jobs(mcpt_ctx* ctx) {
    for (auto& L : ctx->lanes) { mcpt_status st = check_lane_verdicts(L, true); if (st != MCPT_OK) return st; }
    return MCPT_OK;
}

// ---- The executor of a WfPlan: wf_plan.h decides what a call's shape makes of it, everything from here to render_wavefront's end launches it.
constexpr uint32_t WF_CHECK = 4, WF_RING = 8;     // a polled job snapshots its control block every WF_CHECK iterations, into a ring of WF_RING slots
// What changes while a sub-pipeline's loop runs; the rest is its WfLanePlan.
struct Run { const WfLanePlan* plan = nullptr; PathPool pool; uint32_t it = 0, issued = 0, seen = 0, snap_it[WF_RING] = {0}; size_t kev = 0; bool done = false;
             uint32_t grid = 0;         // blocks of this sub-pipeline's trace launches (WfLanePlan::grid, until wf_poll sees a compacted sweep)
             bool drain = false; };     // drain: a snapshot showed the shared work-item cursors moving -> the compaction launches follow every trace launch from here on
static hipError_t wf_k_event(mcpt_ctx::WfLane& L, Run& r, bool timed) {
    if (!timed) return hipSuccess;
    if (r.kev == L.k_ev.size()) { Event ev; hipError_t e = hipEventCreate(ev.out()); if (e != hipSuccess) return e; L.k_ev.push_back(std::move(ev)); }
    return hipEventRecord(L.k_ev[r.kev++], L.stream);
}
// the control block as it is after the launches enqueued so far, copied to slot q of the sub-pipeline's ring, and the event that says it has arrived
static hipError_t wf_snapshot(mcpt_ctx::WfLane& L, uint32_t q) {
    const hipError_t e = hipMemcpyAsync(&L.h_ctl[q], L.ctl_buf.p, sizeof(IterCtl), hipMemcpyDeviceToHost, L.stream);
    return e != hipSuccess ? e : hipEventRecord(L.chk_ev[q], L.stream);
}
// consume finished control-block snapshots of one sub-pipeline; `block` waits for the oldest one
static mcpt_status wf_poll(mcpt_ctx::WfLane& L, Run& r, const WfPlan& plan, bool debug, bool block) {
    const uint32_t n_shared = r.plan->n_shared;
    while (r.seen < r.issued) {
        const uint32_t k = r.seen % WF_RING;
        bool done; HIP_TRY(event_done(L.chk_ev[k], block, done));
        if (!done) break;
        block = false;
        const IterCtl& s = L.h_ctl[k];
        const uint32_t it_of = r.snap_it[k];                           // snapshot taken after iteration it_of
        if (debug && (r.seen < 40 || s.pad[WF_CTL_P_ACTIVE]))
            fprintf(stderr, "[wf] it=%u active=%u head=%u cursor0=%u/%u swept=%u live@compaction=%u compactions=%u\n", it_of, s.any_active[it_of & 3],
                    s.trace_head[it_of & 3], s.item_cursor[0].v, wf_shard_capacity(n_shared, 0), s.pad[WF_CTL_P_ACTIVE], s.pad[WF_CTL_LIVE], s.pad[WF_CTL_COMPACTIONS]);
        const JobState js = job_state(s, it_of, n_shared);
        if (js == JobState::Watchdog) return fail(MCPT_ERR_HIP, WATCHDOG_MSG);
        if (js == JobState::Finished) r.done = true;
        // the compaction launches start as soon as the SHARED cursors move at all: a block turns to them when its private range (90 % of the items) is
        // used up, i.e. in the last tenth of the job -- the host reads snapshots 4 - 8 iterations late, and a drain lasts about ten; the plan kernel
        // itself waits until every item has been handed out
        if (plan.small_job && s.pad[WF_CTL_P_ACTIVE] != 0u && s.pad[WF_CTL_P_ACTIVE] <= plan.small_job) r.grid = plan.shared_grid;   // (the compacted sweep of a draining job)
        if (!r.drain) { uint64_t moved = 0; for (uint32_t q = 0; q < WF_ITEM_SHARDS; q++) moved += s.item_cursor[q].v; if (moved != 0) r.drain = true; }   // (a job has at least one shared item: none left => moved)
        r.seen++;
    }
    return MCPT_OK;
}

// One mcpt_render call: plan it; per active sub-pipeline, in their order, grow its pool and look at the verdicts of its earlier jobs; then
// their streams fork from the context's stream, run their [shade, trace] loops and join it.
static mcpt_status render_wavefront(mcpt_ctx* ctx, const RenderParams& p0, float4* accum) {
    const WfKnobs& knobs = ctx->knobs;
    const WfPlan plan = wf_plan_call(p0, uint32_t(ctx->lanes.size()), knobs, ctx->trace_grid, wf_trace_block_threads());
    const uint32_t n_lanes = uint32_t(plan.lanes.size());
    const bool count = (p0.flags & MCPT_FLAG_COUNT_TRAVERSAL) != 0;
    DevCounters* cnt = ctx->counters.p;
    std::vector<Run> runs(n_lanes);
    for (uint32_t k = 0; k < n_lanes; k++) {
        const WfLanePlan& lp = plan.lanes[k]; mcpt_ctx::WfLane& L = ctx->lanes[k]; Run& r = runs[k];
        r.plan = &lp; r.done = !lp.active; r.grid = lp.grid;
        if (!lp.active) { L.last_iterations = 0; L.last_timed = 0; continue; }
        mcpt_status st = ensure_pool(ctx, L, lp.P); if (st != MCPT_OK) return st;
        r.pool = L.pool;
        r.pool.P = lp.P;                                                  // (a smaller job sweeps only the slots it needs)
        // snapshots of earlier known-length jobs on this sub-pipeline: a polled job starts with none outstanding (it takes the ring's slots
        // in turn from 0), a known-length one needs a free slot for its own
        st = check_lane_verdicts(L, lp.bound == 0); if (st != MCPT_OK) return st;
        if (L.verdicts.size() > WF_RING - 2) { st = check_lane_verdicts(L, true); if (st != MCPT_OK) return st; }
    }
    HIP_TRY(hipEventRecord(ctx->fork_ev, ctx->stream));
    for (uint32_t k = 0; k < n_lanes; k++) {
        if (!plan.lanes[k].active) continue;
        mcpt_ctx::WfLane& L = ctx->lanes[k];
        HIP_TRY(hipStreamWaitEvent(L.stream, ctx->fork_ev, 0));
        HIP_TRY(launch_wf_pool_reset(runs[k].pool, L.ctl_buf.p, L.stream));   // every slot DEAD, control block zeroed
    }
    // the shade interlock (wf_plan.h): `last_shade` recorded the latest shade event of THIS call, so every wait names an event already enqueued
    auto state_of = [&](uint32_t j) { return WfLaneState{runs[j].done, runs[j].grid}; };
    int last_shade = WF_NO_LANE; uint32_t n_waits = 0;
    bool all_done = plan.n_active == 0;
    while (!all_done) {
        all_done = true;
        for (uint32_t k = 0; k < n_lanes; k++) {                            // one iteration of every live sub-pipeline per round
            Run& r = runs[k];
            if (r.done) continue;
            const WfLanePlan& lp = plan.lanes[k]; mcpt_ctx::WfLane& L = ctx->lanes[k];
            IterCtl* ctl = L.ctl_buf.p;
            const bool timed = knobs.time_kernels && r.it % knobs.time_kernels == 0;
            const int wait_for = wf_shade_wait(plan, p0, knobs, k, state_of, last_shade);
            if (wait_for != WF_NO_LANE) { HIP_TRY(hipStreamWaitEvent(L.stream, ctx->lanes[wait_for].shade_ev, 0)); n_waits++; }   // (ahead of the first kernel event: the sampled shade time stays the kernel's)
            HIP_TRY(wf_k_event(L, r, timed));
            HIP_TRY(launch_wf_shade(ctx->dev, lp.p, r.pool, ctl, r.it, lp.n_shared, accum, cnt, L.stream));
            if (wf_lane_gated(plan, p0, knobs, k, state_of(k))) { HIP_TRY(hipEventRecord(L.shade_ev, L.stream)); last_shade = int(k); }
            HIP_TRY(wf_k_event(L, r, timed));
            HIP_TRY(launch_wf_trace(ctx->dev, r.pool, ctl, r.it, ctx->tune, count, cnt, r.grid, L.ovf_buf.p, L.stream));
            HIP_TRY(wf_k_event(L, r, timed));
            // end-of-job drain: move the live slots to the front of the pool once at most half of the swept ones are alive (decided on the device)
            if (r.drain && !lp.bound && L.compact.capacity && lp.p.samples_per_item == 1 && !p0.probe_n)
                HIP_TRY(launch_wf_compact(r.pool, L.compact, ctl, r.it, lp.n_shared, lp.p.priv_items, L.stream));
            r.it++;
            if (lp.bound && r.it == lp.bound) {                             // known-length job: all of it is enqueued; its verdict is read later
                const uint32_t q = L.ring_next++ % WF_RING;
                HIP_TRY(wf_snapshot(L, q));
                L.verdicts.push_back({q, r.it - 1, lp.n_shared});
                r.done = true;
                continue;
            }
            if (!lp.bound && r.it % WF_CHECK == 0) {
                mcpt_status ps = wf_poll(L, r, plan, knobs.debug, r.issued - r.seen >= 2); if (ps != MCPT_OK) return ps;   // at most 2 checks (8 iterations) ahead
                if (!r.done) {
                    const uint32_t q = r.issued % WF_RING;
                    HIP_TRY(wf_snapshot(L, q));
                    r.snap_it[q] = r.it - 1;
                    r.issued++;
                }
            }
            if (!r.done) { mcpt_status ps = wf_poll(L, r, plan, knobs.debug, false); if (ps != MCPT_OK) return ps; }
            if (r.it > knobs.max_it) return fail(MCPT_ERR_HIP, "wavefront loop did not terminate within MCPT_WF_MAXIT iterations");
            if (!r.done) all_done = false;
        }
    }
    if (knobs.debug) fprintf(stderr, "[wf] interlock waits=%u\n", n_waits);
    for (uint32_t k = 0; k < n_lanes; k++) {
        if (!plan.lanes[k].active) continue;
        mcpt_ctx::WfLane& L = ctx->lanes[k];
        L.last_iterations = runs[k].it; L.last_timed = runs[k].kev / 3;
        ctx->total_iterations += runs[k].it;
        HIP_TRY(hipEventRecord(L.done_ev, L.stream));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, L.done_ev, 0));            // join: the caller's stream continues after every sub-pipeline
    }
    return MCPT_OK;
}

// The bracket of a timed call: an event pair of the ring around its stream work, and the call counts as a launch.  Durations of earlier calls: read what
// has finished; wait only when the ring is full -- or when per-kernel timing is on, whose sampled kernel events belong to one call at a time.
static mcpt_status timed_begin(mcpt_ctx* ctx) {
    mcpt_status st = resolve_timing(ctx, ctx->knobs.time_kernels != 0 || ctx->timed_head - ctx->timed_tail >= mcpt_ctx::TIMED - 1); if (st != MCPT_OK) return st;
    HIP_TRY(hipEventRecord(ctx->ev0[ctx->timed_head % mcpt_ctx::TIMED], ctx->stream));
    return MCPT_OK;
}
static mcpt_status timed_end(mcpt_ctx* ctx) {
    HIP_TRY(hipEventRecord(ctx->ev1[ctx->timed_head % mcpt_ctx::TIMED], ctx->stream));
    ctx->timed_head++; ctx->launches++;
    return MCPT_OK;
}

mcpt_status mcpt_render(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample) { return mcpt_render_tiles(ctx, spp, seed, first_sample, 1u, 0u); }

// One render call: `spp` samples of the tiles (tile_mod, tile_rem) selects -- of the tile numbers themselves, or, with a device list `list` of
// n_list entries, of the list -- into `accum`.  `timed`: bracket it with an event pair and count it as a launch (what every entry point does;
// mcpt_render_adaptive brackets its passes as one call instead).
static mcpt_status render_call(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample, uint32_t tile_mod, uint32_t tile_rem,
                               const uint32_t* list, uint32_t n_list, float4* accum, bool timed) {
    if (spp == 0) return MCPT_OK;
    if (!ctx->use_wavefront && !ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the megakernel's traversal stack");
    mcpt_status st;
    if (timed) { st = timed_begin(ctx); if (st != MCPT_OK) return st; }
    RenderParams p;
    const WfCall verdict = wf_plan_params(p, list ? uint64_t(n_list) : film_tiles(ctx), tile_mod, tile_rem, spp, first_sample, seed, ctx->opts, ctx->use_wavefront);
    if (verdict == WfCall::Nothing) return MCPT_OK;                       // more shards than tiles: nothing for this one
    if (verdict == WfCall::TooLarge) return fail(MCPT_ERR_UNSUPPORTED, "launch too large: lower spp per call or raise samples_per_item");
    p.tiles_x = uint32_t((ctx->width + 7) / 8); p.tiles_y = uint32_t((ctx->height + 7) / 8); p.tile_list = list;
    if (ctx->use_wavefront) {
        st = render_wavefront(ctx, p, accum); if (st != MCPT_OK) return st;
    } else {
        HIP_TRY(launch_render(ctx->dev, p, accum, ctx->counters.p, ctx->stream));
    }
    return timed ? timed_end(ctx) : MCPT_OK;
}

mcpt_status mcpt_render_tiles(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample, uint32_t tile_mod, uint32_t tile_rem) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (tile_mod == 0 || tile_rem >= tile_mod) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_tiles: need tile_rem < tile_mod");
    return render_call(ctx, spp, seed, first_sample, tile_mod, tile_rem, nullptr, 0u, ctx->accum, true);
}

mcpt_status mcpt_render_tile_list(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample, const uint32_t* tiles, uint32_t n_tiles) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (n_tiles == 0) return MCPT_OK;
    if (!tiles) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_tile_list: null list");
    // one-sample items write the film with a plain read-modify-write (RenderParams::atomic_accum = 0): a tile listed twice would race with itself
    const uint64_t all = film_tiles(ctx);
    if (n_tiles > all) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_tile_list: more tiles than the image has (a duplicate)");
    std::vector<uint8_t> seen(all, 0);
    for (uint32_t i = 0; i < n_tiles; i++) {
        if (tiles[i] >= all) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_tile_list: tile " + std::to_string(tiles[i]) + " out of range");
        if (seen[tiles[i]]++) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_tile_list: tile " + std::to_string(tiles[i]) + " listed twice");
    }
    if (spp == 0) return MCPT_OK;
    HIP_TRY(ctx->tl_stage.wait());
    if (ctx->tl_stage.cap < n_tiles) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));                        // (kernels of earlier calls may still read the device list)
        HIP_TRY(alloc_all(Want(ctx->tl_dev, n_tiles, &ctx->info.device_bytes), Want(ctx->tl_stage, n_tiles)));   // the longer pair replaces the old one
    }
    std::memcpy(ctx->tl_stage.host, tiles, size_t(n_tiles) * sizeof(uint32_t));
    HIP_TRY(ctx->tl_stage.send(ctx->tl_dev.p, 0, n_tiles, ctx->stream));
    return render_call(ctx, spp, seed, first_sample, 1u, 0u, ctx->tl_dev.p, n_tiles, ctx->accum, true);
}

// Make the context's device current, drain its stream and read the finished calls' durations.
static mcpt_status use_drained(mcpt_ctx* ctx) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return resolve_timing(ctx);
}
mcpt_status mcpt_sync(mcpt_ctx* ctx) { return use_drained(ctx); }

// Every device-to-host read of a handed-out context: the copy in stream order, the stream drained (`host` is complete and may be let go), and,
// with `timing`, the finished calls' durations read -- what the read entry points do once their arguments are checked.
static mcpt_status read_back(mcpt_ctx* ctx, void* host, const void* dev, size_t bytes, bool timing) {
    if (bytes) HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return timing ? resolve_timing(ctx) : MCPT_OK;
}
mcpt_status mcpt_read_accum(mcpt_ctx* ctx, float* rgba_host) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!rgba_host) return fail(MCPT_ERR_INVALID_ARG, "null output");
    return read_back(ctx, rgba_host, ctx->accum, size_t(ctx->width) * ctx->height * sizeof(float4));
}
mcpt_status mcpt_write_accum(mcpt_ctx* ctx, const float* rgba_host) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!rgba_host) return fail(MCPT_ERR_INVALID_ARG, "null input");
    HIP_TRY(hipMemcpyAsync(ctx->accum, rgba_host, size_t(ctx->width) * ctx->height * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));                        // (the caller's array is free again)
    return MCPT_OK;
}
mcpt_status mcpt_clear_accum(mcpt_ctx* ctx) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    HIP_TRY(hipMemsetAsync(ctx->accum, 0, size_t(ctx->width) * ctx->height * sizeof(float4), ctx->stream));
    return MCPT_OK;
}

// tonemap_kernel over `film` into the context's persistent u8 buffer, copied to its pinned host image on the context's stream; returns after
// the stream has drained (the image is complete).  The kernel writes every byte: nothing to clear.
static mcpt_status tonemap_to_pinned(mcpt_ctx* ctx, const float4* film, int flip_y) {
    const size_t n = size_t(ctx->width) * ctx->height;
    if (!ctx->tone_dev.p) HIP_TRY(alloc_all(Want(ctx->tone_dev, 3 * n), Want(ctx->tone_host, 3 * n)));
    HIP_TRY(launch_tonemap(film, ctx->tone_dev.p, ctx->width, ctx->height, flip_y, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->tone_host, ctx->tone_dev.p, 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return resolve_timing(ctx);
}
// ... and copied on into the caller's image
static mcpt_status tonemap_to_host(mcpt_ctx* ctx, const float4* film, uint8_t* rgb_host, int flip_y) {
    const mcpt_status st = tonemap_to_pinned(ctx, film, flip_y);
    if (st == MCPT_OK) std::memcpy(rgb_host, ctx->tone_host, 3 * size_t(ctx->width) * ctx->height);
    return st;
}

mcpt_status mcpt_tonemap(mcpt_ctx* ctx, uint8_t* rgb_host, int flip_y) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!rgb_host) return fail(MCPT_ERR_INVALID_ARG, "null output");
    return tonemap_to_host(ctx, ctx->accum, rgb_host, flip_y);
}

/* The same without the last copy: *out_rgb points at the context's own pinned host image (width * height * 3 bytes), valid until the next
 * tonemap call on this context or its destruction -- what Scene::getPixelsColor hands out (Scene.cpp:23-33 returns a pointer into the
 * Scene's own vector, overwritten by the next call). */
mcpt_status mcpt_tonemap_map(mcpt_ctx* ctx, int flip_y, const uint8_t** out_rgb) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out_rgb) return fail(MCPT_ERR_INVALID_ARG, "null output");
    *out_rgb = nullptr;
    st = tonemap_to_pinned(ctx, ctx->accum, flip_y); if (st != MCPT_OK) return st;
    *out_rgb = ctx->tone_host;
    return MCPT_OK;
}

/* Scene::getPixelsColor of ANY film of this context's size that lives on its device -- e.g. the sum of several devices' films, reduced
 * into a scratch buffer for a progressive image of a multi-GPU render (mcpt_cli --gpus N --save-every K). */
mcpt_status mcpt_tonemap_buffer(mcpt_ctx* ctx, const void* device_rgba, uint8_t* rgb_host, int flip_y) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!rgb_host || !device_rgba) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    return tonemap_to_host(ctx, static_cast<const float4*>(device_rgba), rgb_host, flip_y);
}

mcpt_status mcpt_get_counters(mcpt_ctx* ctx, mcpt_counters* out) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    std::vector<DevCounters> rep(WF_COUNTER_REPLICAS);               // kernels spread their atomics over replicas; sum them here
    st = read_back(ctx, rep.data(), ctx->counters.p, ctx->counters.bytes); if (st != MCPT_OK) return st;
    std::memset(out, 0, sizeof *out);
    for (const DevCounters& r : rep) {
        out->paths += r.paths; out->rays_primary += r.rays_primary; out->rays_continuation += r.rays_continuation; out->rays_shadow += r.rays_shadow;
        out->box_tests += r.box_tests; out->tri_tests += r.tri_tests; out->shaded_hits += r.shaded_hits; out->texel_fetches += r.texel_fetches;
        out->self_shadow_tests += r.self_shadow_tests; out->self_shadow_hits += r.self_shadow_hits; out->stack_spills += r.stack_spills; for (int q = 0; q < 4; q++) out->debug[q] += r.debug[q];
    }
    out->kernel_ms = ctx->last_kernel_ms; out->kernel_ms_total = ctx->total_kernel_ms; out->launches = ctx->launches;
    out->trace_ms_total = ctx->total_trace_ms; out->shade_ms_total = ctx->total_shade_ms; out->iterations = ctx->total_iterations;
    return MCPT_OK;
}
mcpt_status mcpt_reset_counters(mcpt_ctx* ctx) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    HIP_TRY(hipMemsetAsync(ctx->counters.p, 0, ctx->counters.bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    st = resolve_timing(ctx); if (st != MCPT_OK) return st;
    ctx->total_kernel_ms = 0.0; ctx->launches = 0; ctx->total_trace_ms = 0.0; ctx->total_shade_ms = 0.0; ctx->total_iterations = 0;
    return MCPT_OK;
}

mcpt_status mcpt_bind_accum(mcpt_ctx* ctx, void* device_rgba) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->accum = device_rgba ? static_cast<float4*>(device_rgba) : ctx->accum_own.p;
    return MCPT_OK;
}
mcpt_status mcpt_accum_device_ptr(mcpt_ctx* ctx, void** out_device_rgba) {
    if (!ctx || !out_device_rgba) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    *out_device_rgba = ctx->accum;
    return MCPT_OK;
}
mcpt_status mcpt_set_stream(mcpt_ctx* ctx, void* hip_stream) {
    mcpt_status st = use_drained(ctx); if (st != MCPT_OK) return st;
    ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return MCPT_OK;
}

mcpt_status mcpt_set_null_stream(mcpt_ctx* ctx) {
    mcpt_status st = use_drained(ctx); if (st != MCPT_OK) return st;
    ctx->stream = nullptr;                                             // the device's legacy default stream
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ denoised preview
// The features of the current scene and view into dn_feat (allocated by the caller) on the context's stream -- and, once the context owns the
// emission buffer, the emission in the same traversal.  Remembers what they were rendered with: a later split denoise renders the emission of
// features that lack it from the same samples.
static mcpt_status dn_render_features(mcpt_ctx* ctx, uint32_t spp, uint64_t seed) {
    HIP_TRY(launch_dn_features(ctx->dev, spp, uint32_t(seed), uint32_t(seed >> 32), ctx->dn_feat.p, ctx->dn_emis.p, ctx->stream));
    ctx->dn_have_features = true; ctx->dn_have_emis = ctx->dn_emis.p != nullptr;
    ctx->dn_feat_spp = spp; ctx->dn_feat_seed = seed;
    return MCPT_OK;
}

mcpt_status mcpt_render_features(mcpt_ctx* ctx, uint32_t spp, uint64_t seed) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (spp < 1 || spp > DN_MAX_SPP) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_features: need 1 <= spp <= 64");
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the feature kernel's traversal stack");
    const size_t n = size_t(ctx->width) * ctx->height;
    if (!ctx->dn_feat.p) HIP_TRY(ctx->dn_feat.alloc(2 * n, &ctx->info.device_bytes));
    return dn_render_features(ctx, spp, seed);
}

mcpt_status mcpt_read_features(mcpt_ctx* ctx, float* out8) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out8) return fail(MCPT_ERR_INVALID_ARG, "null output");
    if (!ctx->dn_have_features) return fail(MCPT_ERR_INVALID_ARG, "mcpt_read_features: no features rendered yet (mcpt_render_features)");
    return read_back(ctx, out8, ctx->dn_feat.p, ctx->dn_feat.bytes);
}

// The options of a filter call, read and checked: what mcpt_denoise and mcpt_probe_denoise both refuse, before anything else of the call.
static mcpt_status dn_read_opts(const mcpt_denoise_opts* opts, mcpt_denoise_opts& o, const char* fn) {
    const mcpt_status st = read_opts(opts, o, fn, "mcpt_denoise_opts"); if (st != MCPT_OK) return st;
    const std::string who = std::string(fn) + ": ";
    if (o.iterations > DN_MAX_LEVELS) return fail(MCPT_ERR_INVALID_ARG, who + "at most 10 iterations");
    if (!(o.sigma_color >= 0.f) || !(o.sigma_normal >= 0.f) || !(o.sigma_depth >= 0.f)) return fail(MCPT_ERR_INVALID_ARG, who + "sigmas must be >= 0 (0 = default)");
    if (o.flags & ~(MCPT_DENOISE_SPLIT_EMISSION | MCPT_DENOISE_CLAMP_FIREFLIES)) return fail(MCPT_ERR_INVALID_ARG, who + "unknown bit in flags");
    if (o.firefly_clamp != 0.f && !(std::isfinite(o.firefly_clamp) && o.firefly_clamp >= 1.f)) return fail(MCPT_ERR_INVALID_ARG, who + "firefly_clamp must be finite and >= 1 (0 = default)");
    return MCPT_OK;
}
// The filter's parameters from checked options (defaults filled in) and the context's film size and camera; `levels` gets the a-trous levels.
static DnParams dn_params(const mcpt_ctx* ctx, const mcpt_denoise_opts& o, uint32_t& levels) {
    DnParams p;
    p.width = ctx->width; p.height = ctx->height;
    p.sigma_c = o.sigma_color > 0.f ? o.sigma_color : 4.f;
    p.sigma_n = o.sigma_normal > 0.f ? o.sigma_normal : 128.f;
    p.sigma_z = o.sigma_depth > 0.f ? o.sigma_depth : 4.f;
    p.theta = float(ctx->dev.cam.h / double(ctx->height));
    p.clamp_k = !(o.flags & MCPT_DENOISE_CLAMP_FIREFLIES) ? 0.f : o.firefly_clamp > 0.f ? o.firefly_clamp : MCPT_DENOISE_DEFAULT_FIREFLY_CLAMP;
    levels = o.iterations ? o.iterations : 5u;
    return p;
}

mcpt_status mcpt_denoise(mcpt_ctx* ctx, const void* device_rgba, const mcpt_denoise_opts* opts) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    mcpt_denoise_opts o;
    st = dn_read_opts(opts, o, "mcpt_denoise"); if (st != MCPT_OK) return st;
    if (!ctx->dn_have_features) return fail(MCPT_ERR_INVALID_ARG, "mcpt_denoise: no features rendered yet (mcpt_render_features)");
    const size_t n = size_t(ctx->width) * ctx->height;
    uint64_t* tally = &ctx->info.device_bytes;
    const bool split = (o.flags & MCPT_DENOISE_SPLIT_EMISSION) != 0;
    HIP_TRY(alloc_all(Want(ctx->dn_guide, n, tally, !ctx->dn_out.p), Want(ctx->dn_iv0, n, tally, !ctx->dn_out.p), Want(ctx->dn_iv1, n, tally, !ctx->dn_out.p),
                      Want(ctx->dn_out, n, tally, !ctx->dn_out.p), Want(ctx->dn_emis, n, tally, split && !ctx->dn_emis.p)));
    if (split && !ctx->dn_have_emis) {                                     // features rendered before the context owned the buffer: the same samples again
        HIP_TRY(launch_dn_features(ctx->dev, ctx->dn_feat_spp, uint32_t(ctx->dn_feat_seed), uint32_t(ctx->dn_feat_seed >> 32), nullptr, ctx->dn_emis.p, ctx->stream));
        ctx->dn_have_emis = true;
    }
    uint32_t levels;
    const DnParams p = dn_params(ctx, o, levels);
    const float4* film = device_rgba ? static_cast<const float4*>(device_rgba) : ctx->accum;
    HIP_TRY(launch_dn_filter(p, levels, film, ctx->dn_feat.p, split ? ctx->dn_emis.p : nullptr, ctx->dn_guide.p, ctx->dn_iv0.p, ctx->dn_iv1.p, ctx->dn_out.p,
                             ctx->stream));
    ctx->dn_have_out = true;
    return MCPT_OK;
}

// The filter alone on caller films, features and emission of the context's film size, in scratch buffers on the context's stream: nothing of
// the context's own denoiser state (features, emission, denoised film, device_bytes) is read or written.
mcpt_status mcpt_probe_denoise(mcpt_ctx* ctx, const float* film_rgba_host, const float* feat8_host, const float* emis4_host, const mcpt_denoise_opts* opts,
                               float* out_rgba_host) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!film_rgba_host || !feat8_host || !out_rgba_host) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    mcpt_denoise_opts o;
    st = dn_read_opts(opts, o, "mcpt_probe_denoise"); if (st != MCPT_OK) return st;
    const bool split = (o.flags & MCPT_DENOISE_SPLIT_EMISSION) != 0;
    if (split && !emis4_host) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_denoise: MCPT_DENOISE_SPLIT_EMISSION needs an emission buffer");
    if (!split && emis4_host) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_denoise: an emission buffer without MCPT_DENOISE_SPLIT_EMISSION");
    const size_t n = size_t(ctx->width) * ctx->height;
    for (size_t i = 0; i < 8 * n; i++)
        if (!std::isfinite(feat8_host[i])) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_denoise: a feature is not finite");
    for (size_t i = 0; i < n; i++)
        if (feat8_host[8 * i + 7] < 0.f) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_denoise: a feature depth is < 0 (the filter marks invalid pixels by a negative depth)");
    for (size_t i = 0; split && i < 4 * n; i++)
        if (!std::isfinite(emis4_host[i])) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_denoise: an emission value is not finite");
    uint32_t levels;
    const DnParams p = dn_params(ctx, o, levels);
    Scratch s(ctx->stream); float4 *film, *feat, *emis = nullptr, *guide, *iv0, *iv1, *out;
    HIP_TRY(s.in(reinterpret_cast<const float4*>(film_rgba_host), n, &film)); HIP_TRY(s.in(reinterpret_cast<const float4*>(feat8_host), 2 * n, &feat));
    if (split) HIP_TRY(s.in(reinterpret_cast<const float4*>(emis4_host), n, &emis));
    HIP_TRY(s.out(n, &guide)); HIP_TRY(s.out(n, &iv0)); HIP_TRY(s.out(n, &iv1)); HIP_TRY(s.out(n, &out));
    HIP_TRY(launch_dn_filter(p, levels, film, feat, emis, guide, iv0, iv1, out, ctx->stream));
    HIP_TRY(s.fetch(reinterpret_cast<float4*>(out_rgba_host), out, n));
    HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_read_emission(mcpt_ctx* ctx, float* out4) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out4) return fail(MCPT_ERR_INVALID_ARG, "null output");
    if (!ctx->dn_have_emis) return fail(MCPT_ERR_INVALID_ARG, "mcpt_read_emission: no emission held (mcpt_denoise with MCPT_DENOISE_SPLIT_EMISSION)");
    return read_back(ctx, out4, ctx->dn_emis.p, ctx->dn_emis.bytes);
}

mcpt_status mcpt_read_denoised(mcpt_ctx* ctx, float* rgba_host) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!rgba_host) return fail(MCPT_ERR_INVALID_ARG, "null output");
    if (!ctx->dn_have_out) return fail(MCPT_ERR_INVALID_ARG, "mcpt_read_denoised: nothing denoised yet (mcpt_denoise)");
    return read_back(ctx, rgba_host, ctx->dn_out.p, ctx->dn_out.bytes);
}

mcpt_status mcpt_denoised_device_ptr(mcpt_ctx* ctx, void** out_device_rgba) {
    if (!ctx || !out_device_rgba) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    *out_device_rgba = nullptr;
    if (!ctx->dn_have_out) return fail(MCPT_ERR_INVALID_ARG, "mcpt_denoised_device_ptr: nothing denoised yet (mcpt_denoise)");
    *out_device_rgba = ctx->dn_out.p;
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ adaptive sampling
// Device buffers of the error + compaction round, allocated on first use and counted in device_bytes (the half films are what costs: 32 B per pixel).
static mcpt_status ad_ensure(mcpt_ctx* ctx) {
    if (ctx->ad_h.p) return MCPT_OK;
    const size_t n = size_t(ctx->width) * ctx->height;
    const uint32_t n_tiles = uint32_t(film_tiles(ctx)), nb = ad_blocks(n_tiles);
    uint64_t* tally = &ctx->info.device_bytes;
    HIP_TRY(alloc_all(Want(ctx->ad_h, n, tally), Want(ctx->ad_o, n, tally), Want(ctx->ad_err, n_tiles, tally), Want(ctx->ad_list, n_tiles, tally),
                      Want(ctx->ad_flags, n_tiles, tally), Want(ctx->ad_counts, nb, tally), Want(ctx->ad_offs, nb, tally), Want(ctx->ad_tot, 1, tally),
                      Want(ctx->ad_host, 1)));
    return MCPT_OK;
}
static AdScratch ad_scratch(mcpt_ctx* ctx) {
    AdScratch s;
    s.block_counts = ctx->ad_counts.p; s.block_offsets = ctx->ad_offs.p; s.flags = ctx->ad_flags.p; s.totals = ctx->ad_tot.p;
    return s;
}

mcpt_status mcpt_render_adaptive(mcpt_ctx* ctx, uint64_t seed, uint32_t first_sample, const mcpt_adaptive_opts* opts, mcpt_adaptive_stats* out_stats) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    mcpt_adaptive_opts o;
    st = read_opts(opts, o, "mcpt_render_adaptive", "mcpt_adaptive_opts"); if (st != MCPT_OK) return st;
    const uint32_t min_spp = o.min_spp ? o.min_spp : 16u, max_spp = o.max_spp ? o.max_spp : 1024u;
    if (min_spp < 2 || (min_spp & 1u)) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_adaptive: min_spp must be even and >= 2");
    if (max_spp < min_spp) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_adaptive: max_spp < min_spp");
    if (!std::isfinite(o.threshold) || o.threshold < 0.f) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_adaptive: threshold must be finite and > 0 (0 = default)");
    if (uint64_t(first_sample) + max_spp > 0x100000000ull) return fail(MCPT_ERR_INVALID_ARG, "mcpt_render_adaptive: first_sample + max_spp overflows the sample index");
    const float thr = o.threshold > 0.f ? o.threshold : MCPT_ADAPTIVE_DEFAULT_THRESHOLD;
    if (!ctx->use_wavefront && !ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the megakernel's traversal stack");
    st = ad_ensure(ctx); if (st != MCPT_OK) return st;
    const size_t n_px = size_t(ctx->width) * ctx->height;
    const uint32_t n_tiles = uint32_t(film_tiles(ctx));
    const AdScratch scr = ad_scratch(ctx);
    mcpt_adaptive_stats stats; std::memset(&stats, 0, sizeof stats); stats.struct_size = sizeof stats;
    st = timed_begin(ctx); if (st != MCPT_OK) return st;
    HIP_TRY(hipMemsetAsync(ctx->ad_h.p, 0, ctx->ad_h.bytes, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->ad_o.p, 0, ctx->ad_o.bytes, ctx->stream));
    ctx->ad_have_err = false;
    // pass 0: every tile, samples [fs, fs + min/2) into H and [fs + min/2, fs + min) into O
    const uint32_t half = min_spp / 2;
    st = render_call(ctx, half, seed, first_sample, 1u, 0u, nullptr, 0u, ctx->ad_h.p, false); if (st != MCPT_OK) return st;
    st = render_call(ctx, half, seed, first_sample + half, 1u, 0u, nullptr, 0u, ctx->ad_o.p, false); if (st != MCPT_OK) return st;
    stats.passes = 1; stats.pixel_samples = uint64_t(min_spp) * n_px;
    uint32_t c = min_spp;                                                  // the count every active tile has
    for (;;) {
        HIP_TRY(launch_ad_error_compact(ctx->ad_h.p, ctx->ad_o.p, ctx->width, ctx->height, thr, max_spp, ctx->ad_err.p, ctx->ad_list.p, scr, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->ad_host, ctx->ad_tot.p, sizeof(AdTotals), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->ad_have_err = true;
        const AdTotals t = *ctx->ad_host;
        if (t.n_active == 0 || c >= max_spp) {                            // (c < max_spp for every active tile: the second test is a guard)
            stats.tiles_capped = t.n_hot; stats.tiles_converged = n_tiles - t.n_hot;
            break;
        }
        // the next pass doubles the active tiles' count, or brings it to max_spp: n samples [fs + c, fs + c + n), the first floor(n/2) into H
        const uint32_t n = std::min(c, max_spp - c), nh = n / 2;
        st = render_call(ctx, nh, seed, first_sample + c, 1u, 0u, ctx->ad_list.p, t.n_active, ctx->ad_h.p, false); if (st != MCPT_OK) return st;
        st = render_call(ctx, n - nh, seed, first_sample + c + nh, 1u, 0u, ctx->ad_list.p, t.n_active, ctx->ad_o.p, false); if (st != MCPT_OK) return st;
        stats.passes++; stats.pixel_samples += uint64_t(n) * t.active_pixels;
        c += n;
    }
    HIP_TRY(launch_ad_merge(ctx->accum, ctx->ad_h.p, ctx->ad_o.p, uint32_t(n_px), ctx->stream));
    st = timed_end(ctx); if (st != MCPT_OK) return st;
    if (out_stats) *out_stats = stats;
    return MCPT_OK;
}

mcpt_status mcpt_read_tile_error(mcpt_ctx* ctx, float* out) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    if (!ctx->ad_have_err) return fail(MCPT_ERR_INVALID_ARG, "mcpt_read_tile_error: no adaptive render yet (mcpt_render_adaptive)");
    return read_back(ctx, out, ctx->ad_err.p, ctx->ad_err.bytes);
}

mcpt_status mcpt_probe_tile_error(mcpt_ctx* ctx, const float* h_rgba_host, const float* o_rgba_host, float threshold, uint32_t max_spp,
                                  float* out_err, uint32_t* out_list, uint32_t* out_n) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!h_rgba_host || !o_rgba_host || !out_err || !out_list || !out_n) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (!std::isfinite(threshold) || threshold < 0.f) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_tile_error: threshold must be finite and >= 0");
    const size_t n_px = size_t(ctx->width) * ctx->height;
    const uint32_t n_tiles = uint32_t(film_tiles(ctx)), nb = ad_blocks(n_tiles);
    Scratch s(ctx->stream); float4 *h, *o; float* err; uint32_t *list, *flags, *offs; uint4* counts; AdTotals* tot;
    HIP_TRY(s.in(reinterpret_cast<const float4*>(h_rgba_host), n_px, &h)); HIP_TRY(s.in(reinterpret_cast<const float4*>(o_rgba_host), n_px, &o));
    HIP_TRY(s.out(n_tiles, &err)); HIP_TRY(s.out(n_tiles, &list)); HIP_TRY(s.out(n_tiles, &flags));
    HIP_TRY(s.out(nb, &offs)); HIP_TRY(s.out(nb, &counts)); HIP_TRY(s.out(1, &tot));
    AdScratch scr; scr.block_counts = counts; scr.block_offsets = offs; scr.flags = flags; scr.totals = tot;
    HIP_TRY(launch_ad_error_compact(h, o, ctx->width, ctx->height, threshold, max_spp, err, list, scr, ctx->stream));
    AdTotals t;
    HIP_TRY(s.fetch(&t, tot, 1)); HIP_TRY(s.fetch(out_err, err, n_tiles)); HIP_TRY(s.fetch(out_list, list, n_tiles));   // (entries past the active ones are 0)
    HIP_TRY(s.finish());
    if (t.n_active > n_tiles) return fail(MCPT_ERR_HIP, "mcpt_probe_tile_error: active count out of range (internal error)");
    *out_n = t.n_active;
    return MCPT_OK;
}


// ------------------------------------------------------------------------------------------------ live scenes
// What a camera for an existing context must be (mcpt_set_camera's rules); `fn` names the entry point in the message.
static mcpt_status check_camera(const mcpt_ctx* ctx, const mcpt_camera* cm, const char* fn) {
    const std::string who = std::string(fn) + ": ";
    if (!cm) return fail(MCPT_ERR_INVALID_ARG, who + "null camera");
    if (cm->width != ctx->width || cm->height != ctx->height) return fail(MCPT_ERR_INVALID_ARG, who + "width / height differ from the context's film");
    bool finite = std::isfinite(cm->fovy);
    for (int a = 0; a < 3; a++) finite = finite && std::isfinite(cm->eye[a]) && std::isfinite(cm->lookat[a]) && std::isfinite(cm->up[a]);
    if (!finite) return fail(MCPT_ERR_INVALID_ARG, who + "a camera field is not finite");
    if (cm->eye[0] == cm->lookat[0] && cm->eye[1] == cm->lookat[1] && cm->eye[2] == cm->lookat[2]) return fail(MCPT_ERR_INVALID_ARG, who + "eye == lookat");
    const std::string bad = camera_defect(*cm);
    if (!bad.empty()) return fail(MCPT_ERR_INVALID_ARG, who + bad);
    return MCPT_OK;
}
// The camera travels by value with every launch (DevScene::cam): launches already enqueued keep the old one, later ones get this one.
static void apply_camera(mcpt_ctx* ctx, const mcpt_camera& cm) {
    camera_constants(cm, ctx->dev.centre, ctx->dev.cam);
    rf_forget_derived(ctx);
}

mcpt_status mcpt_set_camera(mcpt_ctx* ctx, const mcpt_camera* cm) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    st = check_camera(ctx, cm, "mcpt_set_camera"); if (st != MCPT_OK) return st;
    apply_camera(ctx, *cm);
    return MCPT_OK;
}

// mcpt_update_vertices' rules for its arrays, host only; `fn` names the entry point in the message.
static mcpt_status rf_check_update(const mcpt_ctx* ctx, const double* vertex, uint32_t n_vertex, const double* normal, uint32_t n_normal, const char* fn) {
    const std::string who = std::string(fn) + ": ";
    if (!vertex) return fail(MCPT_ERR_INVALID_ARG, who + "null vertex array");
    if (n_vertex != ctx->rf_n_vertex) return fail(MCPT_ERR_INVALID_ARG, who + "n_vertex differs from the scene's");
    if (normal && n_normal != ctx->rf_n_normal) return fail(MCPT_ERR_INVALID_ARG, who + "n_normal differs from the scene's");
    for (uint32_t v = 0; v < n_vertex; v++) {
        if (!ctx->rf_used_vertex[v]) continue;
        const double* x = vertex + 3 * size_t(v);
        if (!(std::fabs(x[0]) <= MCPT_MAX_COORD && std::fabs(x[1]) <= MCPT_MAX_COORD && std::fabs(x[2]) <= MCPT_MAX_COORD))
            return fail(MCPT_ERR_INVALID_ARG, who + "vertex " + std::to_string(v) + ": coordinate is not finite or exceeds 1e18");
    }
    return MCPT_OK;
}
// mcpt_update_transforms' rules for its matrices (§16), host only: no device round trip, hence the conservative row bound against R_g.
static mcpt_status xf_check_update(const mcpt_ctx* ctx, const double* m3x4, uint32_t n_groups, const char* fn) {
    const std::string who = std::string(fn) + ": ";
    if (!ctx->xf.n_groups) return fail(MCPT_ERR_INVALID_ARG, who + "no groups are set (mcpt_set_vertex_groups)");
    if (!m3x4) return fail(MCPT_ERR_INVALID_ARG, who + "null matrices");
    if (n_groups != ctx->xf.n_groups) return fail(MCPT_ERR_INVALID_ARG, who + "n_groups differs from the groups set");
    for (size_t k = 0; k < size_t(n_groups) * 12; k++)
        if (!std::isfinite(m3x4[k])) return fail(MCPT_ERR_INVALID_ARG, who + "group " + std::to_string(k / 12) + ": a matrix entry is not finite");
    for (uint32_t g = 0; g < n_groups; g++) {
        double rec[XF_RECORD];
        xf_group_record(m3x4 + 12 * size_t(g), rec);
        const double det = xf_record_det(rec);
        if (!(std::isfinite(det) && det != 0.0)) return fail(MCPT_ERR_INVALID_ARG, who + "group " + std::to_string(g) + ": det A is zero or not finite");
    }
    for (uint32_t g = 0; g < n_groups; g++)
        for (int r = 0; r < 3; r++) {
            const double reach = xf_row_reach(m3x4 + 12 * size_t(g) + 4 * r, ctx->xf.radius[g]);
            if (!(reach <= MCPT_MAX_COORD)) return fail(MCPT_ERR_INVALID_ARG, who + "group " + std::to_string(g) + ": a vertex could leave |coordinate| <= 1e18 (conservative bound)");
        }
    return MCPT_OK;
}
// mcpt_update_skin's rules for its matrices (§18), host only, as xf_check_update: the conservative row bound against R_b carries a slack factor.
// `every_radius` (§19, morph then skin): the radius that stands for EVERY bone's R_b -- the morphed pose's reach, not the skin's rest pose.
static mcpt_status sk_check_update(const mcpt_ctx* ctx, const double* m3x4, uint32_t n_bones, const char* fn, const double* every_radius = nullptr) {
    const std::string who = std::string(fn) + ": ";
    if (!ctx->sk.n_bones) return fail(MCPT_ERR_INVALID_ARG, who + "no skin is set (mcpt_set_vertex_skin)");
    if (!m3x4) return fail(MCPT_ERR_INVALID_ARG, who + "null matrices");
    if (n_bones != ctx->sk.n_bones) return fail(MCPT_ERR_INVALID_ARG, who + "n_bones differs from the skin set");
    for (size_t k = 0; k < size_t(n_bones) * 12; k++)
        if (!std::isfinite(m3x4[k])) return fail(MCPT_ERR_INVALID_ARG, who + "bone " + std::to_string(k / 12) + ": a matrix entry is not finite");
    for (uint32_t b = 0; b < n_bones; b++) {
        const double det = sk_bone_det(m3x4 + 12 * size_t(b));
        if (!(std::isfinite(det) && det != 0.0)) return fail(MCPT_ERR_INVALID_ARG, who + "bone " + std::to_string(b) + ": det A is zero or not finite");
    }
    const bool dq = ctx->sk.dq();                                                // §21: rigid bones only, and the reach bound in place of the row bound
    for (uint32_t b = 0; dq && b < n_bones; b++)
        if (!sk_bone_rigid(m3x4 + 12 * size_t(b)))
            return fail(MCPT_ERR_INVALID_ARG, who + "bone " + std::to_string(b) + ": not a rigid transform (det A <= 0, or A^T A differs from the identity by more than 1e-6): "
                                                    "dual-quaternion skinning takes rotations and translations only; scaled, sheared or mirrored bones need MCPT_SKIN_LINEAR");
    const auto within = [dq](const double* m, double radius) {                   // the mode's bound on where a bone can take a vertex of that radius
        if (dq) return sk_dq_reach(m, radius) <= MCPT_MAX_COORD;
        return sk_row_reach(m, radius) <= MCPT_MAX_COORD && sk_row_reach(m + 4, radius) <= MCPT_MAX_COORD && sk_row_reach(m + 8, radius) <= MCPT_MAX_COORD;
    };
    for (uint32_t b = 0; b < n_bones; b++)
        if (!within(m3x4 + 12 * size_t(b), every_radius ? *every_radius : ctx->sk.radius[b]))
            return fail(MCPT_ERR_INVALID_ARG, who + "bone " + std::to_string(b) + ": a vertex could leave |coordinate| <= 1e18 (conservative bound)");
    return MCPT_OK;
}
// mcpt_update_morph's rules for its weights and, when given, its bones (§19), host only: the reach E of the morphed pose bounds the vertices, and
// stands for every bone's radius in the skin's row bound.
static mcpt_status mo_check_update(const mcpt_ctx* ctx, const double* weight, uint32_t n_targets, const double* bones, uint32_t n_bones, const char* fn) {
    const std::string who = std::string(fn) + ": ";
    if (!ctx->mo.n_targets) return fail(MCPT_ERR_INVALID_ARG, who + "no morph is set (mcpt_set_vertex_morph)");
    if (!weight) return fail(MCPT_ERR_INVALID_ARG, who + "null weights");
    if (n_targets != ctx->mo.n_targets) return fail(MCPT_ERR_INVALID_ARG, who + "n_targets differs from the morph set");
    for (uint32_t k = 0; k < n_targets; k++)
        if (!(std::fabs(weight[k]) <= MCPT_MAX_COORD)) return fail(MCPT_ERR_INVALID_ARG, who + "target " + std::to_string(k) + ": the weight is not finite or exceeds 1e18");
    const double reach = mo_reach(ctx->mo.radius, weight, ctx->mo.delta.data(), n_targets);
    if (!(reach <= MCPT_MAX_COORD)) return fail(MCPT_ERR_INVALID_ARG, who + "a vertex could leave |coordinate| <= 1e18 (conservative bound)");
    return bones ? sk_check_update(ctx, bones, n_bones, fn, &reach) : MCPT_OK;
}
// mcpt_update_keyframes' rules (§22), host only: set-up has bounded every frame and the reach of every blend, so only the time is judged.
static mcpt_status kf_check_update(const mcpt_ctx* ctx, double time, const char* fn) {
    const std::string who = std::string(fn) + ": ";
    if (!std::isfinite(time)) return fail(MCPT_ERR_INVALID_ARG, who + "the time is not finite");
    if (!ctx->kf.n_frames) return fail(MCPT_ERR_INVALID_ARG, who + "no keyframes are set (mcpt_set_vertex_keyframes)");
    return MCPT_OK;
}
// A scene update and where its new vertices come from: the caller's arrays (rf_check_update), one matrix per group (xf_check_update), one per
// bone (sk_check_update), one weight per morph target alone or in front of the bones (mo_check_update), the time of the keyframes' clock
// (kf_check_update), several of those at once, each for the records it owns (§23, pt_check_update).  None (§20, mcpt_update_normals):
// nothing is staged and no vertex moves; the normals pass and the refit run on the arrays as they are.
struct RfUpdate {
    enum class Source { Arrays, Groups, Skin, Morph, MorphSkin, Keyframes, Parts, None } source = Source::None;
    const mcpt_scene_update* parts = nullptr;                                                               // Parts: the caller's record
    const double* vertex = nullptr; const double* normal = nullptr; uint32_t n_vertex = 0, n_normal = 0;    // Arrays
    const double* m3x4 = nullptr; uint32_t n_m3x4 = 0;                                                      // Groups: per group; Skin, MorphSkin: per bone
    const double* weight = nullptr; uint32_t n_weight = 0;                                                  // Morph, MorphSkin: per target
    double time = 0.0;                                                                                      // Keyframes
    bool lights = false; uint32_t n_lights = 0;                                                             // None, §24: the mask changed -- the light list is rebuilt, to this length
    static RfUpdate none() { return RfUpdate(); }
    static RfUpdate visibility(uint32_t n_lights) { RfUpdate u; u.lights = true; u.n_lights = n_lights; return u; }
    static RfUpdate keyframes(double t) { RfUpdate u; u.source = Source::Keyframes; u.time = t; return u; }
    static RfUpdate arrays(const double* v, uint32_t nv, const double* n, uint32_t nn) {
        RfUpdate u; u.source = Source::Arrays; u.vertex = v; u.n_vertex = nv; u.normal = n; u.n_normal = nn; return u;
    }
    static RfUpdate matrices(Source to, const double* m, uint32_t n) { RfUpdate u; u.source = to; u.m3x4 = m; u.n_m3x4 = n; return u; }
    static RfUpdate groups(const double* m, uint32_t n) { return matrices(Source::Groups, m, n); }
    static RfUpdate skin(const double* m, uint32_t n) { return matrices(Source::Skin, m, n); }
    static RfUpdate morph(const double* w, uint32_t nw, const double* bones, uint32_t n_bones) {             // bones: null = the morph alone
        RfUpdate u = matrices(bones ? Source::MorphSkin : Source::Morph, bones, n_bones); u.weight = w; u.n_weight = nw; return u;
    }
    static RfUpdate of_parts(const mcpt_scene_update* p) { RfUpdate u; u.source = Source::Parts; u.parts = p; return u; }
    // Parts (checked): is its morph followed by the skin?  What its morph route is as an update of its own.
    bool parts_morph_then_skin() const { return source == Source::Parts && (parts->flags & MCPT_PARTS_MORPH_THEN_SKIN) != 0; }
    RfUpdate parts_morph() const { return morph(parts->morph_weight, parts->n_targets, parts_morph_then_skin() ? parts->bone_m3x4 : nullptr, parts->n_bones); }
};
using Source = RfUpdate::Source;
static mcpt_status rf_update(mcpt_ctx* ctx, const RfUpdate& u, const char* fn, const mcpt_camera* cm, const mcpt_reproject_opts* opts, bool reproject);
// The bones of a checked update into the pinned stage of the context's skinning mode: the 3x4 matrices as they are (§18), or one unit dual
// quaternion per bone (§21).
static mcpt_status sk_stage(mcpt_ctx* ctx, const double* bones) {
    mcpt_ctx::Skin& sk = ctx->sk;
    HIP_TRY(sk.bone_stage().wait());
    if (!sk.dq()) std::memcpy(sk.stage.host, bones, sk.table.bytes);
    else for (uint32_t b = 0; b < sk.n_bones; b++) sk_bone_dualquat(bones + 12 * size_t(b), sk.dq_stage.host + SK_DQ_RECORD * size_t(b));
    return MCPT_OK;
}
// The staged table to the device, in stream order.
static hipError_t sk_send_bones(mcpt_ctx::Skin& sk, hipStream_t s) { return sk.bone_stage().send(sk.bone_table().p, 0, sk.bone_table().count(), s); }
// Where a deformer writes: the context's current arrays (rf_current: every single-route call) or the scratch pair of a parts update (§23).
struct RfDest { double* vtx; double* nrm; };
static RfDest rf_current(mcpt_ctx* ctx) { return RfDest{ctx->rf_vtx.p, ctx->rf_nrm.p}; }
// The two skinning kernels of the context's mode: `to` from the given rest pose.
static mcpt_status sk_launch(mcpt_ctx* ctx, const double* rest_vtx, const double* rest_nrm, RfDest to, hipStream_t s) {
    mcpt_ctx::Skin& sk = ctx->sk; const double* table = sk.bone_table().p;
    HIP_TRY((sk.dq() ? launch_sk_dq_vertices : launch_sk_vertices)(rest_vtx, sk.vbone.p, sk.vweight.p, table, to.vtx, ctx->rf_n_vertex, s));
    HIP_TRY((sk.dq() ? launch_sk_dq_normals : launch_sk_normals)(rest_nrm, sk.nbone.p, sk.nweight.p, table, to.nrm, ctx->rf_n_normal, s));
    return MCPT_OK;
}
// Per source the two halves of an update.  *_stage: the caller's values into the pinned stage once the last copy out of it has been made -- host
// work and waits only.  *_enqueue: the stage's copy and the kernels that write `to` (rf_vtx / rf_nrm, or §23's scratch pair) on `s`, inside the
// record's watch, and counted.
static mcpt_status rf_stage_arrays(mcpt_ctx* ctx, const RfUpdate& u) {
    HIP_TRY(ctx->rf_stage.wait());
    std::memcpy(ctx->rf_stage.host, u.vertex, ctx->rf_vtx.bytes);
    if (u.normal) std::memcpy(ctx->rf_stage.host + ctx->rf_vtx.count(), u.normal, ctx->rf_nrm.bytes);   // the caller's normals are copied too
    return MCPT_OK;
}
static mcpt_status rf_enqueue_arrays(mcpt_ctx* ctx, const RfUpdate& u, hipStream_t s) {
    HIP_TRY(ctx->rf_stage.send(ctx->rf_vtx.p, 0, ctx->rf_vtx.count(), s, !u.normal));
    if (u.normal) HIP_TRY(ctx->rf_stage.send(ctx->rf_nrm.p, ctx->rf_vtx.count(), ctx->rf_nrm.count(), s));
    return MCPT_OK;
}
static mcpt_status xf_stage(mcpt_ctx* ctx, const RfUpdate& u) {
    HIP_TRY(ctx->xf.stage.wait());
    for (uint32_t g = 0; g < ctx->xf.n_groups; g++) xf_group_record(u.m3x4 + 12 * size_t(g), ctx->xf.stage.host + XF_RECORD * size_t(g));
    return MCPT_OK;
}
static mcpt_status xf_enqueue(mcpt_ctx* ctx, hipStream_t s, RfDest to) {
    HIP_TRY(ctx->xf.watch.begin(s));
    HIP_TRY(ctx->xf.stage.send(ctx->xf.table.p, 0, ctx->xf.table.count(), s));
    HIP_TRY(launch_xf_vertices(ctx->xf.rest.vtx.p, ctx->xf.vgroup.p, ctx->xf.table.p, to.vtx, ctx->rf_n_vertex, s));
    HIP_TRY(launch_xf_normals(ctx->xf.rest.nrm.p, ctx->xf.ngroup.p, ctx->xf.table.p, to.nrm, ctx->rf_n_normal, s));
    HIP_TRY(ctx->xf.watch.end(s));
    ctx->xf.updates++;
    return MCPT_OK;
}
static mcpt_status sk_enqueue(mcpt_ctx* ctx, hipStream_t s, RfDest to) {
    HIP_TRY(ctx->sk.watch.begin(s));
    HIP_TRY(sk_send_bones(ctx->sk, s));
    const mcpt_status st = sk_launch(ctx, ctx->sk.rest.vtx.p, ctx->sk.rest.nrm.p, to, s); if (st != MCPT_OK) return st;   // in the context's skinning mode (§21)
    HIP_TRY(ctx->sk.watch.end(s));
    ctx->sk.updates++;
    return MCPT_OK;
}
static mcpt_status mo_stage(mcpt_ctx* ctx, const RfUpdate& u) {
    HIP_TRY(ctx->mo.stage.wait());
    std::memcpy(ctx->mo.stage.host, u.weight, ctx->mo.weight.bytes);
    return u.source == Source::MorphSkin ? sk_stage(ctx, u.m3x4) : MCPT_OK;
}
// `send_bones`: false when the table of this call's bones is on its way already (§23: the skin route of the same parts update sent it).
static mcpt_status mo_enqueue(mcpt_ctx* ctx, const RfUpdate& u, hipStream_t s, RfDest to, bool send_bones = true) {
    const bool skin = u.source == Source::MorphSkin;                             // morph, then skin: the morphed arrays are the skin kernels' rest pose
    double* const mv = skin ? ctx->mo.tmp.vtx.p : to.vtx; double* const mn = skin ? ctx->mo.tmp.nrm.p : to.nrm;
    HIP_TRY(ctx->mo.watch.begin(s));
    HIP_TRY(ctx->mo.stage.send(ctx->mo.weight.p, 0, ctx->mo.weight.count(), s));
    if (skin && send_bones) HIP_TRY(sk_send_bones(ctx->sk, s));
    HIP_TRY(launch_mo_vertices(ctx->mo.rest.vtx.p, ctx->mo.voffset.p, ctx->mo.ventry.p, ctx->mo.weight.p, mv, ctx->rf_n_vertex, s));
    HIP_TRY(launch_mo_normals(ctx->mo.rest.nrm.p, ctx->mo.noffset.p, ctx->mo.nentry.p, ctx->mo.weight.p, mn, ctx->rf_n_normal, s));
    if (skin) {
        const mcpt_status st = sk_launch(ctx, mv, mn, to, s); if (st != MCPT_OK) return st;   // in the context's skinning mode (§21)
        ctx->sk.updates++;
    }
    HIP_TRY(ctx->mo.watch.end(s));
    ctx->mo.updates++;
    return MCPT_OK;
}
// Keyframes stage nothing: the time becomes a segment, tap indices and weights on the host, and those are kernel arguments.  On a keyframe
// (u == 0) the frame is copied as it is; without normal frames every call writes the normals captured at set-up.
static mcpt_status kf_enqueue(mcpt_ctx* ctx, const RfUpdate& u, hipStream_t s, RfDest to) {
    mcpt_ctx::Keyframes& kf = ctx->kf;
    KfBlend b = kf_segment(u.time, kf.start_time, kf.frame_time, kf.n_frames, kf.interpolation, kf.wrap);
    kf_weights(b.u, kf.interpolation, b.w);
    const size_t sv = kf_stride(ctx->rf_n_vertex), sn = kf_stride(ctx->rf_n_normal);
    HIP_TRY(kf.watch.begin(s));
    if (b.u == 0.0) {
        if (ctx->rf_vtx.bytes) HIP_TRY(hipMemcpyAsync(to.vtx, kf.vframes.p + sv * b.k, ctx->rf_vtx.bytes, hipMemcpyDeviceToDevice, s));
    } else HIP_TRY(launch_kf_vertices(kf.vframes.p, sv, b, to.vtx, ctx->rf_n_vertex, s));
    if (!kf.normal_frames() || b.u == 0.0) {
        const double* from = kf.normal_frames() ? kf.nframes.p + sn * b.k : kf.rest.nrm.p;
        if (ctx->rf_nrm.bytes) HIP_TRY(hipMemcpyAsync(to.nrm, from, ctx->rf_nrm.bytes, hipMemcpyDeviceToDevice, s));
    } else HIP_TRY(launch_kf_normals(kf.nframes.p, sn, b, to.nrm, ctx->rf_n_normal, s));
    HIP_TRY(kf.watch.end(s));
    kf.updates++; kf.last_frame = b.k; kf.last_u = b.u; kf.last_time = u.time;
    return MCPT_OK;
}
// mcpt_update_parts' rules (§23), host only, in the documented order: the record itself, the owners, the plan of `routes` / `flags`, then per
// route that runs, in id order, that route's own check with its payload.
static mcpt_status pt_check_update(const mcpt_ctx* ctx, const mcpt_scene_update* p, const char* fn) {
    const std::string who = std::string(fn) + ": ";
    if (!p) return fail(MCPT_ERR_INVALID_ARG, who + "null update");
    if (p->struct_size != sizeof(mcpt_scene_update)) return fail(MCPT_ERR_INVALID_ARG, who + "update->struct_size != sizeof(mcpt_scene_update)");
    if (!ctx->pt.set) return fail(MCPT_ERR_INVALID_ARG, who + "no owners are set (mcpt_set_vertex_owners)");
    PtPlan plan;
    switch (pt_plan(p->routes, p->flags, plan)) {
    case PT_PLAN_OK: break;
    case PT_PLAN_NO_ROUTE: return fail(MCPT_ERR_INVALID_ARG, who + "routes names no route");
    case PT_PLAN_UNKNOWN_ROUTE: return fail(MCPT_ERR_INVALID_ARG, who + "routes has an unknown bit");
    case PT_PLAN_UNKNOWN_FLAG: return fail(MCPT_ERR_INVALID_ARG, who + "flags has an unknown bit");
    case PT_PLAN_SKIN_WITHOUT_MORPH: return fail(MCPT_ERR_INVALID_ARG, who + "MCPT_PARTS_MORPH_THEN_SKIN without MCPT_ROUTE_MORPH");
    }
    for (uint32_t k = 0; k < plan.n_steps; k++) {
        mcpt_status st = MCPT_OK;
        switch (plan.step[k]) {
        case MCPT_OWNER_GROUPS: st = xf_check_update(ctx, p->group_m3x4, p->n_groups, fn); break;
        case MCPT_OWNER_SKIN: st = sk_check_update(ctx, p->bone_m3x4, p->n_bones, fn); break;
        case MCPT_OWNER_MORPH:
            st = mo_check_update(ctx, p->morph_weight, p->n_targets, plan.morph_then_skin ? p->bone_m3x4 : nullptr, p->n_bones, fn);
            if (st == MCPT_OK && plan.morph_then_skin && !p->bone_m3x4) st = sk_check_update(ctx, nullptr, p->n_bones, fn);   // (mo_check_update reads null bones as "the morph alone")
            break;
        case MCPT_OWNER_KEYFRAMES: st = kf_check_update(ctx, p->time, fn); break;
        }
        if (st != MCPT_OK) return st;
    }
    return MCPT_OK;
}
// The two halves of a checked parts update.  Staging: every route's own, the bones once for the skin route and the skin behind the morph.
static mcpt_status pt_stage(mcpt_ctx* ctx, const RfUpdate& u) {
    const mcpt_scene_update& p = *u.parts;
    PtPlan plan; (void)pt_plan(p.routes, p.flags, plan);
    mcpt_status st = MCPT_OK;
    if (p.routes & MCPT_ROUTE_GROUPS) { st = xf_stage(ctx, RfUpdate::groups(p.group_m3x4, p.n_groups)); if (st != MCPT_OK) return st; }
    if (plan.bones) { st = sk_stage(ctx, p.bone_m3x4); if (st != MCPT_OK) return st; }
    if (p.routes & MCPT_ROUTE_MORPH) st = mo_stage(ctx, RfUpdate::morph(p.morph_weight, p.n_targets, nullptr, 0));   // (the weights alone: the bones are staged)
    return st;
}
// Route after route in id order on `s`: the route's own enqueue into the scratch pair, then from there the records it owns into rf_vtx / rf_nrm.
// The scratch pair is reused in stream order; the morph-then-skin scratch (mo.tmp) is another buffer, because that route uses both.
static mcpt_status pt_enqueue(mcpt_ctx* ctx, const RfUpdate& u, hipStream_t s) {
    const mcpt_scene_update& p = *u.parts; mcpt_ctx::Parts& pt = ctx->pt;
    PtPlan plan; (void)pt_plan(p.routes, p.flags, plan);
    const RfDest tmp{pt.tmp.vtx.p, pt.tmp.nrm.p};
    bool bones_sent = false;
    HIP_TRY(pt.watch.begin(s));
    for (uint32_t k = 0; k < plan.n_steps; k++) {
        const uint32_t id = plan.step[k];
        mcpt_status st = MCPT_OK;
        switch (id) {
        case MCPT_OWNER_GROUPS: st = xf_enqueue(ctx, s, tmp); break;
        case MCPT_OWNER_SKIN: st = sk_enqueue(ctx, s, tmp); bones_sent = true; break;
        case MCPT_OWNER_MORPH: st = mo_enqueue(ctx, u.parts_morph(), s, tmp, !bones_sent); break;
        case MCPT_OWNER_KEYFRAMES: st = kf_enqueue(ctx, RfUpdate::keyframes(p.time), s, tmp); break;
        }
        if (st != MCPT_OK) return st;
        HIP_TRY(launch_pt_select(tmp.vtx, ctx->rf_vtx.p, pt.vowner.p, id, ctx->rf_n_vertex, s));
        HIP_TRY(launch_pt_select(tmp.nrm, ctx->rf_nrm.p, pt.nowner.p, id, ctx->rf_n_normal, s));
    }
    HIP_TRY(pt.watch.end(s));
    pt.updates++; pt.last_routes = p.routes;
    return MCPT_OK;
}
// Does the refit read rf_nrm, i.e. are there new normals?  `upload_normal`: the arrays' route got normals from the caller.
//     source                            auto normals    the refit reads rf_nrm
//     Groups, Skin, Morph, MorphSkin,
//     Keyframes, Parts                  off or on       nd != 0   (a deformer rewrites rf_nrm whenever the scene has normals)
//     Arrays, None                      on              nd != 0   (so does the normals pass, §20)
//     Arrays, None                      off             upload_normal   (None uploads nothing: no; mcpt_update_normals refuses it before)
static bool rf_reads_normals(Source source, size_t nd, bool auto_normals, bool upload_normal) {
    const bool deformer = source != Source::Arrays && source != Source::None;
    return deformer || auto_normals ? nd != 0 : upload_normal;
}
// The update itself: the new vertices and normals reach rf_vtx / rf_nrm -- arrays staged and copied, or the staged table applied to the source's
// rest pose on the device --, with auto normals on the chosen normal records are recomputed from them (§20), and both trees are refitted, all on the
// context's stream.  The order is fixed: all host staging and its waits; then, inside rf_watch, the source's stream work, the normals pass, the refit.
static mcpt_status rf_enqueue_update(mcpt_ctx* ctx, const RfUpdate& u) {
    const bool auto_normals = ctx->nr.mode != MCPT_NORMALS_OFF;                  // §20: the pass below rewrites rf_nrm, so the refit always reads it
    mcpt_status st = MCPT_OK;
    switch (u.source) {
    case Source::Arrays: st = rf_stage_arrays(ctx, u); break;
    case Source::Groups: st = xf_stage(ctx, u); break;
    case Source::Skin: st = sk_stage(ctx, u.m3x4); break;
    case Source::Morph: case Source::MorphSkin: st = mo_stage(ctx, u); break;
    case Source::Keyframes: break;                                               // §22: the time travels as kernel arguments
    case Source::Parts: st = pt_stage(ctx, u); break;
    case Source::None: break;                                                    // §20, mcpt_update_normals: nothing to stage ...
    }
    if (st != MCPT_OK) return st;
    // Everything below is stream work on the context's stream: it starts after every render enqueued so far has finished (the sub-pipelines'
    // streams joined it at the end of their call, known-length jobs included) and the next render's sub-pipelines fork from it after the last
    // kernel here.
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx->rf_watch.begin(s));
    switch (u.source) {
    case Source::Arrays: st = rf_enqueue_arrays(ctx, u, s); break;
    case Source::Groups: st = xf_enqueue(ctx, s, rf_current(ctx)); break;
    case Source::Skin: st = sk_enqueue(ctx, s, rf_current(ctx)); break;
    case Source::Morph: case Source::MorphSkin: st = mo_enqueue(ctx, u, s, rf_current(ctx)); break;
    case Source::Keyframes: st = kf_enqueue(ctx, u, s, rf_current(ctx)); break;
    case Source::Parts: st = pt_enqueue(ctx, u, s); break;
    case Source::None: break;                                                    // ... and nothing to write
    }
    if (st != MCPT_OK) return st;
    if (auto_normals) {                                                          // §20: the chosen records from the faces as they are now, in place
        HIP_TRY(ctx->nr.watch.begin(s));
        HIP_TRY(launch_nr_normals(ctx->rf_vtx.p, ctx->nr.offset.p, ctx->nr.entry.p, ctx->rf_nrm.p, ctx->rf_n_normal, s));
        HIP_TRY(ctx->nr.watch.end(s));
        ctx->nr.updates++;
    }
    const double* d_nrm = rf_reads_normals(u.source, ctx->rf_nrm.count(), auto_normals, u.normal != nullptr) ? ctx->rf_nrm.p : nullptr;
    const DevScene& d = ctx->dev;
    HIP_TRY(launch_rf_triangles(ctx->rf_vtx.p, d_nrm, ctx->rf_idx.p, RfCentre{d.centre[0], d.centre[1], d.centre[2]}, ctx->tri_isect.p, ctx->tri_shade.p,
                                ctx->tri_pos64.p, ctx->rf_tri_box.p, uint32_t(d.n_tris), s));
    // §24: the mask is sticky -- rf_triangles_kernel has just made every face hittable again, so whatever the route, the hidden ones lose their edges
    // and shrink to a point before the light records and the trees are derived from the streams.  A call that changed the mask (u.lights) also
    // rebuilds the light list, by the material update's chain (§15) with the mask as a second membership test.  No mask, no launch.
    const bool hide = ctx->vs.set && ctx->vs.n_hidden != 0;
    if (hide || u.lights) {
        mcpt_ctx::Visibility& vs = ctx->vs; const uint32_t nt = uint32_t(d.n_tris);
        HIP_TRY(vs.watch.begin(s));
        if (hide) HIP_TRY(launch_vs_hide(vs.mask.p, d.tri_face, ctx->tri_isect.p, ctx->rf_tri_box.p, nt, s));
        if (u.lights) {
            HIP_TRY(launch_mt_classes(ctx->tri_isect.p, d.tri_shade, d.tri_face, d.mats, uint32_t(d.n_mats), ctx->mt_flag.p, nt, s, vs.dev_mask()));
            HIP_TRY(launch_mt_scan(ctx->mt_flag.p, ctx->mt_sums.p, nt, s));
            HIP_TRY(launch_mt_emit(d.tri_isect, d.tri_shade, d.tri_pos64, d.tri_face, d.mats, uint32_t(d.n_mats), ctx->mt_flag.p, ctx->lights.p, ctx->light_pos64.p,
                                   uint32_t(ctx->lights.count()), nt, s, vs.dev_mask()));
            ctx->dev.n_lights = int32_t(u.n_lights); ctx->info.n_lights = u.n_lights;
            vs.updates++;
        }
        HIP_TRY(vs.watch.end(s));
    }
    ctx->vs.box_valid = true;
    HIP_TRY(launch_rf_lights(ctx->lights.p, ctx->light_pos64.p, d.tri_isect, d.tri_pos64, d_nrm, ctx->rf_idx.p, uint32_t(d.n_lights), s));
    for (size_t k = 0; k + 1 < ctx->rf_bin_level.size(); k++)                    // heights, lowest first
        HIP_TRY(launch_rf_binary_level(ctx->nodes.p, ctx->rf_bin_order.p, ctx->rf_bin_level[k], ctx->rf_bin_level[k + 1], ctx->rf_tri_box.p, s));
    for (size_t k = ctx->rf_wide_level.size() - 1; k-- > 0;)                     // depths, deepest first
        HIP_TRY(launch_rf_wide_level(ctx->nodes8.p, ctx->rf_wide_level[k], ctx->rf_wide_level[k + 1], ctx->rf_tri_box.p, ctx->rf_node_box.p, s));
    HIP_TRY(launch_rf_wide_area(d.nodes8, uint32_t(d.n_nodes8), ctx->rf_area.p, s));
    HIP_TRY(ctx->rf_watch.end(s));
    ctx->rf_updates++;
    rf_forget_derived(ctx);
    return MCPT_OK;
}

mcpt_status mcpt_update_vertices(mcpt_ctx* ctx, const double* vertex, uint32_t n_vertex, const double* normal, uint32_t n_normal) {
    return rf_update(ctx, RfUpdate::arrays(vertex, n_vertex, normal, n_normal), "mcpt_update_vertices", nullptr, nullptr, false);
}

// ------------------------------------------------------------------------------------------------ rigid parts
mcpt_status mcpt_set_vertex_groups(mcpt_ctx* ctx, const uint32_t* vertex_group, uint32_t n_vertex, const uint32_t* normal_group, uint32_t n_normal, uint32_t n_groups) {
    const std::string who = "mcpt_set_vertex_groups: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    if (n_vertex != ctx->rf_n_vertex || n_normal != ctx->rf_n_normal) return fail(MCPT_ERR_INVALID_ARG, who + "n_vertex / n_normal differ from the scene's");
    if (!vertex_group || (n_normal && !normal_group)) return fail(MCPT_ERR_INVALID_ARG, who + "null group array");
    if (n_groups < 1 || uint64_t(n_groups) > uint64_t(n_vertex) + n_normal) return fail(MCPT_ERR_INVALID_ARG, who + "n_groups must be in [1, n_vertex + n_normal]");
    for (uint32_t v = 0; v < n_vertex; v++) if (vertex_group[v] >= n_groups) return fail(MCPT_ERR_INVALID_ARG, who + "vertex " + std::to_string(v) + ": group id >= n_groups");
    for (uint32_t v = 0; v < n_normal; v++) if (normal_group[v] >= n_groups) return fail(MCPT_ERR_INVALID_ARG, who + "normal " + std::to_string(v) + ": group id >= n_groups");
    return rf_capture_rest(ctx, ctx->xf.rest, [&] { return ctx->xf.alloc(ctx, n_groups); },
        [&](Scratch& s) -> mcpt_status { HIP_TRY(s.put(ctx->xf.vgroup.p, vertex_group, n_vertex)); HIP_TRY(s.put(ctx->xf.ngroup.p, normal_group, n_normal)); return MCPT_OK; },
        [&](uint32_t v, double far) { double& r = ctx->xf.radius[vertex_group[v]]; r = std::max(r, far); });       // R_g: per group
}

mcpt_status mcpt_update_transforms(mcpt_ctx* ctx, const double* m3x4, uint32_t n_groups) {
    return rf_update(ctx, RfUpdate::groups(m3x4, n_groups), "mcpt_update_transforms", nullptr, nullptr, false);
}

mcpt_status mcpt_get_transform_info(mcpt_ctx* ctx, mcpt_transform_info* out) {
    const mcpt_status st = info_begin(ctx, out, ctx ? &ctx->xf.watch : nullptr); if (st != MCPT_OK) return st;
    out->n_groups = ctx->xf.n_groups; out->updates = ctx->xf.updates; out->last_ms = ctx->xf.watch.last_ms;
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ linear-blend skinning
// One array of influence records (SK_INFLUENCES ids and weights each) against mcpt_set_vertex_skin's rules; `what` names the record in the message.
static mcpt_status sk_check_records(const uint32_t* bone, const double* weight, uint32_t n, uint32_t n_bones, const std::string& who, const char* what) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* b = bone + SK_INFLUENCES * size_t(i); const double* w = weight + SK_INFLUENCES * size_t(i);
        const std::string rec = who + what + " " + std::to_string(i);
        for (int k = 0; k < SK_INFLUENCES; k++) {
            if (b[k] >= n_bones) return fail(MCPT_ERR_INVALID_ARG, rec + ": bone id >= n_bones");
            if (!(w[k] >= 0.0 && w[k] <= 1.0)) return fail(MCPT_ERR_INVALID_ARG, rec + ": a weight is not finite or outside [0, 1]");
        }
        const double sum = ((w[0] + w[1]) + w[2]) + w[3];
        if (!(std::fabs(sum - 1.0) <= 1e-6)) return fail(MCPT_ERR_INVALID_ARG, rec + ": the weights do not sum to 1 within 1e-6");
    }
    return MCPT_OK;
}

mcpt_status mcpt_set_vertex_skin(mcpt_ctx* ctx, const uint32_t* vertex_bone, const double* vertex_weight, uint32_t n_vertex, const uint32_t* normal_bone,
                                 const double* normal_weight, uint32_t n_normal, uint32_t n_bones) {
    const std::string who = "mcpt_set_vertex_skin: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    if (n_vertex != ctx->rf_n_vertex || n_normal != ctx->rf_n_normal) return fail(MCPT_ERR_INVALID_ARG, who + "n_vertex / n_normal differ from the scene's");
    if (!vertex_bone || !vertex_weight || (n_normal && (!normal_bone || !normal_weight))) return fail(MCPT_ERR_INVALID_ARG, who + "null bone or weight array");
    if (n_bones < 1 || uint64_t(n_bones) > SK_INFLUENCES * (uint64_t(n_vertex) + n_normal)) return fail(MCPT_ERR_INVALID_ARG, who + "n_bones must be in [1, 4 (n_vertex + n_normal)]");
    st = sk_check_records(vertex_bone, vertex_weight, n_vertex, n_bones, who, "vertex"); if (st != MCPT_OK) return st;
    st = sk_check_records(normal_bone, normal_weight, n_normal, n_bones, who, "normal"); if (st != MCPT_OK) return st;
    mcpt_ctx::Skin& sk = ctx->sk;
    return rf_capture_rest(ctx, sk.rest, [&] { return sk.alloc(ctx, n_bones); },
        [&](Scratch& s) -> mcpt_status {
            HIP_TRY(s.put(sk.vbone.p, vertex_bone, sk.vbone.count())); HIP_TRY(s.put(sk.vweight.p, vertex_weight, sk.vweight.count()));
            HIP_TRY(s.put(sk.nbone.p, normal_bone, sk.nbone.count())); HIP_TRY(s.put(sk.nweight.p, normal_weight, sk.nweight.count()));
            return MCPT_OK; },
        [&](uint32_t v, double far) {                                            // R_b: per bone that the vertex gives a weight > 0
            for (int k = 0; k < SK_INFLUENCES; k++)
                if (vertex_weight[SK_INFLUENCES * size_t(v) + k] > 0.0) { double& r = sk.radius[vertex_bone[SK_INFLUENCES * size_t(v) + k]]; r = std::max(r, far); }
        });
}

mcpt_status mcpt_update_skin(mcpt_ctx* ctx, const double* m3x4, uint32_t n_bones) {
    return rf_update(ctx, RfUpdate::skin(m3x4, n_bones), "mcpt_update_skin", nullptr, nullptr, false);
}

// ------------------------------------------------------------------------------------------------ dual-quaternion skinning
mcpt_status mcpt_set_skin_mode(mcpt_ctx* ctx, uint32_t mode) {
    const std::string who = "mcpt_set_skin_mode: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    if (mode != MCPT_SKIN_LINEAR && mode != MCPT_SKIN_DUAL_QUATERNION) return fail(MCPT_ERR_INVALID_ARG, who + "unknown mode");
    HIP_TRY(hipStreamSynchronize(ctx->stream));                                  // no kernel reads the table and no copy out of its stage is under way
    st = resolve_timing(ctx); if (st != MCPT_OK) return st;
    if (mode == ctx->sk.mode) return MCPT_OK;
    if (mode == MCPT_SKIN_DUAL_QUATERNION && ctx->sk.n_bones) {                  // the table exists while the mode AND a skin are known; all or none
        const size_t nq = size_t(ctx->sk.n_bones) * SK_DQ_RECORD;
        HIP_TRY(alloc_all(Want(ctx->sk.dq_table, nq, &ctx->info.device_bytes), Want(ctx->sk.dq_stage, nq)));
    } else if (mode == MCPT_SKIN_LINEAR) {
        ctx->sk.dq_table.release(); ctx->sk.dq_stage = Staging<double>{};
    }
    ctx->sk.mode = mode;
    return MCPT_OK;
}

mcpt_status mcpt_get_skin_mode(mcpt_ctx* ctx, uint32_t* out_mode) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out_mode) return fail(MCPT_ERR_INVALID_ARG, "mcpt_get_skin_mode: null output");
    *out_mode = ctx->sk.mode;
    return MCPT_OK;
}

mcpt_status mcpt_get_skin_info(mcpt_ctx* ctx, mcpt_skin_info* out) {
    const mcpt_status st = info_begin(ctx, out, ctx ? &ctx->sk.watch : nullptr); if (st != MCPT_OK) return st;
    out->n_bones = ctx->sk.n_bones; out->updates = ctx->sk.updates; out->last_ms = ctx->sk.watch.last_ms;
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ morph targets
// One set of targets against mcpt_set_vertex_morph's rules; `what` names the array in the message.  (null: no targets for this array.)
static mcpt_status mo_check_targets(const mcpt_morph_targets* t, uint32_t n_records, uint32_t n_targets, const std::string& who, const char* what) {
    if (!t) return MCPT_OK;
    const std::string set = who + what + " targets: ";
    if (t->struct_size != sizeof(mcpt_morph_targets)) return fail(MCPT_ERR_INVALID_ARG, set + "struct_size != sizeof(mcpt_morph_targets)");
    if (t->n_targets < 1 || t->n_targets > 65536) return fail(MCPT_ERR_INVALID_ARG, set + "n_targets must be in [1, 65536]");
    if (t->n_targets != n_targets) return fail(MCPT_ERR_INVALID_ARG, set + "n_targets differs from the vertex targets' (one weight drives both)");
    if (!t->target_offset) return fail(MCPT_ERR_INVALID_ARG, set + "null target_offset");
    if (t->target_offset[0] != 0) return fail(MCPT_ERR_INVALID_ARG, set + "target_offset[0] is not 0");
    for (uint32_t k = 0; k < n_targets; k++)
        if (t->target_offset[k + 1] < t->target_offset[k]) return fail(MCPT_ERR_INVALID_ARG, set + "target_offset decreases at target " + std::to_string(k));
    const uint32_t total = t->target_offset[n_targets];
    if (total && (!t->index || !t->delta)) return fail(MCPT_ERR_INVALID_ARG, set + "null index or delta array");
    for (uint32_t k = 0; k < n_targets; k++)
        for (uint32_t e = t->target_offset[k]; e < t->target_offset[k + 1]; e++) {
            const std::string at = set + "target " + std::to_string(k) + ", entry " + std::to_string(e);
            if (t->index[e] >= n_records) return fail(MCPT_ERR_INVALID_ARG, at + ": index >= the record count");
            if (e > t->target_offset[k] && t->index[e] <= t->index[e - 1]) return fail(MCPT_ERR_INVALID_ARG, at + ": indices are not strictly ascending inside the target");
            const double* d = t->delta + 3 * size_t(e);
            if (!(std::fabs(d[0]) <= MCPT_MAX_COORD && std::fabs(d[1]) <= MCPT_MAX_COORD && std::fabs(d[2]) <= MCPT_MAX_COORD))
                return fail(MCPT_ERR_INVALID_ARG, at + ": a delta component is not finite or exceeds 1e18");
        }
    return MCPT_OK;
}

mcpt_status mcpt_set_vertex_morph(mcpt_ctx* ctx, const mcpt_morph_targets* vertex, uint32_t n_vertex, const mcpt_morph_targets* normal, uint32_t n_normal) {
    const std::string who = "mcpt_set_vertex_morph: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    if (n_vertex != ctx->rf_n_vertex || n_normal != ctx->rf_n_normal) return fail(MCPT_ERR_INVALID_ARG, who + "n_vertex / n_normal differ from the scene's");
    if (!vertex) return fail(MCPT_ERR_INVALID_ARG, who + "null vertex targets");
    st = mo_check_targets(vertex, n_vertex, vertex->n_targets, who, "vertex"); if (st != MCPT_OK) return st;
    st = mo_check_targets(normal, n_normal, vertex->n_targets, who, "normal"); if (st != MCPT_OK) return st;
    const uint32_t n_targets = vertex->n_targets;
    std::vector<uint32_t> voff, noff; std::vector<MoEntry> vent, nent;
    mo_per_record(vertex->target_offset, vertex->index, vertex->delta, n_targets, n_vertex, voff, vent);
    if (normal) mo_per_record(normal->target_offset, normal->index, normal->delta, n_targets, n_normal, noff, nent);
    else noff.assign(size_t(n_normal) + 1, 0);                                   // normals are not morphed: every list is empty, every record is copied
    mcpt_ctx::Morph& mo = ctx->mo;
    st = rf_capture_rest(ctx, mo.rest, [&] { return mo.alloc(ctx, n_targets, vent.size(), nent.size()); },
        [&](Scratch& s) -> mcpt_status {
            HIP_TRY(s.put(mo.voffset.p, voff.data(), voff.size())); HIP_TRY(s.put(mo.noffset.p, noff.data(), noff.size()));
            HIP_TRY(s.put(mo.ventry.p, vent.data(), vent.size())); HIP_TRY(s.put(mo.nentry.p, nent.data(), nent.size()));
            return MCPT_OK; },
        [&](uint32_t, double far) { mo.radius = std::max(mo.radius, far); });    // R: global; D_k below: per target
    if (st != MCPT_OK) return st;
    for (uint32_t k = 0; k < n_targets; k++)
        for (uint32_t e = vertex->target_offset[k]; e < vertex->target_offset[k + 1]; e++) {
            if (!ctx->rf_used_vertex[vertex->index[e]]) continue;
            for (int a = 0; a < 3; a++) mo.delta[k] = std::max(mo.delta[k], std::fabs(vertex->delta[3 * size_t(e) + a]));
        }
    return MCPT_OK;
}

mcpt_status mcpt_update_morph(mcpt_ctx* ctx, const double* weight, uint32_t n_targets, const double* bones_m3x4, uint32_t n_bones) {
    return rf_update(ctx, RfUpdate::morph(weight, n_targets, bones_m3x4, n_bones), "mcpt_update_morph", nullptr, nullptr, false);
}

mcpt_status mcpt_get_morph_info(mcpt_ctx* ctx, mcpt_morph_info* out) {
    const mcpt_status st = info_begin(ctx, out, ctx ? &ctx->mo.watch : nullptr); if (st != MCPT_OK) return st;
    out->n_targets = ctx->mo.n_targets; out->updates = ctx->mo.updates; out->last_ms = ctx->mo.watch.last_ms;
    out->vertex_entries = ctx->mo.ventry.count(); out->normal_entries = ctx->mo.nentry.count();
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ keyframe playback
mcpt_status mcpt_set_vertex_keyframes(mcpt_ctx* ctx, const double* vertex_frames, uint32_t n_vertex, const double* normal_frames, uint32_t n_normal, uint32_t n_frames,
                                      const mcpt_keyframe_opts* opts) {
    const char* const fn = "mcpt_set_vertex_keyframes";
    const std::string who = std::string(fn) + ": ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    if (!vertex_frames) return fail(MCPT_ERR_INVALID_ARG, who + "null vertex frames");
    if (n_vertex != ctx->rf_n_vertex || n_normal != ctx->rf_n_normal) return fail(MCPT_ERR_INVALID_ARG, who + "n_vertex / n_normal differ from the scene's");
    mcpt_keyframe_opts o;
    st = read_opts(opts, o, fn, "mcpt_keyframe_opts"); if (st != MCPT_OK) return st;
    if (!opts) o.frame_time = 1.0;                                               // (linear, clamp and start 0 are the zeros read_opts left)
    if (o.interpolation != MCPT_KEYFRAMES_LINEAR && o.interpolation != MCPT_KEYFRAMES_CATMULL_ROM) return fail(MCPT_ERR_INVALID_ARG, who + "unknown interpolation");
    if (o.wrap != MCPT_KEYFRAMES_CLAMP && o.wrap != MCPT_KEYFRAMES_LOOP) return fail(MCPT_ERR_INVALID_ARG, who + "unknown wrap");
    if (n_frames < 2 || n_frames > MCPT_KEYFRAMES_MAX) return fail(MCPT_ERR_INVALID_ARG, who + "n_frames must be in [2, 65536]");
    if (!std::isfinite(o.start_time)) return fail(MCPT_ERR_INVALID_ARG, who + "start_time is not finite");
    if (!(std::isfinite(o.frame_time) && o.frame_time > 0.0)) return fail(MCPT_ERR_INVALID_ARG, who + "frame_time is not finite or not > 0");
    double radius = 0.0;                                                         // R: over the vertices a face uses, all frames
    for (uint32_t k = 0; k < n_frames; k++)
        for (uint32_t v = 0; v < n_vertex; v++) {
            if (!ctx->rf_used_vertex[v]) continue;
            const double* x = vertex_frames + 3 * (size_t(k) * n_vertex + v);
            const double far = std::max({std::fabs(x[0]), std::fabs(x[1]), std::fabs(x[2])});
            if (!(std::fabs(x[0]) <= MCPT_MAX_COORD && std::fabs(x[1]) <= MCPT_MAX_COORD && std::fabs(x[2]) <= MCPT_MAX_COORD))
                return fail(MCPT_ERR_INVALID_ARG, who + "frame " + std::to_string(k) + ", vertex " + std::to_string(v) + ": coordinate is not finite or exceeds 1e18");
            radius = std::max(radius, far);
        }
    for (size_t i = 0; normal_frames && i < 3 * size_t(n_frames) * n_normal; i++)
        if (!std::isfinite(normal_frames[i]))
            return fail(MCPT_ERR_INVALID_ARG, who + "frame " + std::to_string(i / (3 * size_t(n_normal))) + ", normal " + std::to_string(i / 3 % n_normal) + ": a component is not finite");
    if (!(kf_reach(radius, o.interpolation) <= MCPT_MAX_COORD)) return fail(MCPT_ERR_INVALID_ARG, who + "an interpolated vertex could leave |coordinate| <= 1e18 (conservative bound)");
    // the frames at their device stride (the padding is 0), one copy per array
    auto padded = [&](const double* frames, uint32_t n) {
        const size_t stride = kf_stride(n), row = 3 * size_t(n);
        std::vector<double> out(stride * n_frames, 0.0);
        for (uint32_t k = 0; k < n_frames; k++) std::copy_n(frames + row * k, row, out.begin() + stride * k);
        return out;
    };
    const bool normals = normal_frames && n_normal;
    const std::vector<double> vf = padded(vertex_frames, n_vertex), nf = normals ? padded(normal_frames, n_normal) : std::vector<double>();
    mcpt_ctx::Keyframes& kf = ctx->kf;
    st = rf_capture_rest(ctx, kf.rest, [&] { return kf.alloc(ctx, n_frames, normals); },
        [&](Scratch& s) -> mcpt_status {
            HIP_TRY(s.put(kf.vframes.p, vf.data(), vf.size())); HIP_TRY(s.put(kf.nframes.p, nf.data(), nf.size()));
            return MCPT_OK; },
        [](uint32_t, double) {});                                                // (R comes from the frames, not from the pose at set-up)
    if (st != MCPT_OK) return st;
    kf.interpolation = o.interpolation; kf.wrap = o.wrap; kf.start_time = o.start_time; kf.frame_time = o.frame_time;
    return MCPT_OK;
}

mcpt_status mcpt_update_keyframes(mcpt_ctx* ctx, double time) {
    return rf_update(ctx, RfUpdate::keyframes(time), "mcpt_update_keyframes", nullptr, nullptr, false);
}

mcpt_status mcpt_get_keyframe_info(mcpt_ctx* ctx, mcpt_keyframe_info* out) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, "mcpt_get_keyframe_info: ")) != MCPT_OK) return st;
    st = info_begin(ctx, out, &ctx->kf.watch); if (st != MCPT_OK) return st;
    const mcpt_ctx::Keyframes& kf = ctx->kf;
    out->n_frames = kf.n_frames; out->interpolation = kf.interpolation; out->wrap = kf.wrap; out->updates = kf.updates; out->last_frame = kf.last_frame;
    out->last_u = kf.last_u; out->last_time = kf.last_time; out->last_ms = kf.watch.last_ms; out->device_bytes = kf.device_bytes();
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ parts update
mcpt_status mcpt_set_vertex_owners(mcpt_ctx* ctx, const uint8_t* vertex_owner, uint32_t n_vertex, const uint8_t* normal_owner, uint32_t n_normal) {
    const std::string who = "mcpt_set_vertex_owners: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    PtCounts counts{}; std::string err;
    if (vertex_owner && !pt_check_owners(vertex_owner, n_vertex, normal_owner, n_normal, ctx->rf_n_vertex, ctx->rf_n_normal, counts, err)) return fail(MCPT_ERR_INVALID_ARG, who + err);
    HIP_TRY(hipStreamSynchronize(ctx->stream));                                  // no kernel reads the old owners or the scratch pair any more
    st = resolve_timing(ctx); if (st != MCPT_OK) return st;
    if (!vertex_owner) { ctx->pt.drop(); return MCPT_OK; }
    st = ctx->pt.alloc(ctx); if (st != MCPT_OK) return st;                       // afresh, all or none: a context that had owners keeps them on failure
    ctx->pt.counts = counts;
    Scratch s(ctx->stream);
    HIP_TRY(s.put(ctx->pt.vowner.p, vertex_owner, n_vertex)); HIP_TRY(s.put(ctx->pt.nowner.p, normal_owner, n_normal)); HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_update_parts(mcpt_ctx* ctx, const mcpt_scene_update* update) {
    return rf_update(ctx, RfUpdate::of_parts(update), "mcpt_update_parts", nullptr, nullptr, false);
}

mcpt_status mcpt_get_parts_info(mcpt_ctx* ctx, mcpt_parts_info* out) {
    const mcpt_status st = info_begin(ctx, out, ctx ? &ctx->pt.watch : nullptr); if (st != MCPT_OK) return st;
    const mcpt_ctx::Parts& pt = ctx->pt;
    out->set = pt.set; out->updates = pt.updates; out->last_routes = pt.last_routes; out->last_ms = pt.watch.last_ms; out->device_bytes = pt.device_bytes();
    for (int k = 0; k < PT_OWNERS; k++) { out->vertex_records[k] = pt.counts.vertex[k]; out->normal_records[k] = pt.counts.normal[k]; }
    return MCPT_OK;
}

mcpt_status mcpt_probe_vertices(mcpt_ctx* ctx, double* out_vertex, double* out_normal) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, "mcpt_probe_vertices: ")) != MCPT_OK) return st;
    st = read_back(ctx, out_vertex, ctx->rf_vtx.p, out_vertex ? ctx->rf_vtx.bytes : 0); if (st != MCPT_OK) return st;
    return read_back(ctx, out_normal, ctx->rf_nrm.p, out_normal ? ctx->rf_nrm.bytes : 0);
}

// ------------------------------------------------------------------------------------------------ automatic normals
mcpt_status mcpt_set_auto_normals(mcpt_ctx* ctx, const uint8_t* normal_mask, uint32_t n_normal, const mcpt_normals_opts* opts) {
    const char* const fn = "mcpt_set_auto_normals";
    const std::string who = std::string(fn) + ": ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    if (n_normal != ctx->rf_n_normal) return fail(MCPT_ERR_INVALID_ARG, who + "n_normal differs from the scene's");
    mcpt_normals_opts o;
    st = read_opts(opts, o, fn, "mcpt_normals_opts"); if (st != MCPT_OK) return st;
    if (!opts) o.mode = MCPT_NORMALS_AREA;
    if (o.mode != MCPT_NORMALS_OFF && o.mode != MCPT_NORMALS_AREA) return fail(MCPT_ERR_INVALID_ARG, who + "unknown mode");
    HIP_TRY(hipStreamSynchronize(ctx->stream));                                  // rf_vtx / rf_nrm are final, and no kernel reads the old lists any more
    st = resolve_timing(ctx); if (st != MCPT_OK) return st;
    if (o.mode == MCPT_NORMALS_OFF) {
        ctx->nr.offset.release(); ctx->nr.entry.release();
        ctx->nr.mode = MCPT_NORMALS_OFF; ctx->nr.records = 0; ctx->nr.max_valence = 0;
        return MCPT_OK;
    }
    // the faces in the description's order, from the leaf-order index arrays and the leaf order itself; the reference pose
    const size_t nt = size_t(ctx->dev.n_tris);
    std::vector<int32_t> idx6(ctx->rf_idx.count()), leaf_face(nt), fv(3 * nt), fnm(3 * nt);
    std::vector<double> vtx(ctx->rf_vtx.count()), nrm(ctx->rf_nrm.count());
    {   Scratch s(ctx->stream);
        HIP_TRY(s.fetch(idx6.data(), ctx->rf_idx.p, idx6.size())); HIP_TRY(s.fetch(leaf_face.data(), ctx->tri_face.p, leaf_face.size()));
        HIP_TRY(s.fetch(vtx.data(), ctx->rf_vtx.p, vtx.size())); HIP_TRY(s.fetch(nrm.data(), ctx->rf_nrm.p, nrm.size())); HIP_TRY(s.finish()); }
    for (size_t i = 0; i < nt; i++) {
        const size_t f = size_t(leaf_face[i]);
        if (f >= nt) return fail(MCPT_ERR_HIP, who + "the context's leaf order is damaged");
        for (int k = 0; k < 3; k++) { fv[3 * f + k] = idx6[6 * i + k]; fnm[3 * f + k] = idx6[6 * i + 3 + k]; }
    }
    std::vector<uint32_t> offset; std::vector<NrEntry> entry;
    const uint32_t max_valence = nr_per_record(fv.data(), fnm.data(), uint32_t(nt), n_normal, normal_mask, vtx.data(), nrm.data(), offset, entry);
    st = ctx->nr.alloc(ctx, entry.size()); if (st != MCPT_OK) return st;
    {   Scratch s(ctx->stream);
        HIP_TRY(s.put(ctx->nr.offset.p, offset.data(), offset.size())); HIP_TRY(s.put(ctx->nr.entry.p, entry.data(), entry.size())); HIP_TRY(s.finish()); }
    ctx->nr.mode = o.mode; ctx->nr.max_valence = max_valence; ctx->nr.records = 0;
    for (uint32_t i = 0; i < n_normal; i++) ctx->nr.records += offset[size_t(i) + 1] > offset[i];
    return MCPT_OK;
}

mcpt_status mcpt_update_normals(mcpt_ctx* ctx) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, "mcpt_update_normals: ")) != MCPT_OK) return st;
    if (ctx->nr.mode == MCPT_NORMALS_OFF) return fail(MCPT_ERR_INVALID_ARG, "mcpt_update_normals: auto normals are not set (mcpt_set_auto_normals)");
    return rf_enqueue_update(ctx, RfUpdate::none());
}

mcpt_status mcpt_get_normals_info(mcpt_ctx* ctx, mcpt_normals_info* out) {
    const mcpt_status st = info_begin(ctx, out, ctx ? &ctx->nr.watch : nullptr); if (st != MCPT_OK) return st;
    out->mode = ctx->nr.mode; out->records = ctx->nr.records; out->max_valence = ctx->nr.max_valence;
    out->entries = ctx->nr.entry.count(); out->updates = ctx->nr.updates; out->last_ms = ctx->nr.watch.last_ms;
    return MCPT_OK;
}

mcpt_status mcpt_get_update_info(mcpt_ctx* ctx, mcpt_update_info* out) {
    mcpt_status st = info_begin(ctx, out, ctx ? &ctx->rf_watch : nullptr); if (st != MCPT_OK) return st;
    out->updates = ctx->rf_updates; out->last_update_ms = ctx->rf_watch.last_ms; out->wide_area_ratio = 1.0;
    if (ctx->rf_updates) {                                                      // the last update left its partial sums behind
        double a = 0.0;
        st = rf_read_area(ctx, a); if (st != MCPT_OK) return st;
        out->wide_area_ratio = ctx->rf_area0 > 0.0 ? a / ctx->rf_area0 : 1.0;
    }
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ tree rebuild
// New trees for the vertices the context holds, everything else kept.  Every step that can fail works on temporaries -- the builders' input and
// output, the new node buffers, the permuted streams, the renumbered lights, the level tables, a larger overflow area -- and the last block swaps
// them in; a refusal returns before it and the temporaries die with their owners (the tally follows them back).
mcpt_status mcpt_rebuild_trees(mcpt_ctx* ctx, const mcpt_rebuild_opts* opts) {
    const std::string who = "mcpt_rebuild_trees: ";
    const auto t_entry = std::chrono::steady_clock::now();
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    mcpt_rebuild_opts o;
    st = read_opts(opts, o, "mcpt_rebuild_trees", "mcpt_rebuild_opts"); if (st != MCPT_OK) return st;
    if (o.builder > MCPT_REBUILD_DEVICE) return fail(MCPT_ERR_INVALID_ARG, who + "unknown builder");
    const bool device_builder = o.builder == MCPT_REBUILD_DEVICE || (o.builder == MCPT_REBUILD_SAME && (ctx->opts.flags & MCPT_FLAG_GPU_BVH_BUILD));
    st = use_drained(ctx); if (st != MCPT_OK) return st;                          // renders enqueued so far have walked the old tree
    HIP_TRY(ctx->rf_watch.settle());
    double area_before = 1.0;
    if (ctx->rf_updates) {
        double a = 0.0;
        st = rf_read_area(ctx, a); if (st != MCPT_OK) return st;
        if (ctx->rf_area0 > 0.0) area_before = a / ctx->rf_area0;
    }
    const uint32_t nt = uint32_t(ctx->dev.n_tris);
    hipStream_t s = ctx->stream;
    st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
    RebuildPlan plan;
    {   // the bounds kernel scatters by the old order: it is a permutation, or nothing is launched
        const std::string bad = rb_plan(ctx->h_tri_face.data(), ctx->h_tri_face.size(), ctx->h_tri_face.data(), ctx->h_tri_face.size(), plan);
        if (!bad.empty() || ctx->h_tri_face.size() != nt) return fail(MCPT_ERR_HIP, who + "the context's leaf order is damaged: " + bad);
    }

    // ---- the builders' input, from rf_vtx, in face order; fetched when a builder asks for it
    Event ev[4];                                                                  // [0, 1] the bounds kernel, [2, 3] the permutation and the lights
    for (Event& e : ev) HIP_TRY(hipEventCreate(e.out()));
    double device_ms = 0.0;
    DevBuf<float> d_box32; DevBuf<double> d_bound64; Pinned<float> h_box32; Pinned<double> h_bound64;
    static_assert(sizeof(BTri) == 9 * sizeof(double), "rb_face_bounds_kernel writes scene_build.h's BTri: lo, hi, centroid");
    std::string err;
    auto bounds = [&](bool want64) -> bool {
        auto hip_ok = [&](hipError_t e, const char* what) { if (e != hipSuccess) err = who + what + ": " + hipGetErrorString(e); return e == hipSuccess; };
        if (!d_box32.p && !(hip_ok(d_box32.alloc(6 * size_t(nt)), "hipMalloc") && hip_ok(hipHostMalloc(h_box32.out(), 6 * size_t(nt) * sizeof(float), hipHostMallocDefault), "hipHostMalloc"))) return false;
        if (want64 && !(hip_ok(d_bound64.alloc(9 * size_t(nt)), "hipMalloc") && hip_ok(hipHostMalloc(h_bound64.out(), 9 * size_t(nt) * sizeof(double), hipHostMallocDefault), "hipHostMalloc"))) return false;
        const DevScene& d = ctx->dev;
        float ms = 0.f;
        return hip_ok(hipEventRecord(ev[0], s), "hipEventRecord") &&
               hip_ok(launch_rb_face_bounds(ctx->rf_vtx.p, ctx->rf_idx.p, ctx->tri_face.p, RfCentre{d.centre[0], d.centre[1], d.centre[2]}, d_box32.p, want64 ? d_bound64.p : nullptr, nt, s), "rb_face_bounds_kernel") &&
               hip_ok(hipEventRecord(ev[1], s), "hipEventRecord") &&
               hip_ok(hipMemcpyAsync(h_box32, d_box32.p, d_box32.bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync") &&
               (!want64 || hip_ok(hipMemcpyAsync(h_bound64, d_bound64.p, d_bound64.bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync")) &&
               hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize") && hip_ok(hipEventElapsedTime(&ms, ev[0], ev[1]), "hipEventElapsedTime") && ((device_ms += ms), true);
    };
    const TreeInput in{nt, [&]() -> const BTri* { return bounds(true) ? reinterpret_cast<const BTri*>(h_bound64.h) : nullptr; },
                       [&]() -> const float* { return bounds(false) ? h_box32.h : nullptr; }};

    // ---- the trees: mcpt_create's path, builders and depth rule
    HostScene hs; std::vector<int> order;
    hs.allow_deep_binary = device_builder && ctx->use_wavefront;
    st = device_builder ? build_trees(in, hs, order, err, device_bvh_builder(), device_collapse8()) : build_trees(in, hs, order, err);
    if (st != MCPT_OK) return fail(st, who + err);
    if (hs.nodes8.size() * sizeof(f4h) >= (1ull << 32)) return fail(MCPT_ERR_UNSUPPORTED, who + "tree too large for the 8-wide traversal kernel");
    {   const std::string bad = rb_plan(ctx->h_tri_face.data(), ctx->h_tri_face.size(), order.data(), order.size(), plan);
        if (!bad.empty()) return fail(MCPT_ERR_HIP, who + "the builder's leaf order is no permutation of the faces: " + bad); }
    std::vector<uint32_t> bin_order, bin_level, wide_level;
    if (!rf_levels(hs.nodes, hs.nodes8, bin_order, bin_level, wide_level, err)) return fail(MCPT_ERR_HIP, who + err);
    // the overflow area follows the NEW wide depth, known here on the host: a deeper tree gets its larger area before any kernel walks it
    size_t ovf_bytes = 0;
    if (ctx->use_wavefront && (st = overflow_bytes(ctx, hs.bvh8_depth, ovf_bytes)) != MCPT_OK) return st;
    std::vector<DevBuf<int>> ovf(ctx->lanes.size());
    for (size_t l = 0; l < ovf.size(); l++) if (ctx->lanes[l].ovf_buf.bytes != ovf_bytes) HIP_TRY(ovf[l].alloc(ovf_bytes / sizeof(int)));

    // ---- new buffers: the nodes uploaded, the streams permuted, the lights renumbered in a copy, the new tree's area
    uint64_t* tally = &ctx->info.device_bytes;
    const size_t n2 = hs.nodes.size() / 4, n8 = hs.nodes8.size() / 5;
    DevBuf<float4> nodes, nodes8, tri_isect, tri_shade; DevBuf<double> tri_pos64, rf_area; DevBuf<int32_t> rf_idx, tri_face; DevBuf<DevLight> lights;
    DevBuf<float> rf_node_box; DevBuf<uint32_t> rf_bin_order, d_src, d_dst;
    HIP_TRY(nodes.alloc(hs.nodes.size(), tally)); HIP_TRY(nodes8.alloc(hs.nodes8.size(), tally)); HIP_TRY(tri_isect.alloc(ctx->tri_isect.count(), tally));
    HIP_TRY(tri_shade.alloc(ctx->tri_shade.count(), tally)); HIP_TRY(tri_pos64.alloc(ctx->tri_pos64.count(), tally)); HIP_TRY(tri_face.alloc(ctx->tri_face.count(), tally));
    HIP_TRY(rf_idx.alloc(ctx->rf_idx.count(), tally)); HIP_TRY(lights.alloc(ctx->lights.count(), tally)); HIP_TRY(rf_node_box.alloc(n8 * 6, tally));
    HIP_TRY(rf_bin_order.alloc(n2, tally)); HIP_TRY(rf_area.alloc(rf_area_blocks(uint32_t(n8)), tally));
    HIP_TRY(d_src.alloc(nt)); HIP_TRY(d_dst.alloc(nt));
    HIP_TRY(hipMemcpyAsync(nodes.p, hs.nodes.data(), nodes.bytes, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(nodes8.p, hs.nodes8.data(), nodes8.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(rf_bin_order.p, bin_order.data(), rf_bin_order.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_src.p, plan.src_of_dst.data(), d_src.bytes, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(d_dst.p, plan.dst_of_src.data(), d_dst.bytes, hipMemcpyHostToDevice, s));
    // §27: bake points name leaves; the list for the new order, from the face-order copy (the bake film is per point and stays)
    DevBuf<BkPoint> bk_pts; std::vector<BkPoint> bk_host;
    if (ctx->bk.n()) {
        std::vector<int32_t> leaf_of_face(nt, -1);
        for (size_t i = 0; i < order.size(); i++) leaf_of_face[size_t(order[i])] = int32_t(i);
        bk_host = ctx->bk.in_leaf_terms(leaf_of_face);
        HIP_TRY(bk_pts.alloc(bk_host.size(), tally));
        HIP_TRY(hipMemcpyAsync(bk_pts.p, bk_host.data(), bk_pts.bytes, hipMemcpyHostToDevice, s));
    }
    // §28: probe positions are relative to the centre; the device list for the centre this call leaves in force, from the world-coordinate copy
    DevBuf<double> sh_pos; std::vector<double> sh_host;
    if (ctx->sh.n()) {
        sh_host = to_local(ctx, ctx->sh.host.data(), ctx->sh.n());
        HIP_TRY(sh_pos.alloc(sh_host.size(), tally));
        HIP_TRY(hipMemcpyAsync(sh_pos.p, sh_host.data(), sh_pos.bytes, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(tri_isect.p + 3 * size_t(nt), 0, 3 * sizeof(float4), s));                     // the spare record
    if (lights.bytes) HIP_TRY(hipMemcpyAsync(lights.p, ctx->lights.p, lights.bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipEventRecord(ev[2], s));
    HIP_TRY(launch_rb_permute(RbStreams{ctx->tri_isect.p, ctx->tri_shade.p, ctx->tri_pos64.p, ctx->rf_idx.p, ctx->tri_face.p},
                              RbStreams{tri_isect.p, tri_shade.p, tri_pos64.p, rf_idx.p, tri_face.p}, d_src.p, nt, (ctx->opts.flags & MCPT_FLAG_REFERENCE_TIE_ORDER) != 0, s));
    HIP_TRY(launch_rb_lights(lights.p, d_dst.p, uint32_t(ctx->dev.n_lights), nt, s));
    HIP_TRY(hipEventRecord(ev[3], s));
    HIP_TRY(launch_rf_wide_area(nodes8.p, uint32_t(n8), rf_area.p, s));
    std::vector<double> part(rf_area.count());
    HIP_TRY(hipMemcpyAsync(part.data(), rf_area.p, rf_area.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                                             // (the host vectors above have been read)
    {   float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3])); device_ms += ms; }
    double area0 = 0.0;
    for (double v : part) area0 += v;

    // ---- commit: moves and assignments only
    ctx->nodes = std::move(nodes); ctx->nodes8 = std::move(nodes8); ctx->tri_isect = std::move(tri_isect); ctx->tri_shade = std::move(tri_shade);
    ctx->tri_pos64 = std::move(tri_pos64); ctx->tri_face = std::move(tri_face); ctx->rf_idx = std::move(rf_idx); ctx->lights = std::move(lights);
    ctx->rf_node_box = std::move(rf_node_box); ctx->rf_bin_order = std::move(rf_bin_order); ctx->rf_area = std::move(rf_area);
    for (size_t l = 0; l < ovf.size(); l++) if (ovf[l].p) ctx->lanes[l].ovf_buf = std::move(ovf[l]);
    ctx->rf_bin_level.swap(bin_level); ctx->rf_wide_level.swap(wide_level); ctx->rf_area0 = area0;
    ctx->h_tri_face.assign(order.begin(), order.end());
    if (bk_pts.p) ctx->bk.pts = std::move(bk_pts);
    if (sh_pos.p) ctx->sh.pos = std::move(sh_pos);
    ctx->wide_depth = hs.bvh8_depth; ctx->binary_ok = hs.binary_ok;
    ctx->vs.box_valid = false;                                                    // §24: rf_tri_box is scratch in the OLD leaf order; the mask is per face and stays
    DevScene& d = ctx->dev;
    d.nodes = ctx->nodes.p; d.nodes8 = ctx->nodes8.p; d.tri_isect = ctx->tri_isect.p; d.tri_shade = ctx->tri_shade.p; d.tri_pos64 = ctx->tri_pos64.p;
    d.tri_face = ctx->tri_face.p; d.lights = ctx->lights.p; d.n_nodes = int32_t(n2); d.n_nodes8 = int32_t(n8);
    mcpt_scene_info& info = ctx->info;
    info.n_nodes = uint32_t(n2); info.bvh_depth = hs.bvh_depth; info.max_leaf = hs.max_leaf; info.bvh_builder = hs.bvh_builder;
    fill_tree_info(info, hs, ctx->h_tri_face.data(), ctx->h_tri_face.size());
    ctx->rb_rebuilds++; ctx->rb_area_before = area_before; ctx->rb_last_build_ms = hs.bvh_build_ms; ctx->rb_last_device_ms = device_ms;
    ctx->rb_last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    return MCPT_OK;
}

mcpt_status mcpt_get_rebuild_info(mcpt_ctx* ctx, mcpt_rebuild_info* out) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    std::memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out; out->rebuilds = ctx->rb_rebuilds; out->last_ms = ctx->rb_last_ms; out->last_build_ms = ctx->rb_last_build_ms;
    out->last_device_ms = ctx->rb_last_device_ms; out->area_ratio_before = ctx->rb_area_before;
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ material edits
// The device records of `mats` over the context's textures, into `out` (n_mats of them).
static void mt_records(const mcpt_ctx* ctx, const std::vector<mcpt_material>& mats, DevMaterial* out) {
    for (size_t i = 0; i < mats.size(); i++) out[i] = device_material(mats[i], ctx->mt_tex[size_t(mats[i].map_kd)]);
}
// What a rebuild of the light list to `n_lights` entries needs on the device: the scan's scratch (allocated once, one word per face and one per
// scan block) and a list that long.  The list only grows, and what it held is NOT kept: the caller rebuilds all of it.
static mcpt_status mt_ensure_list(mcpt_ctx* ctx, uint64_t n_lights) {
    const uint32_t nt = uint32_t(ctx->dev.n_tris);
    uint64_t* tally = &ctx->info.device_bytes;
    if (!ctx->mt_flag.p) HIP_TRY(alloc_all(Want(ctx->mt_flag, nt, tally), Want(ctx->mt_sums, mt_blocks(nt), tally)));
    if (n_lights > ctx->lights.count()) {
        // the list grows (rare): kernels enqueued earlier may still read the old buffers, which die when the new ones replace them
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(alloc_all(Want(ctx->lights, size_t(n_lights), tally), Want(ctx->light_pos64, 9 * size_t(n_lights), tally)));
        ctx->dev.lights = ctx->lights.p; ctx->dev.light_pos64 = ctx->light_pos64.p;
    }
    return MCPT_OK;
}
// `mats` staged and copied over the device records in stream order (`last`: the staging buffer's only copy of this filling).
static mcpt_status mt_send_records(mcpt_ctx* ctx, const std::vector<mcpt_material>& mats) {
    HIP_TRY(ctx->mt_stage.wait());
    HIP_TRY(ctx->mt_stage.grow(mats.size()));
    mt_records(ctx, mats, ctx->mt_stage.host);
    HIP_TRY(ctx->mt_stage.send(ctx->mats.p, 0, mats.size(), ctx->stream));
    return MCPT_OK;
}

mcpt_status mcpt_update_materials(mcpt_ctx* ctx, const mcpt_material* materials, uint32_t n_materials) {
    const std::string who = "mcpt_update_materials: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!materials) return fail(MCPT_ERR_INVALID_ARG, who + "null materials");
    if (n_materials != uint32_t(ctx->dev.n_mats)) return fail(MCPT_ERR_INVALID_ARG, who + "n_materials differs from the scene's");
    uint64_t n_lights = 0;
    std::vector<uint8_t> emits(n_materials, 0);
    for (uint32_t i = 0; i < n_materials; i++) {
        const mcpt_material& m = materials[i];
        if (m.map_kd < 0 || size_t(m.map_kd) >= ctx->mt_tex.size()) return fail(MCPT_ERR_INVALID_ARG, who + "material " + std::to_string(i) + ": map_kd out of range");
        bool finite = std::isfinite(m.ns);
        for (int k = 0; k < 3; k++) finite = finite && std::isfinite(m.ks[k]) && std::isfinite(m.radiance[k]);
        if (!finite) return fail(MCPT_ERR_INVALID_ARG, who + "material " + std::to_string(i) + ": ks, ns or radiance is not finite");
        emits[i] = (device_material(m, ctx->mt_tex[size_t(m.map_kd)]).flags & MAT_EMIT_REC) ? 1 : 0;
        if (emits[i]) n_lights += ctx->mt_faces[i];
    }
    uint32_t hidden_emitters = 0;
    if (ctx->vs.set) {                                                    // §24: under a mask a light is an emissive face that is visible
        const VsPlan plan = vs_plan(ctx->vs.host.data(), ctx->vs.face_material.data(), uint32_t(ctx->vs.face_material.size()), emits.data(), n_materials);
        n_lights = plan.n_lights; hidden_emitters = plan.n_hidden_emitters;
    }
    if (n_lights == 0) return fail(MCPT_ERR_NO_LIGHTS, who + (ctx->vs.set ? "no visible face would be left with |radiance| > 0.01" : "no face would be left with |radiance| > 0.01"));
    const uint32_t nt = uint32_t(ctx->dev.n_tris);
    if (!ctx->mt_have_watch) { HIP_TRY(ctx->mt_watch.create()); ctx->mt_have_watch = true; }
    HIP_TRY(ctx->mt_stage.wait());
    HIP_TRY(ctx->mt_stage.grow(n_materials));
    st = mt_ensure_list(ctx, n_lights); if (st != MCPT_OK) return st;
    // Everything below is stream work on the context's stream, ordered like mcpt_update_vertices: renders enqueued so far have joined it, the
    // next render's sub-pipelines fork from it after the last kernel here.
    hipStream_t s = ctx->stream;
    const std::vector<mcpt_material> mats(materials, materials + n_materials);
    HIP_TRY(ctx->mt_watch.begin(s));
    st = mt_send_records(ctx, mats); if (st != MCPT_OK) return st;
    HIP_TRY(launch_mt_classes(ctx->tri_isect.p, ctx->dev.tri_shade, ctx->dev.tri_face, ctx->dev.mats, n_materials, ctx->mt_flag.p, nt, s, ctx->vs.dev_mask()));
    HIP_TRY(launch_mt_scan(ctx->mt_flag.p, ctx->mt_sums.p, nt, s));
    HIP_TRY(launch_mt_emit(ctx->dev.tri_isect, ctx->dev.tri_shade, ctx->dev.tri_pos64, ctx->dev.tri_face, ctx->dev.mats, n_materials, ctx->mt_flag.p,
                           ctx->lights.p, ctx->light_pos64.p, uint32_t(ctx->lights.count()), nt, s, ctx->vs.dev_mask()));
    HIP_TRY(ctx->mt_watch.end(s));
    ctx->mt_mats = mats; ctx->vs.n_hidden_emitters = hidden_emitters;
    ctx->dev.n_lights = int32_t(n_lights); ctx->info.n_lights = uint32_t(n_lights);
    ctx->mt_updates++;
    rf_forget_derived(ctx);
    return MCPT_OK;
}

mcpt_status mcpt_update_texture(mcpt_ctx* ctx, uint32_t index, const mcpt_texture* tex) {
    const std::string who = "mcpt_update_texture: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!tex || !tex->rgb) return fail(MCPT_ERR_INVALID_ARG, who + "null texture");
    if (size_t(index) >= ctx->mt_tex.size()) return fail(MCPT_ERR_INVALID_ARG, who + "texture index out of range");
    TexInfo& t = ctx->mt_tex[index];
    if (tex->width != t.w || tex->height != t.h) return fail(MCPT_ERR_INVALID_ARG, who + "width / height differ from the texture's at creation");
    const size_t n = size_t(t.w) * size_t(t.h);
    HIP_TRY(ctx->mt_tex_stage.wait());
    HIP_TRY(ctx->mt_tex_stage.grow(n));
    if (n == 1) { HIP_TRY(ctx->mt_stage.wait()); HIP_TRY(ctx->mt_stage.grow(ctx->mt_mats.size())); }   // (what can fail comes before anything changes)
    float4* h = ctx->mt_tex_stage.host;
    for (size_t k = 0; k < n; k++) h[k] = make_float4(tex->rgb[3 * k], tex->rgb[3 * k + 1], tex->rgb[3 * k + 2], 0.f);
    HIP_TRY(ctx->mt_tex_stage.send(ctx->texels.p + t.off, 0, n, ctx->stream));
    for (int k = 0; k < 3; k++) t.rgb[k] = tex->rgb[k];
    if (n == 1) { st = mt_send_records(ctx, ctx->mt_mats); if (st != MCPT_OK) return st; }   // a constant colour lives in the material records too
    rf_forget_derived(ctx);
    return MCPT_OK;
}

mcpt_status mcpt_get_material_info(mcpt_ctx* ctx, mcpt_material_info* out) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    st = resolve_timing(ctx); if (st != MCPT_OK) return st;
    if (ctx->mt_have_watch) HIP_TRY(ctx->mt_watch.settle());
    std::memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out; out->updates = ctx->mt_updates; out->n_lights = uint32_t(ctx->dev.n_lights); out->last_ms = ctx->mt_watch.last_ms;
    return MCPT_OK;
}

mcpt_status mcpt_probe_lights(mcpt_ctx* ctx, uint32_t capacity, int32_t* out_face, float* out13, double* out_pos9, uint32_t* out_n) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out_n) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    const uint32_t n = uint32_t(ctx->dev.n_lights);
    *out_n = n;
    if (capacity < n) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_lights: capacity < n_lights");
    if (!out_face || !out13 || !out_pos9) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
    std::vector<DevLight> rec(n);
    st = read_back(ctx, rec.data(), ctx->lights.p, size_t(n) * sizeof(DevLight), false); if (st != MCPT_OK) return st;
    st = read_back(ctx, out_pos9, ctx->light_pos64.p, 9 * size_t(n) * sizeof(double), false); if (st != MCPT_OK) return st;
    for (uint32_t i = 0; i < n; i++) {
        const DevLight& L = rec[i];
        if (L.tri < 0 || L.tri >= ctx->dev.n_tris) return fail(MCPT_ERR_HIP, "mcpt_probe_lights: a light names an out-of-range triangle");
        out_face[i] = ctx->h_tri_face[size_t(L.tri)];
        float* o = out13 + 13 * size_t(i);
        o[0] = L.area;
        for (int k = 0; k < 3; k++) { o[1 + k] = L.radiance[k]; o[4 + k] = L.n0[k]; o[7 + k] = L.n1[k]; o[10 + k] = L.n2[k]; }
    }
    return MCPT_OK;
}

mcpt_status mcpt_probe_face_classes(mcpt_ctx* ctx, uint8_t* out_class) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out_class) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
    const size_t nt = size_t(ctx->dev.n_tris);
    std::vector<f4h> isect(3 * nt);
    st = read_back(ctx, isect.data(), ctx->tri_isect.p, isect.size() * sizeof(f4h), false); if (st != MCPT_OK) return st;
    for (size_t i = 0; i < nt; i++) {
        uint32_t w; std::memcpy(&w, &isect[3 * i].w, 4);
        out_class[size_t(ctx->h_tri_face[i])] = uint8_t(w >> HIT_CLASS_SHIFT);
    }
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ temporal reprojection
// The options with their defaults filled in, or the refusal.
static mcpt_status rp_read_opts(const mcpt_reproject_opts* opts, mcpt_reproject_opts& o, const char* fn) {
    mcpt_status st = read_opts(opts, o, fn, "mcpt_reproject_opts"); if (st != MCPT_OK) return st;
    const std::string who = std::string(fn) + ": ";
    if (o.feature_spp > DN_MAX_SPP) return fail(MCPT_ERR_INVALID_ARG, who + "feature_spp must be <= 64 (0 = default 4)");
    if (o.max_history != 0.f && !(std::isfinite(o.max_history) && o.max_history >= 1.f)) return fail(MCPT_ERR_INVALID_ARG, who + "max_history must be finite and >= 1 (0 = default 32)");
    if (o.depth_tolerance != 0.f && !(o.depth_tolerance > 0.f && o.depth_tolerance <= 1.f)) return fail(MCPT_ERR_INVALID_ARG, who + "depth_tolerance must be in (0, 1] (0 = default 0.05)");
    if (o.normal_threshold != 0.f && !(o.normal_threshold > 0.f && o.normal_threshold <= 1.f)) return fail(MCPT_ERR_INVALID_ARG, who + "normal_threshold must be in (0, 1] (0 = default 0.9)");
    if (o.feature_spp == 0) o.feature_spp = 4u;
    if (o.max_history == 0.f) o.max_history = 32.f;
    if (o.depth_tolerance == 0.f) o.depth_tolerance = 0.05f;
    if (o.normal_threshold == 0.f) o.normal_threshold = 0.9f;
    return MCPT_OK;
}
// What motion-vector reprojection (§14) reads besides: the first-hit records of the new scene and view, and rf_n_vertex / rf_n_normal device
// records of the scene before the update.
struct RpOldScene { const float4* hits; const double* vtx; const double* nrm; };
// rp_reproject_kernel -- with `motion`, rp_reproject_motion_kernel -- from the view `old_cam` into the view `new_cam` on the context's stream: `out`
// gets the reprojected film, *count the pixels reused.  An old view whose image basis is singular has no inverse projection: the film is cleared
// instead (no pixel reused).
static mcpt_status rp_run(mcpt_ctx* ctx, const DevCamera& old_cam, const DevCamera& new_cam, const mcpt_reproject_opts& o, const RpOldScene* motion,
                          const float4* old_film, const float4* old_feat, const float4* new_feat, float4* out, unsigned long long* count) {
    RpParams p;
    p.old_cam = old_cam; p.new_cam = new_cam;
    p.max_history = o.max_history; p.depth_tolerance = o.depth_tolerance; p.normal_threshold = o.normal_threshold;
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(unsigned long long), ctx->stream));
    if (!rp_basis_inverse(old_cam, p.inv)) {
        HIP_TRY(hipMemsetAsync(out, 0, size_t(ctx->width) * ctx->height * sizeof(float4), ctx->stream));
        return MCPT_OK;
    }
    if (!motion) {
        HIP_TRY(launch_rp_reproject(p, old_film, old_feat, new_feat, out, count, ctx->stream));
        return MCPT_OK;
    }
    RpMotion m;
    m.hits = motion->hits; m.idx6 = ctx->rf_idx.p; m.old_vtx = motion->vtx; m.old_nrm = motion->nrm;
    m.tri_shade = ctx->dev.tri_shade; m.mats = ctx->dev.mats;
    for (int a = 0; a < 3; a++) m.centre[a] = ctx->dev.centre[a];
    m.n_tris = uint32_t(ctx->dev.n_tris); m.n_vertex = ctx->rf_n_vertex; m.n_normal = ctx->rf_n_normal; m.n_mats = uint32_t(ctx->dev.n_mats);
    HIP_TRY(launch_rp_reproject_motion(p, m, old_film, old_feat, new_feat, out, count, ctx->stream));
    return MCPT_OK;
}

// The buffers of a reprojection call, allocated by the first one and committed only when all of them are there.  `motion`: also those of §14.
static mcpt_status rp_ensure(mcpt_ctx* ctx, bool motion) {
    const size_t n = size_t(ctx->width) * ctx->height;
    uint64_t* tally = &ctx->info.device_bytes;
    const bool base = !ctx->rp_film_old.p, more = motion && !ctx->rp_hits.p;
    HIP_TRY(alloc_all(Want(ctx->rp_feat_old, 2 * n, tally, base), Want(ctx->rp_film_old, n, tally, base), Want(ctx->rp_count, 1, nullptr, base),
                      Want(ctx->dn_feat, 2 * n, tally, base && !ctx->dn_feat.p), Want(ctx->rp_watch, 1, nullptr, base), Want(ctx->rp_hits, n, tally, more),
                      Want(ctx->rp_vtx_old, ctx->rf_vtx.count(), tally, more), Want(ctx->rp_nrm_old, ctx->rf_nrm.count(), tally, more)));
    return MCPT_OK;
}

// The frame of a reprojection entry point whose own arguments have been checked: the film is carried from the scene and view as they are to the
// scene after `update` (null: unchanged, §13) seen from `cm` (null: the same camera).  `fn` names the entry point in the message.
static mcpt_status rp_frame(mcpt_ctx* ctx, const RfUpdate* update, const mcpt_camera* cm, const mcpt_reproject_opts* opts, const char* fn) {
    mcpt_reproject_opts o;
    mcpt_status st = rp_read_opts(opts, o, fn); if (st != MCPT_OK) return st;
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the feature kernel's traversal stack");
    st = rp_ensure(ctx, update != nullptr); if (st != MCPT_OK) return st;
    // Everything below is stream work on the context's stream, ordered like mcpt_set_camera / mcpt_update_vertices: renders enqueued before it have
    // joined the stream, the next render's sub-pipelines fork from it after the last kernel here.
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx->rp_watch.begin(s));
    if (!ctx->dn_have_features) { st = dn_render_features(ctx, o.feature_spp, o.feature_seed); if (st != MCPT_OK) return st; }
    std::swap(ctx->dn_feat, ctx->rp_feat_old);                             // the old scene's and view's features are kept where they lie
    HIP_TRY(hipMemcpyAsync(ctx->rp_film_old.p, ctx->accum, ctx->rp_film_old.bytes, hipMemcpyDeviceToDevice, s));
    if (update && ctx->rf_vtx.bytes) HIP_TRY(hipMemcpyAsync(ctx->rp_vtx_old.p, ctx->rf_vtx.p, ctx->rf_vtx.bytes, hipMemcpyDeviceToDevice, s));
    if (update && ctx->rf_nrm.bytes) HIP_TRY(hipMemcpyAsync(ctx->rp_nrm_old.p, ctx->rf_nrm.p, ctx->rf_nrm.bytes, hipMemcpyDeviceToDevice, s));
    const DevCamera old_cam = ctx->dev.cam;
    if (update) { st = rf_enqueue_update(ctx, *update); if (st != MCPT_OK) return st; }
    if (cm) apply_camera(ctx, *cm);
    st = dn_render_features(ctx, o.feature_spp, o.feature_seed);           // those of the new scene and view: mcpt_denoise may follow at once
    if (st != MCPT_OK) return st;
    if (update) HIP_TRY(launch_rp_first_hit(ctx->dev, ctx->rp_hits.p, s));
    const RpOldScene old{ctx->rp_hits.p, ctx->rp_vtx_old.p, ctx->rp_nrm_old.p};
    st = rp_run(ctx, old_cam, ctx->dev.cam, o, update ? &old : nullptr, ctx->rp_film_old.p, ctx->rp_feat_old.p, ctx->dn_feat.p, ctx->accum, ctx->rp_count.p);
    if (st != MCPT_OK) return st;
    HIP_TRY(ctx->rp_watch.end(s));
    ctx->rp_calls++;
    return MCPT_OK;
}

mcpt_status mcpt_set_camera_reproject(mcpt_ctx* ctx, const mcpt_camera* cm, const mcpt_reproject_opts* opts) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    st = check_camera(ctx, cm, "mcpt_set_camera_reproject"); if (st != MCPT_OK) return st;
    return rp_frame(ctx, nullptr, cm, opts, "mcpt_set_camera_reproject");
}

mcpt_status mcpt_get_reproject_info(mcpt_ctx* ctx, mcpt_reproject_info* out) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    unsigned long long c = 0;                                              // (no call yet: no counter to read, the stream is drained all the same)
    st = read_back(ctx, &c, ctx->rp_count.p, ctx->rp_calls ? sizeof c : 0); if (st != MCPT_OK) return st;
    HIP_TRY(ctx->rp_watch.settle());
    std::memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out; out->reprojections = ctx->rp_calls; out->last_ms = ctx->rp_watch.last_ms; out->pixels_reused = c;
    return MCPT_OK;
}

// What the two reprojection probes share once their own arguments are checked: the two cameras, the options, the three films staged, rp_run into a
// scratch film and counter, both fetched.  `stage_motion` (§14; may refuse) stages its inputs first and says where they are.
using RpStageMotion = std::function<mcpt_status(Scratch&, RpOldScene&)>;
static mcpt_status rp_probe(mcpt_ctx* ctx, const char* fn, const mcpt_camera* old_cam, const mcpt_camera* new_cam, const float* old_film_host,
                            const float* old_feat8_host, const float* new_feat8_host, const mcpt_reproject_opts* opts, const RpStageMotion& stage_motion,
                            float* out_film_host, uint64_t* out_reused) {
    mcpt_status st = check_camera(ctx, old_cam, (std::string(fn) + " (old camera)").c_str()); if (st != MCPT_OK) return st;
    st = check_camera(ctx, new_cam, (std::string(fn) + " (new camera)").c_str()); if (st != MCPT_OK) return st;
    mcpt_reproject_opts o;
    st = rp_read_opts(opts, o, fn); if (st != MCPT_OK) return st;
    const size_t n = size_t(ctx->width) * ctx->height;
    DevCamera co, cn;
    camera_constants(*old_cam, ctx->dev.centre, co); camera_constants(*new_cam, ctx->dev.centre, cn);
    Scratch s(ctx->stream); RpOldScene old{}; float4 *film, *fo, *fnew, *out; unsigned long long* count;
    if (stage_motion) { st = stage_motion(s, old); if (st != MCPT_OK) return st; }
    HIP_TRY(s.in(reinterpret_cast<const float4*>(old_film_host), n, &film));
    HIP_TRY(s.in(reinterpret_cast<const float4*>(old_feat8_host), 2 * n, &fo)); HIP_TRY(s.in(reinterpret_cast<const float4*>(new_feat8_host), 2 * n, &fnew));
    HIP_TRY(s.out(n, &out)); HIP_TRY(s.out(1, &count));
    st = rp_run(ctx, co, cn, o, stage_motion ? &old : nullptr, film, fo, fnew, out, count); if (st != MCPT_OK) return st;
    unsigned long long c = 0;
    HIP_TRY(s.fetch(&c, count, 1)); HIP_TRY(s.fetch(out_film_host, out, 4 * n)); HIP_TRY(s.finish());
    *out_reused = c;
    return MCPT_OK;
}

mcpt_status mcpt_probe_reproject(mcpt_ctx* ctx, const mcpt_camera* old_cam, const mcpt_camera* new_cam, const float* old_film_host, const float* old_feat8_host,
                                 const float* new_feat8_host, const mcpt_reproject_opts* opts, float* out_film_host, uint64_t* out_reused) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!old_film_host || !old_feat8_host || !new_feat8_host || !out_film_host || !out_reused) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    return rp_probe(ctx, "mcpt_probe_reproject", old_cam, new_cam, old_film_host, old_feat8_host, new_feat8_host, opts, nullptr, out_film_host, out_reused);
}

// ------------------------------------------------------------------------------------------------ motion-vector reprojection
// Every update entry point, plain or _reproject, once it has named its source.  The order of the refusals is part of the interface: the context,
// the source's own rules (by its tag), the camera (a _reproject form may pass one), the options.  Morph with bones allocates its scratch next,
// and only in a call that will not be refused: rp_frame turns away unreadable options and a scene whose binary tree is too deep.
static mcpt_status rf_update(mcpt_ctx* ctx, const RfUpdate& u, const char* fn, const mcpt_camera* cm, const mcpt_reproject_opts* opts, bool reproject) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, std::string(fn) + ": ")) != MCPT_OK) return st;
    switch (u.source) {
    case Source::Arrays: st = rf_check_update(ctx, u.vertex, u.n_vertex, u.normal, u.n_normal, fn); break;
    case Source::Groups: st = xf_check_update(ctx, u.m3x4, u.n_m3x4, fn); break;
    case Source::Skin: st = sk_check_update(ctx, u.m3x4, u.n_m3x4, fn); break;
    case Source::Morph: case Source::MorphSkin: st = mo_check_update(ctx, u.weight, u.n_weight, u.m3x4, u.n_m3x4, fn); break;
    case Source::Keyframes: st = kf_check_update(ctx, u.time, fn); break;
    case Source::Parts: st = pt_check_update(ctx, u.parts, fn); break;
    case Source::None: break;                                                    // (mcpt_update_normals makes its own two checks)
    }
    if (st != MCPT_OK) return st;
    if (reproject && cm) { st = check_camera(ctx, cm, fn); if (st != MCPT_OK) return st; }
    if ((u.source == Source::MorphSkin || u.parts_morph_then_skin()) && (!reproject || ctx->binary_ok)) {
        mcpt_reproject_opts o;
        if (reproject) { st = rp_read_opts(opts, o, fn); if (st != MCPT_OK) return st; }
        st = ctx->mo.ensure_scratch(ctx); if (st != MCPT_OK) return st;
    }
    return reproject ? rp_frame(ctx, &u, cm, opts, fn) : rf_enqueue_update(ctx, u);
}

mcpt_status mcpt_update_vertices_reproject(mcpt_ctx* ctx, const double* vertex, uint32_t n_vertex, const double* normal, uint32_t n_normal,
                                           const mcpt_camera* cm, const mcpt_reproject_opts* opts) {
    return rf_update(ctx, RfUpdate::arrays(vertex, n_vertex, normal, n_normal), "mcpt_update_vertices_reproject", cm, opts, true);
}

mcpt_status mcpt_update_transforms_reproject(mcpt_ctx* ctx, const double* m3x4, uint32_t n_groups, const mcpt_camera* cm, const mcpt_reproject_opts* opts) {
    return rf_update(ctx, RfUpdate::groups(m3x4, n_groups), "mcpt_update_transforms_reproject", cm, opts, true);
}

mcpt_status mcpt_update_skin_reproject(mcpt_ctx* ctx, const double* m3x4, uint32_t n_bones, const mcpt_camera* cm, const mcpt_reproject_opts* opts) {
    return rf_update(ctx, RfUpdate::skin(m3x4, n_bones), "mcpt_update_skin_reproject", cm, opts, true);
}

mcpt_status mcpt_update_morph_reproject(mcpt_ctx* ctx, const double* weight, uint32_t n_targets, const double* bones_m3x4, uint32_t n_bones,
                                        const mcpt_camera* cm, const mcpt_reproject_opts* opts) {
    return rf_update(ctx, RfUpdate::morph(weight, n_targets, bones_m3x4, n_bones), "mcpt_update_morph_reproject", cm, opts, true);
}

mcpt_status mcpt_update_keyframes_reproject(mcpt_ctx* ctx, double time, const mcpt_camera* cm, const mcpt_reproject_opts* opts) {
    return rf_update(ctx, RfUpdate::keyframes(time), "mcpt_update_keyframes_reproject", cm, opts, true);
}

mcpt_status mcpt_update_parts_reproject(mcpt_ctx* ctx, const mcpt_scene_update* update, const mcpt_camera* cm, const mcpt_reproject_opts* opts) {
    return rf_update(ctx, RfUpdate::of_parts(update), "mcpt_update_parts_reproject", cm, opts, true);
}

mcpt_status mcpt_probe_first_hits(mcpt_ctx* ctx, int32_t* out_face, float* out_uvt3) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out_face || !out_uvt3) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the first-hit kernel's traversal stack");
    st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
    const size_t n = size_t(ctx->width) * ctx->height;
    std::vector<float> rec(4 * n);
    {   Scratch s(ctx->stream); float4* hits;
        HIP_TRY(s.out(n, &hits));
        HIP_TRY(launch_rp_first_hit(ctx->dev, hits, ctx->stream));
        HIP_TRY(s.fetch(rec.data(), hits, 4 * n)); HIP_TRY(s.finish()); }
    for (size_t i = 0; i < n; i++) {
        int32_t tri; std::memcpy(&tri, &rec[4 * i], 4);
        if (tri >= ctx->dev.n_tris) return fail(MCPT_ERR_HIP, "mcpt_probe_first_hits: the kernel returned an out-of-range triangle");
        out_face[i] = tri < 0 ? -1 : ctx->h_tri_face[size_t(tri)];
        for (int k = 0; k < 3; k++) out_uvt3[3 * i + k] = tri < 0 ? 0.f : rec[4 * i + 1 + k];
    }
    return MCPT_OK;
}

mcpt_status mcpt_probe_reproject_motion(mcpt_ctx* ctx, const mcpt_camera* old_cam, const mcpt_camera* new_cam, const double* old_vertex, const double* old_normal,
                                        const float* old_film_host, const float* old_feat8_host, const float* new_feat8_host, const int32_t* hit_face_host,
                                        const float* hit_uv2_host, const mcpt_reproject_opts* opts, float* out_film_host, uint64_t* out_reused) {
    const char* const fn = "mcpt_probe_reproject_motion";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!old_film_host || !old_feat8_host || !new_feat8_host || !hit_face_host || !hit_uv2_host || !out_film_host || !out_reused) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if ((st = require_dynamic(ctx, std::string(fn) + ": ")) != MCPT_OK) return st;
    const auto stage_motion = [&](Scratch& s, RpOldScene& old) -> mcpt_status {
        mcpt_status st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
        const size_t n = size_t(ctx->width) * ctx->height, nf = ctx->h_tri_face.size();
        // hits the way mcpt_probe_hit_shade takes them (Model::face indices), turned into the kernel's records on the host; nothing out of range leaves it
        std::vector<int32_t> leaf_of_face(nf, -1);
        for (size_t i = 0; i < nf; i++) leaf_of_face[size_t(ctx->h_tri_face[i])] = int32_t(i);
        std::vector<float> rec(4 * n, 0.f);
        for (size_t i = 0; i < n; i++) {
            const int32_t f = hit_face_host[i]; const float u = hit_uv2_host[2 * i], v = hit_uv2_host[2 * i + 1];
            if (f < -1 || (f >= 0 && size_t(f) >= nf)) return fail(MCPT_ERR_INVALID_ARG, std::string(fn) + ": face index out of range");
            if (!std::isfinite(u) || !std::isfinite(v)) return fail(MCPT_ERR_INVALID_ARG, std::string(fn) + ": a hit's u or v is not finite");
            const int32_t tri = f < 0 ? -1 : leaf_of_face[size_t(f)];
            std::memcpy(&rec[4 * i], &tri, 4); rec[4 * i + 1] = u; rec[4 * i + 2] = v;
        }
        double *d_vtx = ctx->rf_vtx.p, *d_nrm = ctx->rf_nrm.p; float4* hits;   // the old scene: the caller's arrays, or the context's current ones
        if (old_vertex) HIP_TRY(s.in(old_vertex, ctx->rf_vtx.count(), &d_vtx));
        if (old_normal) HIP_TRY(s.in(old_normal, ctx->rf_nrm.count(), &d_nrm));
        HIP_TRY(s.in(reinterpret_cast<const float4*>(s.keep(std::move(rec))), n, &hits));
        old = RpOldScene{hits, d_vtx, d_nrm};
        return MCPT_OK;
    };
    return rp_probe(ctx, fn, old_cam, new_cam, old_film_host, old_feat8_host, new_feat8_host, opts, stage_motion, out_film_host, out_reused);
}

mcpt_status mcpt_probe_validate_trees(mcpt_ctx* ctx) {
    mcpt_status st = use_drained(ctx); if (st != MCPT_OK) return st;
    HostScene hs;
    auto get = [&](auto& host, const auto& dev) {
        static_assert(sizeof(host[0]) == sizeof(*dev.p), "the host mirror of a device element has its size (f4h / float4)");
        host.resize(dev.count());
        return read_back(ctx, host.data(), dev.p, dev.bytes, false);
    };
    if ((st = get(hs.nodes, ctx->nodes)) != MCPT_OK || (st = get(hs.nodes8, ctx->nodes8)) != MCPT_OK || (st = get(hs.tri_isect, ctx->tri_isect)) != MCPT_OK ||
        (st = get(hs.tri_face, ctx->tri_face)) != MCPT_OK) return st;
    std::string bad = validate_bvh8(hs);
    if (!bad.empty()) return fail(MCPT_ERR_INVALID_ARG, "8-wide tree: " + bad);
    bad = validate_bvh2(hs);
    if (!bad.empty()) return fail(MCPT_ERR_INVALID_ARG, bad);
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ face visibility
// Both forms of mcpt_set_face_visibility.  Everything that can refuse comes first and is host work: the context, n_face, the light count of the mask
// under the current materials (vs_plan), and for the _reproject form what rp_frame would turn away.  Then the mask is staged and copied in stream
// order, and the call becomes a scene update without a source that also rebuilds the light list.
static mcpt_status vs_set(mcpt_ctx* ctx, const uint8_t* visible, uint32_t n_face, const mcpt_camera* cm, const mcpt_reproject_opts* opts, bool reproject, const char* fn) {
    const std::string who = std::string(fn) + ": ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    if (n_face != uint32_t(ctx->dev.n_tris)) return fail(MCPT_ERR_INVALID_ARG, who + "n_face differs from the scene's");
    mcpt_ctx::Visibility& vs = ctx->vs;
    std::vector<uint8_t> host(visible ? n_face : 0u);
    for (uint32_t f = 0; f < uint32_t(host.size()); f++) host[f] = visible[f] != 0 ? 1 : 0;
    const uint32_t n_mats = uint32_t(ctx->mt_mats.size());
    std::vector<uint8_t> emits(n_mats, 0);
    for (uint32_t i = 0; i < n_mats; i++) emits[i] = (device_material(ctx->mt_mats[i], ctx->mt_tex[size_t(ctx->mt_mats[i].map_kd)]).flags & MAT_EMIT_REC) ? 1 : 0;
    const VsPlan plan = vs_plan(visible ? host.data() : nullptr, vs.face_material.data(), n_face, emits.data(), n_mats);
    if (plan.n_lights == 0) return fail(MCPT_ERR_NO_LIGHTS, who + "no face with |radiance| > 0.01 would stay visible");
    if (reproject) {
        if (cm && (st = check_camera(ctx, cm, fn)) != MCPT_OK) return st;
        mcpt_reproject_opts o;
        if ((st = rp_read_opts(opts, o, fn)) != MCPT_OK) return st;
        if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the feature kernel's traversal stack");
    }
    // nothing below refuses; what fails is a HIP call
    if (!visible && vs.set) HIP_TRY(hipStreamSynchronize(ctx->stream));          // kernels enqueued earlier may still read the mask that is about to be freed
    HIP_TRY(alloc_all(Want(vs.mask, n_face, &ctx->info.device_bytes, visible && !vs.mask.p), Want(vs.stage, n_face, nullptr, visible && vs.stage.cap < n_face),
                      Want(vs.watch, 1, nullptr, !vs.watch.ev0)));
    st = mt_ensure_list(ctx, plan.n_lights); if (st != MCPT_OK) return st;
    if (visible) {
        HIP_TRY(vs.stage.wait());
        std::memcpy(vs.stage.host, host.data(), n_face);
        HIP_TRY(vs.stage.send(vs.mask.p, 0, n_face, ctx->stream));
        vs.host.swap(host); vs.set = true; vs.n_hidden = plan.n_hidden; vs.n_hidden_emitters = plan.n_hidden_emitters;
    } else vs.drop();
    return rf_update(ctx, RfUpdate::visibility(plan.n_lights), fn, cm, opts, reproject);
}

mcpt_status mcpt_set_face_visibility(mcpt_ctx* ctx, const uint8_t* visible, uint32_t n_face) {
    return vs_set(ctx, visible, n_face, nullptr, nullptr, false, "mcpt_set_face_visibility");
}

mcpt_status mcpt_set_face_visibility_reproject(mcpt_ctx* ctx, const uint8_t* visible, uint32_t n_face, const mcpt_camera* cm, const mcpt_reproject_opts* opts) {
    return vs_set(ctx, visible, n_face, cm, opts, true, "mcpt_set_face_visibility_reproject");
}

mcpt_status mcpt_get_visibility_info(mcpt_ctx* ctx, mcpt_visibility_info* out) {
    const mcpt_status st = info_begin(ctx, out, ctx ? &ctx->vs.watch : nullptr); if (st != MCPT_OK) return st;
    const mcpt_ctx::Visibility& vs = ctx->vs;
    out->set = vs.set ? 1u : 0u; out->n_hidden = vs.n_hidden; out->n_hidden_emitters = vs.n_hidden_emitters; out->updates = vs.updates;
    out->last_ms = vs.watch.last_ms; out->device_bytes = vs.mask.bytes;
    return MCPT_OK;
}

mcpt_status mcpt_probe_triangles(mcpt_ctx* ctx, float* out_v0e1e2, float* out_box6) {
    const std::string who = "mcpt_probe_triangles: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if ((st = require_dynamic(ctx, who)) != MCPT_OK) return st;
    if (out_box6 && !ctx->vs.box_valid) return fail(MCPT_ERR_INVALID_ARG, who + "no scene update has written the boxes since creation or the last rebuild");
    st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
    const size_t nt = size_t(ctx->dev.n_tris);
    std::vector<f4h> isect(out_v0e1e2 ? 3 * nt : 0); std::vector<float> box(out_box6 ? 6 * nt : 0);
    st = read_back(ctx, isect.data(), ctx->tri_isect.p, isect.size() * sizeof(f4h), false); if (st != MCPT_OK) return st;
    st = read_back(ctx, box.data(), ctx->rf_tri_box.p, box.size() * sizeof(float)); if (st != MCPT_OK) return st;
    for (size_t i = 0; i < nt; i++) {
        const size_t f = size_t(ctx->h_tri_face[i]);
        if (f >= nt) return fail(MCPT_ERR_HIP, who + "the context's leaf order is damaged");
        if (out_v0e1e2) for (int k = 0; k < 3; k++) { const f4h& r = isect[3 * i + k]; float* o = out_v0e1e2 + 9 * f + 3 * k; o[0] = r.x; o[1] = r.y; o[2] = r.z; }
        if (out_box6) std::memcpy(out_box6 + 6 * f, box.data() + 6 * i, 6 * sizeof(float));
    }
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ camera models
mcpt_status mcpt_set_camera_model(mcpt_ctx* ctx, const mcpt_camera_model* model) {
    const std::string who = "mcpt_set_camera_model: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    mcpt_camera_model m;
    if ((st = read_opts(model, m, "mcpt_set_camera_model", "mcpt_camera_model")) != MCPT_OK) return st;
    if (m.model > MCPT_CAMERA_EQUIRECT) return fail(MCPT_ERR_INVALID_ARG, who + "unknown model");
    if (m.model == MCPT_CAMERA_THIN_LENS) {
        if (!std::isfinite(m.lens_radius) || m.lens_radius < 0.0) return fail(MCPT_ERR_INVALID_ARG, who + "lens_radius must be finite and >= 0");
        if (!std::isfinite(m.focus_distance) || !(m.focus_distance > 0.0)) return fail(MCPT_ERR_INVALID_ARG, who + "focus_distance must be finite and > 0");
        if (m.blades != 0u && (m.blades < 3u || m.blades > MCPT_CAMERA_MAX_BLADES)) return fail(MCPT_ERR_INVALID_ARG, who + "blades must be 0 (a disk) or in [3, 16]");
        if (!std::isfinite(m.blade_rotation)) return fail(MCPT_ERR_INVALID_ARG, who + "blade_rotation must be finite");
    }
    if (m.model == MCPT_CAMERA_ORTHOGRAPHIC && (!std::isfinite(m.ortho_height) || !(m.ortho_height > 0.0))) return fail(MCPT_ERR_INVALID_ARG, who + "ortho_height must be finite and > 0");
    ctx->cm.model = m; ctx->cm.dev = cm_make_model(m);                     // (by value with every launch, like the camera: launches already enqueued keep the old one)
    return MCPT_OK;
}

mcpt_status mcpt_get_camera_model(mcpt_ctx* ctx, mcpt_camera_model* out, mcpt_camera_model_info* out_info) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    *out = ctx->cm.model;
    if (!out_info) return MCPT_OK;
    mcpt_ctx::Camera& cm = ctx->cm;
    HIP_TRY(cm.take());                                                      // (the last call's last pass joins its sum; info_begin then finds the watch settled)
    st = info_begin(ctx, out_info, &cm.watch); if (st != MCPT_OK) return st;
    out_info->model = cm.model.model; out_info->renders = cm.renders; out_info->passes = cm.passes; out_info->last_stage_ms = cm.stage_ms;
    out_info->device_bytes = cm.ray_o.bytes + cm.ray_d.bytes;
    return MCPT_OK;
}

// The RenderParams of a probe job but for its three probe_* fields: item i = entry i of an n x 1 film, one sample `sample` of `seed` each.  Shared by
// mcpt_probe_paths (host rays, a scratch film) and mcpt_render_camera (the stage's rays, the bound film).
static RenderParams probe_job_params(const mcpt_ctx* ctx, uint32_t sample, uint64_t seed, uint32_t flags) {
    RenderParams p; std::memset(&p, 0, sizeof p);
    p.spp = 1; p.first_sample = sample; p.samples_per_item = 1; p.chunks = 1; p.tiles_x = 0x7fffffffu; p.tiles_y = 1; p.tile_mod = 1; p.tile_rem = 0; p.n_owned = 0x7fffffffu;
    p.max_depth = ctx->opts.max_depth; p.flags = flags; p.integrator = MCPT_INTEGRATOR_MIS;
    p.seed_lo = uint32_t(seed); p.seed_hi = uint32_t(seed >> 32);
    return p;
}

mcpt_status mcpt_render_camera(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample) {
    const std::string who = "mcpt_render_camera: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!ctx->use_wavefront || ctx->lanes.empty()) return fail(MCPT_ERR_UNSUPPORTED, who + "needs the wavefront pipeline (MCPT_INTEGRATOR_MIS, no MCPT_PIPELINE=mega)");
    if (uint64_t(first_sample) + spp > (1ull << 32)) return fail(MCPT_ERR_INVALID_ARG, who + "first_sample + spp exceeds 2^32");
    const uint64_t n = uint64_t(ctx->width) * uint64_t(ctx->height);
    if (n > 0x3ffffffull) return fail(MCPT_ERR_INVALID_ARG, who + "the film has more pixels than a probe call takes");
    if (spp == 0) return MCPT_OK;
    mcpt_ctx::Camera& cm = ctx->cm;
    if (!cm.ray_o.p) HIP_TRY(alloc_all(Want(cm.ray_o, 3 * size_t(n), &ctx->info.device_bytes), Want(cm.ray_d, 3 * size_t(n), &ctx->info.device_bytes), Want(cm.watch, 1, nullptr, !cm.watch.ev0)));
    HIP_TRY(cm.take());                                                      // (the last call's last pass)
    cm.stage_ms = 0.0;
    st = timed_begin(ctx); if (st != MCPT_OK) return st;
    for (uint32_t k = 0; k < spp; k++) {
        const uint32_t s = first_sample + k;
        HIP_TRY(cm.take());
        HIP_TRY(cm.watch.begin(ctx->stream));
        HIP_TRY(launch_cm_rays(ctx->dev.cam, cm.dev, s, uint32_t(seed), uint32_t(seed >> 32), cm.ray_o.p, cm.ray_d.p, ctx->stream));
        HIP_TRY(cm.watch.end(ctx->stream));
        // the sub-pipeline's stream forks from the context's after the ray kernel and joins it again: the next pass's kernel overwrites the rays only
        // after this pass's paths have read them
        RenderParams p = probe_job_params(ctx, s, seed, ctx->opts.flags);
        p.probe_n = uint32_t(n); p.probe_o = cm.ray_o.p; p.probe_d = cm.ray_d.p;
        st = render_wavefront(ctx, p, ctx->accum); if (st != MCPT_OK) return st;
        cm.passes++;
    }
    cm.renders++;
    return timed_end(ctx);
}

mcpt_status mcpt_autofocus(mcpt_ctx* ctx, int32_t px, int32_t py, double* out_focus_distance) {
    const std::string who = "mcpt_autofocus: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out_focus_distance) return fail(MCPT_ERR_INVALID_ARG, "null output");
    if (px < 0 || py < 0 || px >= ctx->width || py >= ctx->height) return fail(MCPT_ERR_INVALID_ARG, who + "the pixel is outside the film");
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the first-hit kernel's traversal stack");
    const size_t n = size_t(ctx->width) * ctx->height, i = size_t(py) * ctx->width + size_t(px);
    const int32_t xy[2] = {px, py}; const float xi[2] = {0.5f, 0.5f};
    float rec[4], ray[6];
    {   Scratch s(ctx->stream); float4* hits; int* d_xy; float *d_xi, *d_ray;
        HIP_TRY(s.out(n, &hits)); HIP_TRY(s.in(xy, 2, &d_xy)); HIP_TRY(s.in(xi, 2, &d_xi)); HIP_TRY(s.out(6, &d_ray));
        HIP_TRY(launch_rp_first_hit(ctx->dev, hits, ctx->stream));
        HIP_TRY(launch_probe_cast_ray(ctx->dev, 1, d_xy, d_xi, d_ray, ctx->stream));      // the same pixel-centre ray: its direction as the device forms it
        HIP_TRY(s.fetch(rec, hits + i, 4)); HIP_TRY(s.fetch(ray, d_ray, 6)); HIP_TRY(s.finish()); }
    int32_t tri; std::memcpy(&tri, &rec[0], 4);
    if (tri < 0) return fail(MCPT_ERR_INVALID_ARG, who + "the pixel-centre ray hits nothing");
    const double* f = ctx->dev.cam.front;
    *out_focus_distance = double(rec[3]) * (double(ray[3]) * f[0] + double(ray[4]) * f[1] + double(ray[5]) * f[2]);
    return MCPT_OK;
}

mcpt_status mcpt_probe_camera_rays(mcpt_ctx* ctx, uint32_t n, const int32_t* xy, uint32_t sample, uint64_t seed, double* out_origin3, double* out_dir3) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!xy || !out_origin3 || !out_dir3) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    for (size_t k = 0; k < size_t(n); k++)
        if (xy[2 * k] < 0 || xy[2 * k + 1] < 0 || xy[2 * k] >= ctx->width || xy[2 * k + 1] >= ctx->height)
            return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_camera_rays: pixel " + std::to_string(k) + " is outside the film");
    if (n == 0) return MCPT_OK;
    Scratch s(ctx->stream); int* d_xy; double *d_o, *d_d;
    HIP_TRY(s.in(xy, 2 * size_t(n), &d_xy)); HIP_TRY(s.out(3 * size_t(n), &d_o)); HIP_TRY(s.out(3 * size_t(n), &d_d));
    HIP_TRY(launch_cm_probe(ctx->dev.cam, ctx->cm.dev, n, d_xy, sample, uint32_t(seed), uint32_t(seed >> 32), d_o, d_d, ctx->stream));
    HIP_TRY(s.fetch(out_origin3, d_o, 3 * size_t(n))); HIP_TRY(s.fetch(out_dir3, d_d, 3 * size_t(n))); HIP_TRY(s.finish());
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ surface baking
mcpt_status mcpt_set_bake_points(mcpt_ctx* ctx, const mcpt_bake_point* points, uint32_t n) {
    const std::string who = "mcpt_set_bake_points: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    const std::string bad = bk_check_points(points, n, uint32_t(ctx->dev.n_tris));
    if (!bad.empty()) return fail(MCPT_ERR_INVALID_ARG, who + bad);
    mcpt_ctx::Bake& bk = ctx->bk;
    // nothing below refuses; what fails is a HIP call
    st = use_drained(ctx); if (st != MCPT_OK) return st;                     // bakes enqueued earlier read the buffers that are about to be replaced
    HIP_TRY(bk.take());
    if (n == 0) { bk.drop(); return MCPT_OK; }
    st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
    std::vector<int32_t> leaf_of_face(ctx->h_tri_face.size(), -1);
    for (size_t i = 0; i < ctx->h_tri_face.size(); i++) leaf_of_face[size_t(ctx->h_tri_face[i])] = int32_t(i);
    uint64_t* tally = &ctx->info.device_bytes;
    HIP_TRY(alloc_all(Want(bk.pts, n, tally), Want(bk.dead, n, tally), Want(bk.film, n, tally), Want(bk.watch, 1, nullptr, !bk.watch.ev0)));
    if (bk.ray_o.p && bk.ray_o.count() != 3 * size_t(n)) { bk.ray_o.release(); bk.ray_d.release(); }   // (the first bake of the new list allocates its own)
    bk.host.assign(points, points + n);
    const std::vector<BkPoint> dev = bk.in_leaf_terms(leaf_of_face);
    HIP_TRY(hipMemcpyAsync(bk.pts.p, dev.data(), bk.pts.bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(bk.dead.p, 0, bk.dead.bytes, ctx->stream));
    HIP_TRY(hipMemsetAsync(bk.film.p, 0, bk.film.bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));                              // (`dev` has been read)
    return MCPT_OK;
}

mcpt_status mcpt_bake(mcpt_ctx* ctx, uint32_t spp, uint64_t seed, uint32_t first_sample) {
    const std::string who = "mcpt_bake: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!ctx->use_wavefront || ctx->lanes.empty()) return fail(MCPT_ERR_UNSUPPORTED, who + "needs the wavefront pipeline (MCPT_INTEGRATOR_MIS, no MCPT_PIPELINE=mega)");
    mcpt_ctx::Bake& bk = ctx->bk;
    const uint32_t n = bk.n();
    if (n == 0) return fail(MCPT_ERR_INVALID_ARG, who + "no bake points are set");
    if (uint64_t(first_sample) + spp > (1ull << 32)) return fail(MCPT_ERR_INVALID_ARG, who + "first_sample + spp exceeds 2^32");
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the first-hit kernel's traversal stack");
    if (spp == 0) return MCPT_OK;
    if (!bk.ray_o.p) HIP_TRY(alloc_all(Want(bk.ray_o, 3 * size_t(n), &ctx->info.device_bytes), Want(bk.ray_d, 3 * size_t(n), &ctx->info.device_bytes)));
    HIP_TRY(bk.take());                                                      // (the last call's last pass)
    bk.stage_ms = 0.0;
    st = timed_begin(ctx); if (st != MCPT_OK) return st;
    for (uint32_t k = 0; k < spp; k++) {
        const uint32_t s = first_sample + k;
        HIP_TRY(bk.take());
        HIP_TRY(bk.watch.begin(ctx->stream));
        HIP_TRY(launch_bk_rays(ctx->dev, bk.pts.p, n, s, uint32_t(seed), uint32_t(seed >> 32), bk.ray_o.p, bk.ray_d.p, bk.dead.p, ctx->stream));
        HIP_TRY(bk.watch.end(ctx->stream));
        // a primary hit emits from either side, a surface point must not see a lamp's back: where the ray first meets an emitter from behind, the
        // radiance the pass will add is taken out of the record beforehand (bk_unlit_kernel; still on the context's stream, ahead of the fork)
        // MCPT_BAKE_DIRECT_MIS: the direct-light kernel in its place -- the same traversal, the same correction, and the point's own light sample
        if (bk.direct == MCPT_BAKE_DIRECT_MIS)
            HIP_TRY(launch_bk_direct(ctx->dev, bk.pts.p, bk.ray_d.p, n, s, uint32_t(seed), uint32_t(seed >> 32), bk.film.p, ctx->stream));
        else
            HIP_TRY(launch_bk_unlit(ctx->dev, bk.ray_o.p, bk.ray_d.p, bk.dead.p, n, bk.film.p, ctx->stream));
        // as in mcpt_render_camera: the sub-pipelines' streams fork from the context's after the ray kernel and join it again, so the next pass's
        // kernel -- of this call or of the next one -- overwrites the rays only after this pass's paths have read them
        RenderParams p = probe_job_params(ctx, s, seed, ctx->opts.flags);
        p.probe_n = n; p.probe_o = bk.ray_o.p; p.probe_d = bk.ray_d.p;
        st = render_wavefront(ctx, p, bk.film.p); if (st != MCPT_OK) return st;
        bk.passes++;
    }
    bk.bakes++;
    return timed_end(ctx);
}

mcpt_status mcpt_clear_bake(mcpt_ctx* ctx) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (ctx->bk.film.bytes) HIP_TRY(hipMemsetAsync(ctx->bk.film.p, 0, ctx->bk.film.bytes, ctx->stream));
    return MCPT_OK;
}

mcpt_status mcpt_read_bake(mcpt_ctx* ctx, uint32_t mode, float* out4) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (mode > MCPT_BAKE_DIFFUSE) return fail(MCPT_ERR_INVALID_ARG, "mcpt_read_bake: unknown mode");
    const mcpt_ctx::Bake& bk = ctx->bk;
    if (bk.n() == 0) return MCPT_OK;
    if (!out4) return fail(MCPT_ERR_INVALID_ARG, "null output");
    {   Scratch s(ctx->stream); float4* d_out;
        HIP_TRY(s.out(size_t(bk.n()), &d_out));
        HIP_TRY(launch_bk_resolve(ctx->dev, bk.pts.p, bk.dead.p, bk.film.p, bk.n(), mode, d_out, ctx->stream));
        HIP_TRY(s.fetch(reinterpret_cast<float4*>(out4), d_out, size_t(bk.n()))); HIP_TRY(s.finish()); }
    return resolve_timing(ctx);
}

mcpt_status mcpt_read_bake_film(mcpt_ctx* ctx, float* out4) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (ctx->bk.n() == 0) return MCPT_OK;
    if (!out4) return fail(MCPT_ERR_INVALID_ARG, "null output");
    return read_back(ctx, out4, ctx->bk.film.p, ctx->bk.film.bytes);
}

mcpt_status mcpt_get_bake_info(mcpt_ctx* ctx, mcpt_bake_info* out) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    mcpt_ctx::Bake& bk = ctx->bk;
    Stopwatch none;                                                          // (a context that never had points has no watch of its own)
    HIP_TRY(bk.take());
    st = info_begin(ctx, out, bk.watch.ev0 ? &bk.watch : &none); if (st != MCPT_OK) return st;
    std::vector<uint8_t> dead(bk.n());
    st = read_back(ctx, dead.data(), bk.dead.p, dead.size(), false); if (st != MCPT_OK) return st;
    uint32_t n_dead = 0;
    for (uint8_t d : dead) n_dead += d ? 1u : 0u;
    out->n_points = bk.n(); out->n_dead = n_dead; out->bakes = bk.bakes; out->passes = bk.passes; out->last_stage_ms = bk.stage_ms; out->device_bytes = bk.device_bytes();
    out->direct_mode = bk.direct;
    return MCPT_OK;
}

mcpt_status mcpt_set_bake_direct(mcpt_ctx* ctx, uint32_t mode) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (mode > MCPT_BAKE_DIRECT_MIS) return fail(MCPT_ERR_INVALID_ARG, "mcpt_set_bake_direct: unknown mode");
    ctx->bk.direct = mode;                                                   // read by mcpt_bake when it enqueues a pass: nothing in flight depends on it
    return MCPT_OK;
}

mcpt_status mcpt_probe_bake_direct(mcpt_ctx* ctx, uint32_t sample, uint64_t seed, uint32_t first, uint32_t n, float* out12, int32_t* out4) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    const mcpt_ctx::Bake& bk = ctx->bk;
    if (uint64_t(first) + n > bk.n()) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_bake_direct: first + n exceeds the number of bake points set");
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the first-hit kernel's traversal stack");
    if (n == 0) return MCPT_OK;
    Scratch s(ctx->stream); float* d_f; int32_t* d_i;
    HIP_TRY(s.out(12 * size_t(n), &d_f)); HIP_TRY(s.out(4 * size_t(n), &d_i));
    HIP_TRY(launch_bk_direct_probe(ctx->dev, bk.pts.p, first, n, sample, uint32_t(seed), uint32_t(seed >> 32), d_f, d_i, ctx->stream));
    if (out12) HIP_TRY(s.fetch(out12, d_f, 12 * size_t(n)));
    if (out4) HIP_TRY(s.fetch(out4, d_i, 4 * size_t(n)));
    HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_probe_bake_rays(mcpt_ctx* ctx, uint32_t sample, uint64_t seed, uint32_t first, uint32_t n, double* out_origin3, double* out_dir3, double* out_normal3,
                                 uint8_t* out_dead) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    const mcpt_ctx::Bake& bk = ctx->bk;
    if (uint64_t(first) + n > bk.n()) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_bake_rays: first + n exceeds the number of bake points set");
    if (n == 0) return MCPT_OK;
    Scratch s(ctx->stream); double *d_o, *d_d, *d_n; uint8_t* d_dead;
    HIP_TRY(s.out(3 * size_t(n), &d_o)); HIP_TRY(s.out(3 * size_t(n), &d_d)); HIP_TRY(s.out(3 * size_t(n), &d_n)); HIP_TRY(s.out(size_t(n), &d_dead));
    HIP_TRY(launch_bk_probe(ctx->dev, bk.pts.p, first, n, sample, uint32_t(seed), uint32_t(seed >> 32), d_o, d_d, d_n, d_dead, ctx->stream));
    if (out_origin3) HIP_TRY(s.fetch(out_origin3, d_o, 3 * size_t(n)));
    if (out_dir3) HIP_TRY(s.fetch(out_dir3, d_d, 3 * size_t(n)));
    if (out_normal3) HIP_TRY(s.fetch(out_normal3, d_n, 3 * size_t(n)));
    if (out_dead) HIP_TRY(s.fetch(out_dead, d_dead, size_t(n)));
    HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_lightmap_points(const mcpt_scene_desc* scene, uint32_t width, uint32_t height, uint32_t capacity, mcpt_bake_point* out_points, uint32_t* out_texel,
                                 uint32_t* out_n) {
    const std::string who = "mcpt_lightmap_points: ";
    if (!scene || !out_n) return fail(MCPT_ERR_INVALID_ARG, who + "null argument");
    *out_n = 0;
    std::vector<mcpt_bake_point> points; std::vector<uint32_t> texel;
    const std::string bad = bk_lightmap_points(scene, width, height, points, texel);
    if (!bad.empty()) return fail(MCPT_ERR_INVALID_ARG, who + bad);
    *out_n = uint32_t(points.size());
    if (capacity < points.size()) return fail(MCPT_ERR_INVALID_ARG, who + "capacity < the number of covered texels");
    if (points.empty()) return MCPT_OK;
    if (!out_points || !out_texel) return fail(MCPT_ERR_INVALID_ARG, who + "null argument");
    std::memcpy(out_points, points.data(), points.size() * sizeof(mcpt_bake_point));
    std::memcpy(out_texel, texel.data(), texel.size() * sizeof(uint32_t));
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ light probes
mcpt_status mcpt_set_sh_probes(mcpt_ctx* ctx, const double* world_xyz, uint32_t n) {
    const std::string who = "mcpt_set_sh_probes: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    const std::string bad = sh_check_probes(world_xyz, n);
    if (!bad.empty()) return fail(MCPT_ERR_INVALID_ARG, who + bad);
    mcpt_ctx::ShProbes& sh = ctx->sh;
    // nothing below refuses; what fails is a HIP call
    st = use_drained(ctx); if (st != MCPT_OK) return st;                     // passes enqueued earlier read the buffers that are about to be replaced
    HIP_TRY(sh.take());
    if (n == 0) { sh.drop(); return MCPT_OK; }
    uint64_t* tally = &ctx->info.device_bytes;
    HIP_TRY(alloc_all(Want(sh.pos, 3 * size_t(n), tally), Want(sh.acc, SH_COEFFS * size_t(n), tally), Want(sh.counts, 3 * size_t(n), tally),
                      Want(sh.watch, 1, nullptr, !sh.watch.ev0)));
    if (sh.ray_o.p && sh.ray_o.count() != 3 * size_t(n) * SH_DIRS) sh.drop_pass();                      // (the first bake of the new list allocates its own)
    sh.have_pass = false;
    sh.host.assign(world_xyz, world_xyz + 3 * size_t(n));
    const std::vector<double> local = to_local(ctx, world_xyz, n);
    HIP_TRY(hipMemcpyAsync(sh.pos.p, local.data(), sh.pos.bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(sh.acc.p, 0, sh.acc.bytes, ctx->stream));
    HIP_TRY(hipMemsetAsync(sh.counts.p, 0, sh.counts.bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));                              // (`local` has been read)
    return MCPT_OK;
}

mcpt_status mcpt_bake_sh(mcpt_ctx* ctx, uint32_t passes, uint64_t seed, uint32_t first_sample) {
    const std::string who = "mcpt_bake_sh: ";
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!ctx->use_wavefront || ctx->lanes.empty()) return fail(MCPT_ERR_UNSUPPORTED, who + "needs the wavefront pipeline (MCPT_INTEGRATOR_MIS, no MCPT_PIPELINE=mega)");
    mcpt_ctx::ShProbes& sh = ctx->sh;
    const uint32_t n = sh.n(), items = sh.items();
    if (n == 0) return fail(MCPT_ERR_INVALID_ARG, who + "no probes are set");
    if (uint64_t(first_sample) + passes > (1ull << 32)) return fail(MCPT_ERR_INVALID_ARG, who + "first_sample + passes exceeds 2^32");
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the first-hit kernel's traversal stack");
    if (passes == 0) return MCPT_OK;
    if (!sh.ray_o.p) {
        uint64_t* tally = &ctx->info.device_bytes;
        HIP_TRY(alloc_all(Want(sh.ray_o, 3 * size_t(items), tally), Want(sh.ray_d, 3 * size_t(items), tally), Want(sh.film, size_t(items), tally), Want(sh.cls, size_t(items), tally)));
    }
    HIP_TRY(sh.take());                                                      // (the last call's last pass)
    sh.stage_ms = 0.0;
    st = timed_begin(ctx); if (st != MCPT_OK) return st;
    for (uint32_t k = 0; k < passes; k++) {
        const uint32_t s = first_sample + k;
        HIP_TRY(sh.take());
        HIP_TRY(sh.watch.begin(ctx->stream));
        HIP_TRY(launch_sh_rays(sh.pos.p, n, s, uint32_t(seed), uint32_t(seed >> 32), sh.ray_o.p, sh.ray_d.p, ctx->stream));
        // the pass's target is a scratch film, not the accumulators: the projection needs each item's own L.  Zeroed, then the first-hit kernel
        // takes an emitter's back out of it and classes the item (still on the context's stream, ahead of the fork)
        HIP_TRY(hipMemsetAsync(sh.film.p, 0, sh.film.bytes, ctx->stream));
        HIP_TRY(launch_sh_first_hit(ctx->dev, sh.ray_o.p, sh.ray_d.p, items, sh.film.p, sh.cls.p, ctx->stream));
        HIP_TRY(sh.watch.end(ctx->stream));
        RenderParams p = probe_job_params(ctx, s, seed, ctx->opts.flags);
        p.probe_n = items; p.probe_o = sh.ray_o.p; p.probe_d = sh.ray_d.p;
        st = render_wavefront(ctx, p, sh.film.p); if (st != MCPT_OK) return st;
        // render_wavefront has joined the context's stream: the projection reads the finished film, and the next pass's ray kernel -- of this call
        // or of the next one -- overwrites rays, film and classes only after it
        HIP_TRY(launch_sh_project(sh.film.p, sh.ray_d.p, sh.cls.p, n, sh.acc.p, sh.counts.p, ctx->stream));
        sh.passes++; sh.have_pass = true;
    }
    sh.bakes++;
    return timed_end(ctx);
}

mcpt_status mcpt_clear_sh(mcpt_ctx* ctx) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (ctx->sh.acc.bytes) {
        HIP_TRY(hipMemsetAsync(ctx->sh.acc.p, 0, ctx->sh.acc.bytes, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->sh.counts.p, 0, ctx->sh.counts.bytes, ctx->stream));
    }
    return MCPT_OK;
}

mcpt_status mcpt_read_sh(mcpt_ctx* ctx, uint32_t mode, float* out27) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (mode > MCPT_SH_IRRADIANCE) return fail(MCPT_ERR_INVALID_ARG, "mcpt_read_sh: unknown mode");
    const mcpt_ctx::ShProbes& sh = ctx->sh;
    if (sh.n() == 0) return MCPT_OK;
    if (!out27) return fail(MCPT_ERR_INVALID_ARG, "null output");
    {   Scratch s(ctx->stream); float* d_out;
        HIP_TRY(s.out(SH_COEFFS * size_t(sh.n()), &d_out));
        HIP_TRY(launch_sh_resolve(sh.acc.p, sh.counts.p, sh.n(), mode, d_out, ctx->stream));
        HIP_TRY(s.fetch(out27, d_out, SH_COEFFS * size_t(sh.n()))); HIP_TRY(s.finish()); }
    return resolve_timing(ctx);
}

mcpt_status mcpt_read_sh_film(mcpt_ctx* ctx, float* out27, uint32_t* out_counts3) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    const mcpt_ctx::ShProbes& sh = ctx->sh;
    if (sh.n() == 0) return MCPT_OK;
    if (out27) HIP_TRY(hipMemcpyAsync(out27, sh.acc.p, sh.acc.bytes, hipMemcpyDeviceToHost, ctx->stream));
    return read_back(ctx, out_counts3, sh.counts.p, out_counts3 ? sh.counts.bytes : 0);
}

mcpt_status mcpt_get_sh_info(mcpt_ctx* ctx, mcpt_sh_info* out) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!out) return fail(MCPT_ERR_INVALID_ARG, "null output");
    mcpt_ctx::ShProbes& sh = ctx->sh;
    Stopwatch none;                                                          // (a context that never had probes has no watch of its own)
    HIP_TRY(sh.take());
    st = info_begin(ctx, out, sh.watch.ev0 ? &sh.watch : &none); if (st != MCPT_OK) return st;
    out->n_probes = sh.n(); out->bakes = sh.bakes; out->passes = sh.passes; out->last_stage_ms = sh.stage_ms; out->device_bytes = sh.device_bytes();
    return MCPT_OK;
}

mcpt_status mcpt_probe_sh_rays(mcpt_ctx* ctx, uint32_t sample, uint64_t seed, uint32_t first_item, uint32_t n_items, double* out_origin3, double* out_dir3) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    const mcpt_ctx::ShProbes& sh = ctx->sh;
    if (uint64_t(first_item) + n_items > sh.items()) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_sh_rays: first_item + n_items exceeds 64 x the number of probes set");
    if (n_items == 0) return MCPT_OK;
    Scratch s(ctx->stream); double *d_o, *d_d;
    HIP_TRY(s.out(3 * size_t(n_items), &d_o)); HIP_TRY(s.out(3 * size_t(n_items), &d_d));
    HIP_TRY(launch_sh_probe(sh.pos.p, first_item, n_items, sample, uint32_t(seed), uint32_t(seed >> 32), d_o, d_d, ctx->stream));
    if (out_origin3) HIP_TRY(s.fetch(out_origin3, d_o, 3 * size_t(n_items)));
    if (out_dir3) HIP_TRY(s.fetch(out_dir3, d_d, 3 * size_t(n_items)));
    HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_read_sh_pass(mcpt_ctx* ctx, float* out_film4, uint8_t* out_class) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    const mcpt_ctx::ShProbes& sh = ctx->sh;
    if (!sh.have_pass) return fail(MCPT_ERR_INVALID_ARG, "mcpt_read_sh_pass: no pass has run for the probes set");
    if (out_film4) HIP_TRY(hipMemcpyAsync(out_film4, sh.film.p, sh.film.bytes, hipMemcpyDeviceToHost, ctx->stream));
    return read_back(ctx, out_class, sh.cls.p, out_class ? sh.cls.bytes : 0);
}

mcpt_status mcpt_sh_grid(const double* lo3, const double* hi3, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t capacity, double* out_xyz, uint32_t* out_n) {
    const std::string who = "mcpt_sh_grid: ";
    if (!out_n) return fail(MCPT_ERR_INVALID_ARG, who + "null argument");
    *out_n = 0;
    std::vector<double> xyz;
    const std::string bad = sh_grid_points(lo3, hi3, nx, ny, nz, xyz);
    if (!bad.empty()) return fail(MCPT_ERR_INVALID_ARG, who + bad);
    *out_n = uint32_t(xyz.size() / 3);
    if (capacity < xyz.size() / 3) return fail(MCPT_ERR_INVALID_ARG, who + "capacity < the number of cells");
    if (!out_xyz) return fail(MCPT_ERR_INVALID_ARG, who + "null argument");
    std::memcpy(out_xyz, xyz.data(), xyz.size() * sizeof(double));
    return MCPT_OK;
}

mcpt_status mcpt_sh_eval(const float* coeffs27, const double* normal3, double* out_rgb3) {
    if (!coeffs27 || !normal3 || !out_rgb3) return fail(MCPT_ERR_INVALID_ARG, "mcpt_sh_eval: null argument");
    sh_eval_probe(coeffs27, normal3, out_rgb3);
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ probes
mcpt_status mcpt_probe_trace(mcpt_ctx* ctx, uint32_t n, const double* origin, const double* dir, const double* t1, const double* t2, int any_hit,
                             float* out_t, int32_t* out_tri, float* out_u, float* out_v) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!origin || !dir || !t1 || !t2 || !out_t || !out_tri || !out_u || !out_v) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary cross-check tree of this (device-built) scene is deeper than its kernels' stack: use mcpt_probe_trace4");
    if (n == 0) return MCPT_OK;
    Scratch s(ctx->stream); double *d_o, *d_d, *d_t1, *d_t2; float *d_t, *d_u, *d_v; int* d_tri;
    HIP_TRY(s.in(s.keep(to_local(ctx, origin, n)), 3 * size_t(n), &d_o)); HIP_TRY(s.in(dir, 3 * size_t(n), &d_d)); HIP_TRY(s.in(t1, n, &d_t1)); HIP_TRY(s.in(t2, n, &d_t2));
    HIP_TRY(s.out(n, &d_t)); HIP_TRY(s.out(n, &d_tri)); HIP_TRY(s.out(n, &d_u)); HIP_TRY(s.out(n, &d_v));
    HIP_TRY(launch_probe_trace(ctx->dev, n, d_o, d_d, d_t1, d_t2, any_hit, d_t, d_tri, d_u, d_v, ctx->stream));
    HIP_TRY(s.fetch(out_t, d_t, n)); HIP_TRY(s.fetch(out_tri, d_tri, n)); HIP_TRY(s.fetch(out_u, d_u, n)); HIP_TRY(s.fetch(out_v, d_v, n)); HIP_TRY(s.finish());
    return MCPT_OK;
}

// The PRODUCTION traversal: the caller's rays are written into a path pool exactly as wf_shade_kernel would leave them (extend rays
// in ray_o / ray_d, shadow rays as sq_o / sq_d records of the per-block shadow queue), wf_trace8_kernel runs once over that pool, and the results
// are read back from where wf_shade_kernel would pick them up (pool.hit; for shadow rays the L += nee the unoccluded ones perform).
mcpt_status mcpt_probe_trace4(mcpt_ctx* ctx, uint32_t n, const double* origin, const double* dir, const double* t2, int any_hit,
                              float* out_t, int32_t* out_tri, float* out_u, float* out_v) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!origin || !dir || !out_t || !out_tri || !out_u || !out_v || (any_hit && !t2)) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (!ctx->use_wavefront || ctx->lanes.empty()) return fail(MCPT_ERR_UNSUPPORTED, "mcpt_probe_trace4 needs the wavefront pipeline (MIS integrator)");
    if (n == 0) return MCPT_OK;
    mcpt_ctx::WfLane& L = ctx->lanes[0];
    const uint32_t P = uint32_t(((uint64_t(n) + WF_SHADE_BLOCK - 1) / WF_SHADE_BLOCK) * WF_SHADE_BLOCK);
    if (P > ctx->knobs.pool_cap) return fail(MCPT_ERR_UNSUPPORTED, "mcpt_probe_trace4: more rays than pool slots");
    st = ensure_pool(ctx, L, P); if (st != MCPT_OK) return st;
    PathPool pool = L.pool;
    pool.P = P;
    Scratch s(ctx->stream);                                           // (holds the host arrays until the stream has used them; the device side is the sub-pipeline's pool)
    const size_t P4 = 4 * size_t(P), nb = P / WF_SHADE_BLOCK;
    float *ro = s.keep(std::vector<float>(P4, 0.f)), *rd = s.keep(std::vector<float>(P4, 0.f)), *sd = s.keep(std::vector<float>(P4, 0.f)), *hit = s.keep(std::vector<float>(P4, 0.f));
    uint32_t *queue = s.keep(std::vector<uint32_t>(P, 0u)), *qcount = s.keep(std::vector<uint32_t>(nb, 0u));
    IterCtl* ctl0 = s.keep(std::vector<IterCtl>(1));                  // all zero but "iteration 0 left live slots": the trace kernel returns at once otherwise
    ctl0->any_active[0] = 1u;
    const int32_t no_skip = -1; float no_skip_f; std::memcpy(&no_skip_f, &no_skip, 4);
    for (uint32_t i = 0; i < P; i++) {
        float* o4 = &ro[4 * size_t(i)]; float* d4 = &rd[4 * size_t(i)]; float* s4 = &sd[4 * size_t(i)];
        o4[3] = no_skip_f; d4[2] = 1.f; s4[2] = 1.f;
        if (i >= n) continue;
        // a closest-hit ray with an all-zero direction stands for "this slot has no pending extend ray" (reported as a miss), like a dead slot of a
        // job that is running out: the trace kernel must look past it
        if (!any_hit && dir[3 * size_t(i)] == 0.0 && dir[3 * size_t(i) + 1] == 0.0 && dir[3 * size_t(i) + 2] == 0.0) continue;
        for (int k = 0; k < 3; k++) { o4[k] = float(origin[3 * size_t(i) + k] - ctx->dev.centre[k]); d4[k] = float(dir[3 * size_t(i) + k]); s4[k] = d4[k]; }
        if (any_hit) {
            s4[3] = t2[i] > 3.0e38 ? 3.0e38f : float(t2[i]);
            queue[i] = i;                                               // shade block b queues its own slots in order
            qcount[i / WF_SHADE_BLOCK]++;
        } else { const uint32_t one = 1u; std::memcpy(&d4[3], &one, 4); }   // bit 0 of ray_d.w: "an extend ray is pending"
    }
    HIP_TRY(s.put(pool.ray_o, ro, P4)); HIP_TRY(s.put(pool.ray_d, rd, P4)); HIP_TRY(s.put(pool.sq_d, sd, P4)); HIP_TRY(s.put(pool.sq_o, ro, P4));   // queue entry i = slot i
    HIP_TRY(s.fill(pool.hit, 0xff, size_t(P) * 16));
    HIP_TRY(s.fill(pool.nee, 0, size_t(P) * 16));                    // nee.w == 0 afterwards <=> the trace kernel did not flag the ray as blocked
    HIP_TRY(s.put(pool.shadow_queue, queue, P)); HIP_TRY(s.put(pool.shadow_count, qcount, nb));
    HIP_TRY(s.put(L.ctl_buf.p, ctl0, 1));
    const bool count = (ctx->opts.flags & MCPT_FLAG_COUNT_TRAVERSAL) != 0;
    HIP_TRY(launch_wf_trace(ctx->dev, pool, L.ctl_buf.p, 0u, ctx->tune, count, ctx->counters.p, ctx->trace_grid, L.ovf_buf.p, ctx->stream));
    {   IterCtl snap; st = read_back(ctx, &snap, L.ctl_buf.p, sizeof snap, false); if (st != MCPT_OK) return st;
        if (job_state(snap, 0u, 0u) == JobState::Watchdog) return fail(MCPT_ERR_HIP, WATCHDOG_MSG); }
    if (any_hit) {
        st = read_back(ctx, hit, pool.nee, P4 * 4, false); if (st != MCPT_OK) return st;     // blocked <=> the trace kernel set nee.w
        for (uint32_t i = 0; i < n; i++) {
            uint32_t flag; std::memcpy(&flag, &hit[4 * size_t(i) + 3], 4);
            out_tri[i] = flag ? 1 : 0; out_t[i] = 0.f; out_u[i] = 0.f; out_v[i] = 0.f;
        }
    } else {
        st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
        st = read_back(ctx, hit, pool.hit, P4 * 4, false); if (st != MCPT_OK) return st;
        for (uint32_t i = 0; i < n; i++) {
            int32_t tri; std::memcpy(&tri, &hit[4 * size_t(i)], 4);
            if (tri >= 0) tri &= HIT_TRI_MASK;                          // the upper bits carry the hit's lobe class for the shade kernel
            if (tri >= ctx->dev.n_tris) return fail(MCPT_ERR_HIP, "mcpt_probe_trace4: trace kernel returned an out-of-range triangle");
            out_tri[i] = tri < 0 ? -1 : ctx->h_tri_face[size_t(tri)];
            out_u[i] = tri < 0 ? 0.f : hit[4 * size_t(i) + 1]; out_v[i] = tri < 0 ? 0.f : hit[4 * size_t(i) + 2]; out_t[i] = tri < 0 ? 0.f : hit[4 * size_t(i) + 3];
        }
    }
    return MCPT_OK;
}

mcpt_status mcpt_probe_cast_ray(mcpt_ctx* ctx, uint32_t n, const int32_t* xy, const float* xi, float* out6) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!xy || !xi || !out6) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (n == 0) return MCPT_OK;
    Scratch s(ctx->stream); int* d_xy; float *d_xi, *d_out;
    HIP_TRY(s.in(xy, 2 * size_t(n), &d_xy)); HIP_TRY(s.in(xi, 2 * size_t(n), &d_xi)); HIP_TRY(s.out(6 * size_t(n), &d_out));
    HIP_TRY(launch_probe_cast_ray(ctx->dev, n, d_xy, d_xi, d_out, ctx->stream));
    HIP_TRY(s.fetch(out6, d_out, 6 * size_t(n))); HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_probe_hit_shade(mcpt_ctx* ctx, uint32_t n, const int32_t* face, const float* u, const float* v, const double* dir, float* out6) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!face || !u || !v || !dir || !out6) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (n == 0) return MCPT_OK;
    st = fetch_tri_face(ctx); if (st != MCPT_OK) return st;
    std::vector<int32_t> leaf_of_face(ctx->h_tri_face.size(), -1), tri(n);
    for (size_t i = 0; i < ctx->h_tri_face.size(); i++) leaf_of_face[size_t(ctx->h_tri_face[i])] = int32_t(i);
    for (uint32_t i = 0; i < n; i++) {
        if (face[i] < 0 || size_t(face[i]) >= leaf_of_face.size()) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_hit_shade: face index out of range");
        tri[i] = leaf_of_face[size_t(face[i])];
    }
    Scratch s(ctx->stream); int* d_tri; float *d_u, *d_v, *d_out; double* d_d;
    HIP_TRY(s.in(s.keep(std::move(tri)), n, &d_tri)); HIP_TRY(s.in(u, n, &d_u)); HIP_TRY(s.in(v, n, &d_v)); HIP_TRY(s.in(dir, 3 * size_t(n), &d_d)); HIP_TRY(s.out(6 * size_t(n), &d_out));
    HIP_TRY(launch_probe_hit_shade(ctx->dev, n, d_tri, d_u, d_v, d_d, d_out, ctx->stream));
    HIP_TRY(s.fetch(out6, d_out, 6 * size_t(n))); HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_probe_bsdf(mcpt_ctx* ctx, uint32_t n, const float* normal, const float* wi, const float* kd, const float* ks, const float* ns,
                            const float* wo, const float* xi, float* out12) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!normal || !wi || !kd || !ks || !ns || !wo || !xi || !out12) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (n == 0) return MCPT_OK;
    Scratch s(ctx->stream); float *d_n, *d_wi, *d_kd, *d_ks, *d_ns, *d_wo, *d_xi, *d_out;
    HIP_TRY(s.in(normal, 3 * size_t(n), &d_n)); HIP_TRY(s.in(wi, 3 * size_t(n), &d_wi)); HIP_TRY(s.in(kd, 3 * size_t(n), &d_kd));
    HIP_TRY(s.in(ks, 3 * size_t(n), &d_ks)); HIP_TRY(s.in(ns, n, &d_ns)); HIP_TRY(s.in(wo, 3 * size_t(n), &d_wo)); HIP_TRY(s.in(xi, 3 * size_t(n), &d_xi));
    HIP_TRY(s.out(12 * size_t(n), &d_out));
    HIP_TRY(launch_probe_bsdf(n, d_n, d_wi, d_kd, d_ks, d_ns, d_wo, d_xi, d_out, ctx->stream));
    HIP_TRY(s.fetch(out12, d_out, 12 * size_t(n))); HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_probe_sample_light(mcpt_ctx* ctx, uint32_t n, const double* point, const float* xi, float* out10) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!point || !xi || !out10) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (n == 0) return MCPT_OK;
    Scratch s(ctx->stream); double* d_p; float *d_xi, *d_out;
    HIP_TRY(s.in(s.keep(to_local(ctx, point, n)), 3 * size_t(n), &d_p)); HIP_TRY(s.in(xi, 3 * size_t(n), &d_xi)); HIP_TRY(s.out(10 * size_t(n), &d_out));
    HIP_TRY(launch_probe_sample_light(ctx->dev, n, d_p, d_xi, d_out, ctx->stream));
    HIP_TRY(s.fetch(out10, d_out, 10 * size_t(n))); HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_probe_paths(mcpt_ctx* ctx, uint32_t n, const double* origin, const double* dir, uint64_t seed, float* out_L3) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!origin || !dir || !out_L3) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (n == 0) return MCPT_OK;
    if (ctx->opts.integrator != MCPT_INTEGRATOR_MIS) return fail(MCPT_ERR_UNSUPPORTED, "mcpt_probe_paths drives the MIS integrator only");
    Scratch s(ctx->stream); double *d_o, *d_d; float* d_out; DevCounters* d_cnt;
    HIP_TRY(s.in(s.keep(to_local(ctx, origin, n)), 3 * size_t(n), &d_o)); HIP_TRY(s.in(dir, 3 * size_t(n), &d_d)); HIP_TRY(s.out(3 * size_t(n), &d_out)); HIP_TRY(s.out(1, &d_cnt));
    RenderParams p = probe_job_params(ctx, 0u, seed, ctx->opts.flags & ~MCPT_FLAG_COUNT_TRAVERSAL);
    if (ctx->use_wavefront) {
        // the production pipeline: [wf_shade, wf_trace] iterations over the path pool, item i = entry i of an n x 1 film
        if (n > 0x3ffffffu) return fail(MCPT_ERR_UNSUPPORTED, "mcpt_probe_paths: too many paths for one call");
        float4* d_film = nullptr;
        HIP_TRY(s.out(size_t(n), &d_film));
        p.probe_n = n; p.probe_o = d_o; p.probe_d = d_d;
        st = render_wavefront(ctx, p, d_film); if (st != MCPT_OK) return st;
        float* film = s.keep(std::vector<float>(4 * size_t(n)));
        HIP_TRY(s.fetch(film, d_film, 4 * size_t(n)));
        HIP_TRY(s.finish());
        for (auto& L : ctx->lanes) { L.last_iterations = 0; L.last_timed = 0; }
        for (uint32_t i = 0; i < n; i++) {
            if (film[4 * size_t(i) + 3] != 1.f) return fail(MCPT_ERR_HIP, "mcpt_probe_paths: a probe path did not finish exactly once");
            for (int k = 0; k < 3; k++) out_L3[3 * size_t(i) + k] = film[4 * size_t(i) + k];
        }
        return MCPT_OK;
    }
    if (!ctx->binary_ok) return fail(MCPT_ERR_BVH_DEPTH, "the binary tree of this (device-built) scene is deeper than the megakernel's traversal stack");
    HIP_TRY(launch_probe_paths(ctx->dev, p, n, d_o, d_d, d_out, d_cnt, ctx->stream));
    HIP_TRY(s.fetch(out_L3, d_out, 3 * size_t(n))); HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_probe_texture(mcpt_ctx* ctx, uint32_t material, uint32_t n, const float* uv2, float* out_rgb3) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!uv2 || !out_rgb3) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (material >= uint32_t(ctx->dev.n_mats)) return fail(MCPT_ERR_INVALID_ARG, "material index out of range");
    if (n == 0) return MCPT_OK;
    for (size_t i = 0; i < 2 * size_t(n); i++)
        if (!std::isfinite(uv2[i])) return fail(MCPT_ERR_INVALID_ARG, "mcpt_probe_texture: uv is not finite");    // (int)(NaN * tex_w) is undefined; a scene's own uv are finite
    Scratch s(ctx->stream); float *d_uv, *d_out;
    HIP_TRY(s.in(uv2, 2 * size_t(n), &d_uv)); HIP_TRY(s.out(3 * size_t(n), &d_out));
    HIP_TRY(launch_probe_texture(ctx->dev, int(material), n, d_uv, d_out, ctx->stream));
    HIP_TRY(s.fetch(out_rgb3, d_out, 3 * size_t(n))); HIP_TRY(s.finish());
    return MCPT_OK;
}

mcpt_status mcpt_probe_rng(mcpt_ctx* ctx, uint32_t n, const uint32_t* key3, uint64_t seed, float* out4) {
    mcpt_status st = use(ctx); if (st != MCPT_OK) return st;
    if (!key3 || !out4) return fail(MCPT_ERR_INVALID_ARG, "null argument");
    if (n == 0) return MCPT_OK;
    Scratch s(ctx->stream); uint32_t* d_k; float* d_out;
    HIP_TRY(s.in(key3, 3 * size_t(n), &d_k)); HIP_TRY(s.out(4 * size_t(n), &d_out));
    HIP_TRY(launch_probe_rng(n, d_k, uint32_t(seed), uint32_t(seed >> 32), d_out, ctx->stream));
    HIP_TRY(s.fetch(out4, d_out, 4 * size_t(n))); HIP_TRY(s.finish());
    return MCPT_OK;
}

}  // extern "C"
