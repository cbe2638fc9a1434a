// The wavefront scheduler's DECISIONS: what a render call's shape (tiles, samples, sub-pipelines, knobs) makes of it, as data and pure functions.
// Nothing here touches a device, the HIP runtime, a context or the environment (wavefront.h is included for RenderParams and the block
// constants): tests/wf_plan_check.cpp runs every plan on the CPU, tests/wf_interlock_check.cpp the shade interlock's decisions.  mcpt_api.cpp executes a plan.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/mcpt.h"
#include "wavefront.h"

constexpr uint32_t WF_INTERLOCK_DEFAULT = 1;      // MCPT_WF_INTERLOCK where it is unset (the measurement behind it)

// What the scheduler takes from the environment (developer knobs): read ONCE per context, by wf_read_knobs.
struct WfKnobs {
    uint32_t pool_cap;                 // most slots a sub-pipeline's pool may have (MCPT_WF_POOL_LOG2, _SLOTS); pools are allocated on first use, sized to the job
    uint32_t items_per_slot;           // pool sizing: a job of n work items gets n / items_per_slot slots, at most pool_cap (MCPT_WF_ITEMS_PER_SLOT), see wf_plan_call
    bool private_items, small_job_split, compact, debug;   // MCPT_WF_PRIVATE_ITEMS, _SMALL_JOB_SPLIT (both: wf_plan_call), _COMPACT (drain compaction), _DEBUG (snapshots on stderr)
    uint32_t compact_eighths, max_it;  // MCPT_WF_COMPACT_EIGHTHS: compact when at most this many eighths of the swept slots are alive; MCPT_WF_MAXIT: iteration cap of the host loop
    uint32_t time_kernels;             // MCPT_TIME_KERNELS=N: bracket the two kernels of every Nth iteration with HIP events (0 = off)
    bool interlock;                    // MCPT_WF_INTERLOCK: the sub-pipelines' shade launches run one after the other (wf_shade_wait)
};
template <class Env> WfKnobs wf_read_knobs(Env env) {      // env(name, default): the variable as a number, the default where it is unset
    WfKnobs k;
    k.pool_cap = 1u << std::min(26u, uint32_t(env("MCPT_WF_POOL_LOG2", 23)));
    k.pool_cap = uint32_t(env("MCPT_WF_POOL_SLOTS", k.pool_cap)) & ~uint32_t(16 * WF_SHADE_BLOCK - 1);   // (any multiple of 4096 slots)
    if (k.pool_cap < 4096) k.pool_cap = 4096;
    k.items_per_slot = std::max(1u, uint32_t(env("MCPT_WF_ITEMS_PER_SLOT", 1)));
    k.private_items = env("MCPT_WF_PRIVATE_ITEMS", 1) != 0; k.small_job_split = env("MCPT_WF_SMALL_JOB_SPLIT", 1) != 0;
    k.compact = env("MCPT_WF_COMPACT", 1) != 0; k.compact_eighths = std::max(1u, std::min(7u, uint32_t(env("MCPT_WF_COMPACT_EIGHTHS", 4))));
    k.max_it = env("MCPT_WF_MAXIT", 1u << 20); k.debug = env("MCPT_WF_DEBUG", 0) != 0; k.time_kernels = env("MCPT_TIME_KERNELS", 0);
    k.interlock = env("MCPT_WF_INTERLOCK", WF_INTERLOCK_DEFAULT) != 0;
    return k;
}

// One render call before it is shared out: spp >= 1 samples of the tiles (tile_mod, tile_rem) selects among `all` (the film's tiles, or the
// entries of a tile list).  Fills all of `p` that follows from these; the caller adds the film's tiles_x / tiles_y and the list pointer.
enum class WfCall { Nothing, TooLarge, Go };      // Nothing: more shards than tiles, none for this one.  TooLarge: the item count leaves the cursors' range
inline WfCall wf_plan_params(RenderParams& p, uint64_t all, uint32_t tile_mod, uint32_t tile_rem, uint32_t spp, uint32_t first_sample, uint64_t seed,
                             const mcpt_opts& o, bool use_wavefront) {
    memset(&p, 0, sizeof p);
    p.spp = spp; p.first_sample = first_sample;
    p.tile_mod = tile_mod; p.tile_rem = tile_rem;
    p.n_owned = all > tile_rem ? uint32_t((all - tile_rem + tile_mod - 1) / tile_mod) : 0u;
    if (p.n_owned == 0) return WfCall::Nothing;
    const uint64_t tiles = p.n_owned;
    uint32_t spi = o.samples_per_item;
    if (o.flags & MCPT_FLAG_DETERMINISTIC) spi = spp;               // one lane owns a pixel for the whole call
    else if (spi == 0) {
        if (use_wavefront) {
            // auto: one sample per item, longer ones only to keep the item count in the cursors' range.  Short items keep the end-of-render
            // drain short (a slot works its item off sample after sample: 8-sample items cost 2.7 % at 1024 spp on the bench workload).
            // Rounds 1-2 also grew the items when many pool slots would share a film pixel (more than 32 per pixel), for fear of the film's
            // float atomics; measured in round 3 that rule was the problem, not the atomics: 64 x 64 x 4096 spp 88 -> 17 ms without it
            // (4 096 slots per pixel), 16 x 16 x 16 384 spp 49 -> 9 ms, 256 x 256 x 1024 spp 60 -> 51 ms, and an interleaved-tile share of
            // the bench job (1/8 of the pixels) 72 -> 58 ms -- the atomics execute at the memory side and 10^4 adders per address are fine.
            spi = 1;
            while (tiles * ((spp + spi - 1) / spi) > 0x3ffffffull && spi < spp) spi <<= 1;
        } else {
            // megakernel: long enough that per-item overheads vanish, short enough that the work balances across the chip
            spi = 64;
            const uint64_t want_items = 256ull * 16 * 16;
            while (spi > 8 && tiles * ((spp + spi - 1) / spi) < want_items) spi >>= 1;
        }
    }
    if (spi > spp) spi = spp;
    p.samples_per_item = spi; p.chunks = (spp + spi - 1) / spi;
    p.atomic_accum = p.chunks > 1 ? 1u : 0u;
    p.max_depth = o.max_depth; p.flags = o.flags; p.integrator = o.integrator;
    p.seed_lo = uint32_t(seed); p.seed_hi = uint32_t(seed >> 32);
    return tiles * p.chunks > 0x3ffffffull ? WfCall::TooLarge : WfCall::Go;
}

struct WfLanePlan {             // one sub-pipeline's share of a call
    bool active = false;       // false: its sample range is empty (fewer samples than sub-pipelines and too few tiles to split)
    RenderParams p;            // what its shade launches get
    uint32_t n_items = 0, n_shared = 0;   // work items; those of them handed out through the shared cursors
    uint32_t P = 0, bound = 0; // pool slots it sweeps (and needs); known-length job: its iteration count, 0 = polled
    uint32_t grid = 0;         // blocks of its trace launches at the start of the job
};
struct WfPlan {
    std::vector<WfLanePlan> lanes;
    uint32_t n_active = 0; bool split_tiles = false;
    uint32_t small_job = 0, shared_grid = 1;   // a sweep of at most small_job slots (0 = none) takes shared_grid trace blocks
};

// One call = per sub-pipeline a loop of [shade, trace] launches over its slot pool until its work items are done.  The sample range is split
// contiguously over the sub-pipelines.  trace_grid: blocks of a full trace launch.
inline WfPlan wf_plan_call(const RenderParams& p0, uint32_t n_lanes, const WfKnobs& knobs, uint32_t trace_grid, uint32_t trace_block_threads) {
    const uint64_t tiles = p0.n_owned;
    if (p0.probe_n) n_lanes = 1;                                          // a probe (mcpt_probe_paths) runs on one sub-pipeline
    WfPlan plan; plan.lanes.resize(n_lanes);
    // A call with fewer samples than sub-pipelines (the reference's one-sample-per-call loop, Render.cpp:56-69) splits its TILES over them
    // instead of its samples -- pipeline k takes every n_lanes-th tile of this call's share -- so that the shade of one still runs
    // beside the trace of the other.  Their pixel sets are disjoint.
    plan.split_tiles = !p0.probe_n && p0.spp < n_lanes && tiles >= n_lanes;
    for (uint32_t k = 0; k < n_lanes; k++) {
        WfLanePlan& r = plan.lanes[k];
        r.p = p0;
        uint64_t my_tiles = tiles;
        if (plan.split_tiles) {
            r.p.tile_mod = p0.tile_mod * n_lanes; r.p.tile_rem = p0.tile_rem + k * p0.tile_mod;
            my_tiles = (tiles - k + n_lanes - 1) / n_lanes; r.p.n_owned = uint32_t(my_tiles);
        } else {
            const uint32_t lo = uint32_t(uint64_t(p0.spp) * k / n_lanes), hi = uint32_t(uint64_t(p0.spp) * (k + 1) / n_lanes);   // (equal shares: 40 / 60 and 35 / 65 splits, so that the two pools do not drain together, were 6 - 10 % slower)
            if (hi == lo) continue;
            r.p.spp = hi - lo; r.p.first_sample = p0.first_sample + lo;
        }
        if (r.p.samples_per_item > r.p.spp) r.p.samples_per_item = r.p.spp;
        r.p.chunks = (r.p.spp + r.p.samples_per_item - 1) / r.p.samples_per_item;
        r.n_items = p0.probe_n ? p0.probe_n : uint32_t(my_tiles * 64 * r.p.chunks);
        // Pool slots for this job: one per work item, at most pool_cap (2^23 by default).  (items_per_slot, a developer knob, default 1: a job of more
        // than 2^20 items gets items / items_per_slot slots, at least 2^20 -- what a slot costs is the end-of-job drain, the last ~8 iterations sweep a
        // pool that is emptying; measured in round 3, fewer slots than the job can fill lose more in short launches than they save in the drain.)
        const uint64_t want64 = ((uint64_t(r.n_items) + WF_SHADE_BLOCK - 1) / WF_SHADE_BLOCK) * WF_SHADE_BLOCK;
        uint64_t P = std::min<uint64_t>(want64, knobs.pool_cap);
        if (want64 > (1ull << 20)) {
            const uint64_t by_items = ((uint64_t(r.n_items) / knobs.items_per_slot) + 16 * WF_SHADE_BLOCK - 1) & ~uint64_t(16 * WF_SHADE_BLOCK - 1);   // (rounded UP: a job just over 2^20 items keeps one slot per item and its known length)
            P = std::min<uint64_t>(P, std::max<uint64_t>(by_items, 1ull << 20));
        }
        r.P = uint32_t(P);                                                // (a smaller job sweeps only the slots it needs)
        // Every item has a slot of its own and one sample: all paths start in iteration 0, vertex b is shaded in iteration b + 1, the
        // depth limit ends the path by iteration max_depth + 1 and a parked NEE term (SLOT_DRAIN) costs one more.  The loop then runs
        // exactly that many iterations before it looks at the control block for the first time -- no launches past the end of the job.
        if (r.n_items <= r.P && r.p.chunks == 1 && r.p.samples_per_item == 1 && p0.max_depth != 0 && !p0.probe_n) r.bound = p0.max_depth + 3;
        // Work items: 90 % are split evenly into one private range per shade block -- the block advances a cursor only it touches, so
        // the returning atomic that used to sit between two barriers of every block is gone from the steady state -- and the last
        // 10 % still come from the shared cursors, which is what balances the blocks at the end of the call.
        r.p.priv_items = 0; r.p.shared_base = 0; r.n_shared = r.n_items;
        const uint32_t n_blocks = r.P / WF_SHADE_BLOCK;
        if (!p0.probe_n && uint64_t(r.n_items) >= 4ull * r.P && knobs.private_items) {
            r.p.priv_items = uint32_t(0.9 * double(r.n_items) / double(n_blocks)) & ~63u;   // whole 64-item units (block b owns unit k * n_blocks + b)
            r.p.shared_base = n_blocks * r.p.priv_items;
            r.n_shared = r.n_items - r.p.shared_base;
        }
        r.active = true; plan.n_active++;
    }
    for (WfLanePlan& r : plan.lanes) if (r.active) r.p.atomic_accum = ((plan.n_active > 1 && !plan.split_tiles) || r.p.chunks > 1) ? 1u : 0u;
    // Trace grid.  A CU holds ONE trace block (registers), so the trace launches of two sub-pipelines queue for each other's CUs.  That is what the steady
    // state wants (the other pipeline's SHADE runs beside a trace launch); a job with about a ray per trace lane -- the one-sample frame of the reference's
    // display loop: 320 k paths per sub-pipeline, 262 k trace lanes -- has nothing to hide and is a chain of 2 x (depth + 3) dependent launches: there each
    // sub-pipeline's launch takes its share of the CUs and the chains run side by side.  S-cornell 800x800, render + tonemapped read per frame: 2.43 -> 2.06 ms;
    // two samples per call 2.83 -> 2.76, four 3.95 -> 4.73 (profiles/r04_frame_knobs.txt): the split applies up to 2.5 paths per trace lane.  The same holds
    // at the end of a long job once the drain compaction has shrunk the sweep that far (mcpt_api.cpp: wf_poll).
    plan.small_job = knobs.small_job_split && plan.n_active > 1 ? uint32_t(std::min<uint64_t>(0xffffffffull, uint64_t(trace_grid) * trace_block_threads * 5 / 2)) : 0u;
    plan.shared_grid = std::max(1u, trace_grid / std::max(1u, plan.n_active));
    for (WfLanePlan& r : plan.lanes) if (r.active) r.grid = (plan.small_job && !p0.probe_n && r.n_items <= plan.small_job) ? plan.shared_grid : trace_grid;
    return plan;
}

// The shade interlock.  Left alone, the sub-pipelines fall into step: their shade launches run beside each other (VALUs waiting on HBM) and then their
// trace launches queue for each other's CUs with no shade beside them.  With the interlock the shade launches of the gated sub-pipelines
// run strictly one after the other, in the round-robin order in which the executor enqueues them: the shade launch of sub-pipeline k waits (on k's stream)
// for an event recorded right after the shade launch enqueued just before it, which belongs to the previous gated sub-pipeline in round order.  Each
// sub-pipeline's trace launch then sits between its own two shade launches, i.e. beside the other's shade.  Trace launches are never gated: a queued trace
// launch takes CUs as the other's blocks retire, which keeps the tail of one overlapped with the head of the next.
// No deadlock: a wait only ever names `last`, the sub-pipeline whose event the executor recorded most recently -- earlier in host enqueue order.
struct WfLaneState { bool done; uint32_t grid; };   // what the executor knows of a running sub-pipeline: its job has finished; blocks of its trace launches now
constexpr int WF_NO_LANE = -1;
// the call as a whole: off for a single active sub-pipeline, a probe and deterministic mode
inline bool wf_interlock_call(const WfPlan& plan, const RenderParams& p0, const WfKnobs& knobs) {
    return knobs.interlock && plan.n_active >= 2 && !p0.probe_n && !(p0.flags & MCPT_FLAG_DETERMINISTIC);
}
// one sub-pipeline: gated while it is live, polled (a known-length job is enqueued whole and not waited for), on the full trace grid (on shared_grid --
// a small job, or a draining one after wf_poll saw its compacted sweep -- the chains run side by side by design) and working off more items than it has
// slots.  A job with a slot per item starts every path in iteration 0 and only drains from there: a chain of dependent launches that get shorter, no
// steady state to put in order (the display loop's 4-sample call, 800 x 800: 3.95 ms without the interlock, 4.16 ms with).  It records its event iff it is gated.
inline bool wf_lane_gated(const WfPlan& plan, const RenderParams& p0, const WfKnobs& knobs, uint32_t k, WfLaneState s) {
    const WfLanePlan& lp = plan.lanes[k];
    return wf_interlock_call(plan, p0, knobs) && lp.active && !s.done && lp.bound == 0 && lp.n_items > lp.P && s.grid != plan.shared_grid;
}
// The sub-pipeline whose latest shade event the next shade launch of sub-pipeline k waits for, or WF_NO_LANE.  state_of(j): WfLaneState of sub-pipeline j;
// last: the sub-pipeline that recorded the latest shade event of this call (WF_NO_LANE: none yet).  A sub-pipeline that has finished or left the full grid
// since it recorded is not waited for: the chain is broken for that one launch, which may run beside an earlier shade launch, and is formed again by the next.
template <class StateOf> int wf_shade_wait(const WfPlan& plan, const RenderParams& p0, const WfKnobs& knobs, uint32_t k, StateOf state_of, int last) {
    if (!wf_lane_gated(plan, p0, knobs, k, state_of(k))) return WF_NO_LANE;
    uint32_t gated = 0;
    for (uint32_t j = 0; j < plan.lanes.size(); j++) gated += wf_lane_gated(plan, p0, knobs, j, state_of(j));
    if (gated < 2 || last < 0 || uint32_t(last) == k || !wf_lane_gated(plan, p0, knobs, uint32_t(last), state_of(uint32_t(last)))) return WF_NO_LANE;
    return last;
}
