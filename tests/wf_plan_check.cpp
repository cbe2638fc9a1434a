// CPU check of the wavefront scheduler's plans (csrc/wf_plan.h: wf_read_knobs, wf_plan_params, wf_plan_call): a sweep of call shapes, and on
// every plan the invariants the kernels rely on -- each (tile, sample) of the call is rendered exactly once, pools fit, known-length jobs
// are known-length, the work-item hand-out adds up, film atomics are on wherever two writers can meet, small jobs share the trace grid.
// The assertions restate what must hold, not how the plan computes it.  Header-only: no library, no GPU.  Prints "ok <plans>" or the
// first counter-example.
#include "../monte-carlo-path-tracer_amd/csrc/wf_plan.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

struct Case {
    uint32_t spp, all, tile_mod, tile_rem, n_lanes, pool_cap, spi, flags, max_depth, priv, small, probe_n, items_per_slot;
};
static void print_case(const Case& c) {
    std::printf("spp=%u all=%u mod=%u rem=%u lanes=%u pool_cap=%u spi=%u flags=%u max_depth=%u priv=%u small=%u probe_n=%u items_per_slot=%u\n", c.spp, c.all,
                c.tile_mod, c.tile_rem, c.n_lanes, c.pool_cap, c.spi, c.flags, c.max_depth, c.priv, c.small, c.probe_n, c.items_per_slot);
}
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED: %s (line %d)\n  ", #cond, __LINE__); print_case(c); return false; } } while (0)

static const uint32_t FIRST = 7, BLOCK_THREADS = 1024;                  // the call's first sample; threads of a trace block
static uint64_t count_tiles(uint64_t all, uint32_t mod, uint32_t rem) { return all / mod + (all % mod > rem ? 1 : 0); }   // |{i < all : i % mod == rem}|, rem < mod
static unsigned long long n_plans = 0;

static bool check(const Case& c) {
    const bool det = (c.flags & MCPT_FLAG_DETERMINISTIC) != 0;
    const uint32_t trace_grid = c.all == 3 ? 1u : 256u;                   // (one shape with fewer blocks than sub-pipelines)
    mcpt_opts o; std::memset(&o, 0, sizeof o);
    o.samples_per_item = c.spi; o.flags = c.flags; o.max_depth = c.max_depth; o.integrator = MCPT_INTEGRATOR_MIS;
    const bool small_shape = c.all <= 187 && c.spp <= 24;                 // the sets are enumerated; larger ones are counted
    uint64_t owned = count_tiles(c.all, c.tile_mod, c.tile_rem);
    if (small_shape) { uint64_t n = 0; for (uint32_t i = 0; i < c.all; i++) n += i % c.tile_mod == c.tile_rem; REQUIRE(n == owned); }

    // ---- the call (7: item-count range)
    RenderParams p0;
    const WfCall verdict = wf_plan_params(p0, c.all, c.tile_mod, c.tile_rem, c.spp, FIRST, 0x123456789abcdefull, o, true);
    REQUIRE((verdict == WfCall::Nothing) == (owned == 0));
    if (verdict == WfCall::Nothing) return true;
    REQUIRE(p0.n_owned == owned && p0.spp == c.spp && p0.first_sample == FIRST && p0.tile_mod == c.tile_mod && p0.tile_rem == c.tile_rem);
    REQUIRE(p0.samples_per_item >= 1 && p0.samples_per_item <= c.spp);
    REQUIRE(uint64_t(p0.chunks) * p0.samples_per_item >= c.spp && uint64_t(p0.chunks - 1) * p0.samples_per_item < c.spp);
    REQUIRE(p0.seed_lo == 0x89abcdefu && p0.seed_hi == 0x01234567u && p0.max_depth == c.max_depth && p0.flags == c.flags && !p0.probe_n && !p0.tile_list);
    if (det) REQUIRE(p0.chunks == 1);
    else if (c.spi) REQUIRE(p0.samples_per_item == std::min(c.spi, c.spp));
    REQUIRE((verdict == WfCall::TooLarge) == (owned * p0.chunks > 0x3ffffffull));
    if (verdict == WfCall::TooLarge && !det && !c.spi) REQUIRE(p0.samples_per_item == c.spp);   // automatic items are refused only when they cannot grow
    {   // the megakernel's rule: refused on the same condition, automatic items of 8 .. 64 samples (or the whole call)
        RenderParams pm;
        const WfCall vm = wf_plan_params(pm, c.all, c.tile_mod, c.tile_rem, c.spp, FIRST, 1, o, false);
        REQUIRE(vm != WfCall::Nothing && pm.n_owned == owned && (vm == WfCall::TooLarge) == (owned * pm.chunks > 0x3ffffffull));
        REQUIRE(uint64_t(pm.chunks) * pm.samples_per_item >= c.spp && uint64_t(pm.chunks - 1) * pm.samples_per_item < c.spp);
        if (!det && !c.spi) REQUIRE(pm.samples_per_item == c.spp || (pm.samples_per_item >= 8 && pm.samples_per_item <= 64));
    }
    if (verdict == WfCall::TooLarge) return true;

    // ---- the plan
    p0.probe_n = c.probe_n;
    const WfKnobs knobs = wf_read_knobs([&](const char* name, uint32_t dflt) -> uint32_t {
        if (!std::strcmp(name, "MCPT_WF_POOL_SLOTS")) return c.pool_cap;
        if (!std::strcmp(name, "MCPT_WF_ITEMS_PER_SLOT")) return c.items_per_slot;
        if (!std::strcmp(name, "MCPT_WF_PRIVATE_ITEMS")) return c.priv;
        if (!std::strcmp(name, "MCPT_WF_SMALL_JOB_SPLIT")) return c.small;
        return dflt; });
    REQUIRE(knobs.pool_cap == c.pool_cap);
    const uint32_t n_lanes = det ? 1u : c.n_lanes;                       // (as the context does: one owner per pixel)
    const WfPlan plan = wf_plan_call(p0, n_lanes, knobs, trace_grid, BLOCK_THREADS);
    n_plans++;
    REQUIRE(plan.lanes.size() == (c.probe_n ? 1u : n_lanes));
    uint32_t n_active = 0; for (const WfLanePlan& l : plan.lanes) n_active += l.active;
    REQUIRE(n_active == plan.n_active && n_active >= 1);
    if (c.probe_n) REQUIRE(!plan.split_tiles);
    REQUIRE(plan.shared_grid >= 1 && uint64_t(plan.shared_grid) * n_active <= std::max(trace_grid, n_active));   // the shares fit the grid

    // 1: exact cover
    std::vector<uint8_t> cover(small_shape && !c.probe_n ? size_t(c.all) * c.spp : 0, 0);
    uint64_t sum_owned = 0, sum_work = 0, next_sample = FIRST;
    std::vector<uint32_t> rems;
    for (const WfLanePlan& l : plan.lanes) {
        if (!l.active) { REQUIRE(!plan.split_tiles && c.spp < n_lanes); continue; }   // only a sample range can be empty
        const RenderParams& p = l.p;
        REQUIRE(p.spp >= 1 && p.first_sample >= FIRST && uint64_t(p.first_sample) + p.spp <= uint64_t(FIRST) + c.spp);
        if (plan.split_tiles) {
            REQUIRE(n_active == n_lanes && p.spp == c.spp && p.first_sample == FIRST);
            REQUIRE(p.tile_mod == c.tile_mod * n_lanes && p.tile_rem < p.tile_mod && p.tile_rem % c.tile_mod == c.tile_rem);   // a part of the call's tiles
            for (uint32_t r : rems) REQUIRE(r != p.tile_rem);                                                                   // and nobody else's
            rems.push_back(p.tile_rem);
            REQUIRE(p.n_owned == count_tiles(c.all, p.tile_mod, p.tile_rem) && p.n_owned >= 1);
        } else {
            REQUIRE(p.tile_mod == c.tile_mod && p.tile_rem == c.tile_rem && p.n_owned == owned);
            REQUIRE(p.first_sample == next_sample);                       // contiguous, in lane order
            next_sample += p.spp;
        }
        sum_owned += p.n_owned; sum_work += uint64_t(p.n_owned) * p.spp;
        for (size_t j = 0; j < (cover.empty() ? 0 : p.n_owned); j++) {    // tile j of a launch = tile_rem + j * tile_mod (RenderParams)
            const uint64_t t = p.tile_rem + uint64_t(j) * p.tile_mod;
            REQUIRE(t < c.all);
            for (uint32_t s = p.first_sample; s < p.first_sample + p.spp; s++) REQUIRE(++cover[t * c.spp + (s - FIRST)] == 1);
        }
    }
    if (plan.split_tiles) REQUIRE(sum_owned == owned); else REQUIRE(next_sample == uint64_t(FIRST) + c.spp);
    REQUIRE(sum_work == owned * c.spp);
    for (size_t i = 0; i < cover.size(); i++) REQUIRE(cover[i] == ((i / c.spp) % c.tile_mod == c.tile_rem ? 1 : 0));

    for (const WfLanePlan& l : plan.lanes) {
        if (!l.active) continue;
        const RenderParams& p = l.p;
        // the items of a lane: 64 pixels of each of its tiles, times the chunks of its sample range
        REQUIRE(p.samples_per_item >= 1 && p.samples_per_item <= p.spp);
        REQUIRE(uint64_t(p.chunks) * p.samples_per_item >= p.spp && uint64_t(p.chunks - 1) * p.samples_per_item < p.spp);
        REQUIRE(uint64_t(l.n_items) == (c.probe_n ? uint64_t(c.probe_n) : uint64_t(p.n_owned) * 64 * p.chunks));
        // 2: pool
        const uint64_t want = (uint64_t(l.n_items) + WF_SHADE_BLOCK - 1) / WF_SHADE_BLOCK * WF_SHADE_BLOCK;
        REQUIRE(l.P % WF_SHADE_BLOCK == 0 && l.P >= WF_SHADE_BLOCK && l.P <= c.pool_cap && l.P <= want);
        if (c.items_per_slot == 1) REQUIRE(l.P == std::min<uint64_t>(want, c.pool_cap));
        // 3: known length
        const bool known = l.n_items <= l.P && p.chunks == 1 && p.samples_per_item == 1 && c.max_depth != 0 && !c.probe_n;
        REQUIRE((l.bound != 0) == known);
        if (known) REQUIRE(l.bound == c.max_depth + 3);
        // 4: hand-out
        REQUIRE(uint64_t(p.shared_base) + l.n_shared == l.n_items && l.n_shared >= 1 && p.priv_items % 64 == 0);
        REQUIRE(p.shared_base == (l.P / WF_SHADE_BLOCK) * p.priv_items);
        if (p.priv_items) REQUIRE(uint64_t(l.n_items) >= 4ull * l.P && c.priv && !c.probe_n);
        if (known) REQUIRE(p.priv_items == 0);
        // 5: atomics
        REQUIRE(p.atomic_accum <= 1);
        if ((n_active > 1 && !plan.split_tiles) || p.chunks > 1) REQUIRE(p.atomic_accum == 1);
        if (det || (plan.split_tiles && p.chunks == 1)) REQUIRE(p.atomic_accum == 0);
        // 6: grid
        REQUIRE(l.grid == trace_grid || l.grid == plan.shared_grid);
        if (l.grid != trace_grid) REQUIRE(n_active > 1 && c.small && !c.probe_n && uint64_t(l.n_items) <= uint64_t(trace_grid) * BLOCK_THREADS * 5 / 2);
        if (plan.small_job) REQUIRE(n_active > 1 && c.small && uint64_t(plan.small_job) <= uint64_t(trace_grid) * BLOCK_THREADS * 5 / 2);
    }
    return true;
}

// 8: the knob reader's clamps, through a fake environment
static bool check_knobs() {
    const Case c{};
    std::map<std::string, uint32_t> env;
    auto read = [&]() { return wf_read_knobs([&](const char* name, uint32_t dflt) { auto it = env.find(name); return it == env.end() ? dflt : it->second; }); };
    WfKnobs k = read();
    REQUIRE(k.pool_cap == 1u << 23 && k.items_per_slot == 1 && k.private_items && k.small_job_split && k.compact && k.compact_eighths == 4);
    REQUIRE(k.max_it == 1u << 20 && !k.debug && k.time_kernels == 0);
    env = {{"MCPT_WF_POOL_LOG2", 40}};  REQUIRE(read().pool_cap == 1u << 26);
    env = {{"MCPT_WF_POOL_LOG2", 11}};  REQUIRE(read().pool_cap == 4096);            // (2048 is below the mask's unit)
    env = {{"MCPT_WF_POOL_LOG2", 13}};  REQUIRE(read().pool_cap == 8192);
    env = {{"MCPT_WF_POOL_SLOTS", 100}};   REQUIRE(read().pool_cap == 4096);
    env = {{"MCPT_WF_POOL_SLOTS", 9000}};  REQUIRE(read().pool_cap == 8192);
    env = {{"MCPT_WF_POOL_SLOTS", 12288}, {"MCPT_WF_POOL_LOG2", 20}};  REQUIRE(read().pool_cap == 12288);
    env = {{"MCPT_WF_ITEMS_PER_SLOT", 0}};  REQUIRE(read().items_per_slot == 1);
    env = {{"MCPT_WF_ITEMS_PER_SLOT", 6}};  REQUIRE(read().items_per_slot == 6);
    env = {{"MCPT_WF_COMPACT_EIGHTHS", 0}};  REQUIRE(read().compact_eighths == 1);
    env = {{"MCPT_WF_COMPACT_EIGHTHS", 9}};  REQUIRE(read().compact_eighths == 7);
    env = {{"MCPT_WF_COMPACT_EIGHTHS", 5}};  REQUIRE(read().compact_eighths == 5);
    env = {{"MCPT_WF_PRIVATE_ITEMS", 0}, {"MCPT_WF_SMALL_JOB_SPLIT", 0}, {"MCPT_WF_COMPACT", 0}, {"MCPT_WF_DEBUG", 2}, {"MCPT_WF_MAXIT", 50}, {"MCPT_TIME_KERNELS", 8}};
    k = read();
    REQUIRE(!k.private_items && !k.small_job_split && !k.compact && k.debug && k.max_it == 50 && k.time_kernels == 8);
    return true;
}

int main() {
    if (!check_knobs()) return 1;
    const uint32_t spps[] = {1, 2, 3, 5, 24, 1024}, alls[] = {1, 2, 3, 45, 187, 10000, 160000}, mods[][2] = {{1, 0}, {3, 0}, {3, 2}, {8, 7}};
    const uint32_t caps[] = {4096, 8192, 1u << 20, 1u << 23};
    for (uint32_t spp : spps) for (uint32_t all : alls) for (auto& m : mods) for (uint32_t n_lanes = 1; n_lanes <= 3; n_lanes++) for (uint32_t cap : caps)
        for (uint32_t spi : {0u, 1u, 4u, spp}) for (uint32_t flags : {0u, uint32_t(MCPT_FLAG_DETERMINISTIC)}) for (uint32_t depth : {0u, 5u})
            for (uint32_t priv : {1u, 0u}) for (uint32_t small : {1u, 0u}) for (uint32_t probe_n : {0u, 1000u})
                for (uint32_t ips : {1u, 4u}) {
                    if (ips != 1 && all != 160000) continue;              // (the rule is about jobs of more than 2^20 items)
                    if (!check(Case{spp, all, m[0], m[1], n_lanes, cap, spi, flags, depth, priv, small, probe_n, ips})) return 1;
                }
    std::printf("ok %llu\n", n_plans);
    return 0;
}
