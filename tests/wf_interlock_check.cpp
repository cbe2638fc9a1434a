// CPU check of the shade interlock's decisions (csrc/wf_plan.h: wf_interlock_call, wf_lane_gated, wf_shade_wait).  The executor's loop of
// render_wavefront is replayed on real plans -- rounds of 2 and 3 sub-pipelines whose jobs finish, and leave the full trace grid, at arbitrary
// rounds; known-length, small-job, slot-per-item and single-lane calls; probes and deterministic mode -- and on every shade launch the test asserts
//   * a wait names a sub-pipeline whose event was recorded earlier in enqueue order (the test keeps its own record of that);
//   * while at least two gated sub-pipelines are live the shade launches are ONE chain: each waits for the shade launch enqueued immediately
//     before it -- unless that one's sub-pipeline has finished or left the full grid since, which is then not waited for;
//   * nothing waits, and nothing is waited for, in the exempt cases.
// Then the enqueued streams are run by a model of the device (a stream executes in order; a wait holds its stream until the record it bound
// to has executed): everything executes, and no two gated shade launches are ever in flight together.
// Header-only: no library, no GPU.  Prints "ok <shade launches>" or the first counter-example.
#include "../monte-carlo-path-tracer_amd/csrc/wf_plan.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

struct Case {
    uint32_t n_lanes, all, spp, max_depth, flags, probe_n, small, interlock, pool_cap;
    uint32_t finish[3], degrade[3];       // the round after whose launch sub-pipeline k's job is seen finished / its trace grid becomes shared_grid (0 = never)
};
static void print_case(const Case& c) {
    std::printf("lanes=%u all=%u spp=%u depth=%u flags=%u probe_n=%u small=%u interlock=%u pool_cap=%u finish=%u,%u,%u degrade=%u,%u,%u\n", c.n_lanes, c.all, c.spp, c.max_depth,
                c.flags, c.probe_n, c.small, c.interlock, c.pool_cap, c.finish[0], c.finish[1], c.finish[2], c.degrade[0], c.degrade[1], c.degrade[2]);
}
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED: %s (line %d)\n  ", #cond, __LINE__); print_case(c); return false; } } while (0)

static const uint32_t TRACE_GRID = 256, BLOCK_THREADS = 1024, MAX_ROUNDS = 40;
static unsigned long long n_launches = 0, n_waits = 0, n_cases_chained = 0;

enum OpKind { WAIT, SHADE, RECORD, TRACE };
struct Op { OpKind kind; int lane; uint32_t version; bool gated; };   // WAIT: for record `version` of `lane`; RECORD: its own version; SHADE: gated or not

static bool check(const Case& c) {
    mcpt_opts o; std::memset(&o, 0, sizeof o);
    o.flags = c.flags; o.max_depth = c.max_depth; o.integrator = MCPT_INTEGRATOR_MIS;
    RenderParams p0;
    REQUIRE(wf_plan_params(p0, c.all, 1, 0, c.spp, 0, 1, o, true) == WfCall::Go);
    p0.probe_n = c.probe_n;
    const WfKnobs knobs = wf_read_knobs([&](const char* name, uint32_t dflt) -> uint32_t {
        if (!std::strcmp(name, "MCPT_WF_SMALL_JOB_SPLIT")) return c.small;
        if (!std::strcmp(name, "MCPT_WF_INTERLOCK")) return c.interlock;
        if (!std::strcmp(name, "MCPT_WF_POOL_SLOTS")) return c.pool_cap;
        return dflt; });
    const bool det = (c.flags & MCPT_FLAG_DETERMINISTIC) != 0;
    const WfPlan plan = wf_plan_call(p0, det ? 1u : c.n_lanes, knobs, TRACE_GRID, BLOCK_THREADS);
    const uint32_t n = uint32_t(plan.lanes.size());
    const bool call_exempt = !c.interlock || plan.n_active < 2 || c.probe_n || det;
    REQUIRE(wf_interlock_call(plan, p0, knobs) == !call_exempt);

    // the executor's state, and the test's own: which sub-pipelines have recorded (and how often), every launch in enqueue order
    std::vector<WfLaneState> st(n);
    std::vector<uint32_t> it(n, 0), recorded(n, 0);
    std::vector<std::vector<Op>> stream(n);
    for (uint32_t k = 0; k < n; k++) st[k] = WfLaneState{!plan.lanes[k].active, plan.lanes[k].grid};
    auto state_of = [&](uint32_t j) { return st[j]; };
    auto expect_gated = [&](uint32_t j) {                                 // restated from the rules, not from wf_lane_gated
        if (call_exempt || !plan.lanes[j].active || st[j].done) return false;
        return plan.lanes[j].bound == 0 && plan.lanes[j].n_items > plan.lanes[j].P && st[j].grid != plan.shared_grid;   // polled, more items than slots, full grid
    };
    int last = WF_NO_LANE, prev_shade = -1;                               // prev_shade: the sub-pipeline of the gated shade launch enqueued immediately before
    int prev_any = -1; bool prev_any_gated = false;                       // the shade launch enqueued immediately before, whoever's, and whether it was gated
    bool steady_case = true;                                              // nobody finishes or leaves the full grid during the call
    for (uint32_t k = 0; k < 3; k++) if (c.finish[k] || c.degrade[k]) steady_case = false;
    bool waited_any = false;
    for (uint32_t round = 1; round <= MAX_ROUNDS; round++) {
        bool all_done = true;
        for (uint32_t k = 0; k < n; k++) {
            if (st[k].done) continue;
            const WfLanePlan& lp = plan.lanes[k];
            uint32_t gated = 0; for (uint32_t j = 0; j < n; j++) gated += expect_gated(j);
            const bool me = expect_gated(k);
            REQUIRE(wf_lane_gated(plan, p0, knobs, k, st[k]) == me);
            const int w = wf_shade_wait(plan, p0, knobs, k, state_of, last);
            n_launches++;
            if (w != WF_NO_LANE) {
                REQUIRE(w >= 0 && uint32_t(w) < n && uint32_t(w) != k);
                REQUIRE(recorded[w] > 0);                                 // an event recorded earlier in enqueue order
                REQUIRE(me && gated >= 2 && expect_gated(uint32_t(w)));   // only gated lanes wait, and only for gated ones
                REQUIRE(lp.bound == 0 && plan.lanes[w].bound == 0 && lp.n_items > lp.P && plan.lanes[w].n_items > plan.lanes[w].P && st[k].grid != plan.shared_grid && st[w].grid != plan.shared_grid);
                REQUIRE(w == prev_shade);                                 // the shade launch enqueued immediately before this one
                stream[k].push_back(Op{WAIT, w, recorded[w], false});
                waited_any = true; n_waits++;
            } else if (me && gated >= 2 && prev_shade >= 0) {
                REQUIRE(uint32_t(prev_shade) == k || !expect_gated(uint32_t(prev_shade)));   // the chain breaks only behind a lane that has just left it
            }
            if (call_exempt || !me || gated < 2) REQUIRE(w == WF_NO_LANE);
            if (me && gated >= 2 && prev_any >= 0 && uint32_t(prev_any) != k && prev_any_gated && expect_gated(uint32_t(prev_any))) REQUIRE(w == prev_any);
            prev_any = int(k); prev_any_gated = me;
            stream[k].push_back(Op{SHADE, int(k), 0, me});
            if (wf_lane_gated(plan, p0, knobs, k, st[k])) {               // what render_wavefront does after the shade launch
                stream[k].push_back(Op{RECORD, int(k), ++recorded[k], false});
                last = int(k); prev_shade = int(k);
            }
            stream[k].push_back(Op{TRACE, int(k), 0, false});
            it[k]++;
            if (lp.bound && it[k] == lp.bound) { st[k].done = true; continue; }
            if (!lp.bound && c.degrade[k] && round >= c.degrade[k] && plan.small_job) st[k].grid = plan.shared_grid;   // (wf_poll: a compacted sweep)
            if (!lp.bound && c.finish[k] && round >= c.finish[k]) st[k].done = true;
            if (!st[k].done) all_done = false;
        }
        if (all_done) break;
    }
    if (call_exempt) REQUIRE(!waited_any && last == WF_NO_LANE);
    for (uint32_t k = 0; k < n; k++) if (plan.lanes[k].bound || (plan.lanes[k].active && (plan.lanes[k].grid == plan.shared_grid || plan.lanes[k].n_items <= plan.lanes[k].P))) REQUIRE(recorded[k] == 0);
    // two or more sub-pipelines that stay on the full grid for the whole call: every shade launch but the first waits
    {
        uint32_t steady = 0; for (uint32_t k = 0; k < n; k++) steady += !call_exempt && plan.lanes[k].active && !plan.lanes[k].bound && plan.lanes[k].n_items > plan.lanes[k].P && plan.lanes[k].grid != plan.shared_grid;
        if (steady >= 2 && steady_case) { REQUIRE(waited_any); n_cases_chained++; }
    }

    // ---- the device's side: run the streams
    std::vector<size_t> pc(n, 0);
    std::vector<uint32_t> executed(n, 0);                                 // records executed per sub-pipeline
    std::vector<uint8_t> in_flight(n, 0);                                 // a gated shade launch is in flight until the record behind it executes
    for (bool progress = true; progress;) {
        progress = false;
        for (uint32_t k = 0; k < n; k++) {
            if (pc[k] == stream[k].size()) continue;
            const Op& op = stream[k][pc[k]];
            if (op.kind == WAIT && executed[op.lane] < op.version) continue;
            if (op.kind == SHADE && op.gated) {
                // while the set of gated sub-pipelines does not change, no two gated shade launches are in flight together
                if (steady_case) for (uint32_t j = 0; j < n; j++) REQUIRE(j == k || !in_flight[j]);
                in_flight[k] = 1;
            }
            if (op.kind == RECORD) { executed[k] = op.version; in_flight[k] = 0; }
            pc[k]++; progress = true;
            break;                                                        // one operation at a time, lowest stream first: an adversarial-enough order
        }
    }
    for (uint32_t k = 0; k < n; k++) REQUIRE(pc[k] == stream[k].size()); // everything executed: no wait was left hanging
    return true;
}

static bool check_knob() {
    const Case c{};
    std::map<std::string, uint32_t> env;
    auto read = [&]() { return wf_read_knobs([&](const char* name, uint32_t dflt) { auto f = env.find(name); return f == env.end() ? dflt : f->second; }); };
    REQUIRE(read().interlock == (WF_INTERLOCK_DEFAULT != 0));
    env = {{"MCPT_WF_INTERLOCK", 0}};  REQUIRE(!read().interlock);
    env = {{"MCPT_WF_INTERLOCK", 1}};  REQUIRE(read().interlock);
    return true;
}

int main() {
    if (!check_knob()) return 1;
    // all = tiles of the film: 256 = the 128 x 128 film of the GPU tests, 10000 = 800 x 800.  spp: 1 (tile split, known length), 2 / 3 (a known-length
    // lane beside a polled one), 32 (small jobs on 256 tiles, full grid on 10000), 33 (uneven shares); pools of 65536 slots (fewer than items) and 2^23
    const uint32_t never[3] = {0, 0, 0};
    const uint32_t rounds[] = {0, 1, 2, 3, 5, 8, 13};
    for (uint32_t n_lanes = 1; n_lanes <= 3; n_lanes++) for (uint32_t all : {2u, 256u, 10000u}) for (uint32_t spp : {1u, 2u, 3u, 5u, 32u, 33u})
        for (uint32_t depth : {0u, 8u}) for (uint32_t flags : {0u, uint32_t(MCPT_FLAG_DETERMINISTIC)}) for (uint32_t probe_n : {0u, 1000u})
            for (uint32_t small : {1u, 0u}) for (uint32_t interlock : {1u, 0u}) for (uint32_t cap : {65536u, 1u << 23}) {
                Case c{n_lanes, all, spp, depth, flags, probe_n, small, interlock, cap, {0, 0, 0}, {0, 0, 0}};
                std::memcpy(c.finish, never, sizeof never); std::memcpy(c.degrade, never, sizeof never);
                if (!check(c)) return 1;                                  // nobody finishes: the loop runs its MAX_ROUNDS
                if (flags || probe_n || !interlock) continue;
                for (uint32_t f0 : rounds) for (uint32_t f1 : rounds) for (uint32_t f2 : rounds) for (uint32_t d0 : {0u, 2u, 6u}) for (uint32_t d1 : {0u, 1u, 4u}) {
                    if (n_lanes < 3 && f2) continue;
                    Case v = c; v.finish[0] = f0; v.finish[1] = f1; v.finish[2] = f2; v.degrade[0] = d0; v.degrade[1] = d1; v.degrade[2] = (d0 + d1) % 5;
                    if (!check(v)) return 1;
                }
            }
    if (n_cases_chained < 20 || n_waits < 10000) { std::printf("FAILED: the sweep hardly reached the interlock (%llu chained cases, %llu waits)\n", n_cases_chained, n_waits); return 1; }
    std::printf("ok %llu\n", n_launches);
    return 0;
}
