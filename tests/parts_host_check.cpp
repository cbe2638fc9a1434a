// The host half of the parts update -- pt_check_owners and pt_plan of csrc/parts.hip, what mcpt_set_vertex_owners judges its arrays with and
// mcpt_update_parts turns its `routes` / `flags` into -- as a stand-alone program (no device is touched), for
// tests/test_parts.py::test_host_owner_checks_counts_and_plans_are_the_restatement.  Built from this file and parts.hip; it may be built with the
// host sanitizers (-Xarch_host -fsanitize=address,undefined).
//   parts_host_check in.bin out.bin
// in.bin: n_owner_cases, n_plan_cases (2 u32); per owner case n_vertex, n_normal, scene_vertex, scene_normal, len_v, len_n (6 u32; len_n ==
// 0xffffffff: a NULL normal_owner) and then len_v and len_n owner bytes; per plan case routes, flags (2 u32).
// out.bin: per owner case ok, vertex counts[5], normal counts[5] (11 u32) and the message (96 bytes, zero-padded); per plan case status, n_steps,
// step[4], morph_then_skin, bones (8 u32).
#include <cstdio>
#include <cstring>
#include <vector>
#include "parts.h"

struct OwnerCase { uint32_t n_vertex, n_normal, scene_vertex, scene_normal, len_v, len_n; };
struct OwnerAnswer { uint32_t ok, vertex[PT_OWNERS], normal[PT_OWNERS]; char message[96]; };
struct PlanAnswer { uint32_t status, n_steps, step[4], morph_then_skin, bones; };
static_assert(sizeof(OwnerCase) == 24 && sizeof(OwnerAnswer) == 140 && sizeof(PlanAnswer) == 32, "the layouts the test writes and reads");

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb"); if (!f) return 3;
    FILE* o = std::fopen(argv[2], "wb"); if (!o) { std::fclose(f); return 3; }
    uint32_t head[2] = {0, 0};
    int rc = std::fread(head, sizeof head, 1, f) == 1 ? 0 : 3;
    for (uint32_t c = 0; c < head[0] && !rc; c++) {
        OwnerCase q;
        if (std::fread(&q, sizeof q, 1, f) != 1) { rc = 3; break; }
        const bool null_normal = q.len_n == 0xffffffffu;
        std::vector<uint8_t> vo(q.len_v), no(null_normal ? 0 : q.len_n);
        if (!vo.empty() && std::fread(vo.data(), 1, vo.size(), f) != vo.size()) { rc = 3; break; }
        if (!no.empty() && std::fread(no.data(), 1, no.size(), f) != no.size()) { rc = 3; break; }
        // the function reads n_vertex / n_normal owners once the counts are the scene's: the case must hold that many
        if (q.n_vertex == q.scene_vertex && q.n_normal == q.scene_normal && (vo.size() < q.n_vertex || (!null_normal && no.size() < q.n_normal))) { rc = 5; break; }
        PtCounts counts{}; std::string err;
        static const uint8_t nothing = 0;                                   // (a vector's data() may be null when it is empty; vertex_owner must not be)
        const bool ok = pt_check_owners(vo.empty() ? &nothing : vo.data(), q.n_vertex, null_normal ? nullptr : (no.empty() ? &nothing : no.data()), q.n_normal,
                                        q.scene_vertex, q.scene_normal, counts, err);
        OwnerAnswer a; std::memset(&a, 0, sizeof a);
        a.ok = ok;
        if (ok) { std::memcpy(a.vertex, counts.vertex, sizeof a.vertex); std::memcpy(a.normal, counts.normal, sizeof a.normal); }
        if (ok != err.empty() || err.size() >= sizeof a.message) rc = 4;   // a message exactly when refused
        std::memcpy(a.message, err.data(), err.size() < sizeof a.message ? err.size() : sizeof a.message - 1);
        if (std::fwrite(&a, sizeof a, 1, o) != 1) rc = 3;
    }
    for (uint32_t c = 0; c < head[1] && !rc; c++) {
        uint32_t q[2];
        if (std::fread(q, sizeof q, 1, f) != 1) { rc = 3; break; }
        PtPlan plan;
        PlanAnswer a; std::memset(&a, 0, sizeof a);
        a.status = uint32_t(pt_plan(q[0], q[1], plan));
        a.n_steps = plan.n_steps; a.morph_then_skin = plan.morph_then_skin; a.bones = plan.bones;
        if (plan.n_steps > 4) rc = 4;
        for (uint32_t k = 0; k < plan.n_steps && k < 4; k++) a.step[k] = plan.step[k];
        if (std::fwrite(&a, sizeof a, 1, o) != 1) rc = 3;
    }
    std::fclose(f); std::fclose(o);
    return rc;
}
