// The permutation of a tree rebuild, planned on the host: pure, no HIP call, checkable with the host compiler
// (tests/rebuild_plan_check.cpp), after the precedent of wf_plan.h.
//
// mcpt_rebuild_trees keeps every triangle record and changes only where it lies: the streams are in LEAF ORDER, and a new tree has a new one.
//   old_order[p] = the face at old leaf position p   (tri_face as downloaded from the device)
//   new_order[i] = the face at new leaf position i   (`order` of build_trees)
// Both must be permutations of 0 .. n-1.  The plan:
//   src_of_dst[i] = the old position of the triangle that goes to new position i   (what rb_permute_kernel gathers by)
//   dst_of_src[p] = the new position of the triangle at old position p             (what rb_lights_kernel renumbers DevLight::tri by)
// so old_order[src_of_dst[i]] == new_order[i] and dst_of_src[src_of_dst[i]] == i.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

struct RebuildPlan {
    std::vector<uint32_t> src_of_dst, dst_of_src;
};

// Empty string = planned; otherwise why an input is not a permutation (a duplicate, a gap, an index out of range, a length that differs), and
// `plan` is left empty: the rebuild is refused and nothing changes.
template <class OldIndex, class NewIndex>
std::string rb_plan(const OldIndex* old_order, size_t n_old, const NewIndex* new_order, size_t n_new, RebuildPlan& plan) {
    plan.src_of_dst.clear(); plan.dst_of_src.clear();
    if (n_old != n_new) return "the new leaf order has " + std::to_string(n_new) + " entries, the old one " + std::to_string(n_old);
    const size_t n = n_old;
    if (n >= (size_t(1) << 32)) return "too many triangles";
    constexpr uint32_t NONE = 0xffffffffu;
    std::vector<uint32_t> old_pos(n, NONE);                              // face -> old position
    for (size_t p = 0; p < n; p++) {
        const long long f = (long long)old_order[p];
        if (f < 0 || size_t(f) >= n) return "old leaf order: position " + std::to_string(p) + " names face " + std::to_string(f) + ", out of range";
        if (old_pos[size_t(f)] != NONE) return "old leaf order: face " + std::to_string(f) + " appears twice (positions " + std::to_string(old_pos[size_t(f)]) + " and " + std::to_string(p) + ")";
        old_pos[size_t(f)] = uint32_t(p);
    }
    // n entries in range without a duplicate: no gap either
    std::vector<uint32_t> src(n), dst(n, NONE);
    for (size_t i = 0; i < n; i++) {
        const long long f = (long long)new_order[i];
        if (f < 0 || size_t(f) >= n) return "new leaf order: position " + std::to_string(i) + " names face " + std::to_string(f) + ", out of range";
        const uint32_t p = old_pos[size_t(f)];
        if (dst[p] != NONE) return "new leaf order: face " + std::to_string(f) + " appears twice (positions " + std::to_string(dst[p]) + " and " + std::to_string(i) + "): another face is missing";
        src[i] = p; dst[p] = uint32_t(i);
    }
    plan.src_of_dst.swap(src); plan.dst_of_src.swap(dst);
    return std::string();
}
