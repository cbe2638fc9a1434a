// gfx950 kernel and host half of the parts update: mcpt_update_parts drives each part of a live scene by its own deformer in ONE
// call.  Every vertex record and every normal record names the one route that writes it (mcpt_set_vertex_owners: one byte per record).  The
// deformer kernels of transform.hip, skin.hip, morph.hip and keyframes.hip are used as they are -- their bit-for-bit suites stay the yardstick --
// and write a scratch pair; the one kernel here then copies the records that the route owns into the context's CURRENT arrays (rf_vtx / rf_nrm),
// route after route on the same stream, in front of one normals pass and one refit.
//
// The select is a memory-bound stream without arithmetic: one owner byte, 8 B read and 8 B written per double that is taken.  One lane per
// DOUBLE, the record being j / 3: lane i of a wave touches base + 8 i, so every load and store of a wave is one contiguous, aligned 512-byte
// run.  One lane per 24-byte record would put the lanes of each of its three accesses 24 B apart.  Contraction is off in this file like in its
// siblings (there is nothing to contract: one rule for all of them).  Plain C++ loads and vector stores only.
#include "parts.h"

#pragma clang fp contract(off)

bool pt_check_owners(const uint8_t* vertex_owner, uint32_t n_vertex, const uint8_t* normal_owner, uint32_t n_normal, uint32_t scene_vertex,
                     uint32_t scene_normal, PtCounts& counts, std::string& err) {
    if (n_vertex != scene_vertex || n_normal != scene_normal) { err = "n_vertex / n_normal differ from the scene's"; return false; }
    if (n_normal && !normal_owner) { err = "null normal_owner"; return false; }
    counts = PtCounts{};
    for (uint32_t i = 0; i < n_vertex; i++) {
        if (vertex_owner[i] >= PT_OWNERS) { err = "vertex " + std::to_string(i) + ": owner id " + std::to_string(unsigned(vertex_owner[i])) + " > 4"; return false; }
        counts.vertex[vertex_owner[i]]++;
    }
    for (uint32_t i = 0; i < n_normal; i++) {
        if (normal_owner[i] >= PT_OWNERS) { err = "normal " + std::to_string(i) + ": owner id " + std::to_string(unsigned(normal_owner[i])) + " > 4"; return false; }
        counts.normal[normal_owner[i]]++;
    }
    return true;
}

PtPlanStatus pt_plan(uint32_t routes, uint32_t flags, PtPlan& plan) {
    plan = PtPlan{};
    if (routes == 0) return PT_PLAN_NO_ROUTE;
    if (routes & ~PT_ROUTES) return PT_PLAN_UNKNOWN_ROUTE;
    if (flags & ~PT_MORPH_THEN_SKIN) return PT_PLAN_UNKNOWN_FLAG;
    const bool morph = (routes >> 3) & 1u, skin = (routes >> 2) & 1u;
    if ((flags & PT_MORPH_THEN_SKIN) && !morph) return PT_PLAN_SKIN_WITHOUT_MORPH;
    for (uint32_t id = 1; id < PT_OWNERS; id++) if ((routes >> id) & 1u) plan.step[plan.n_steps++] = id;
    plan.morph_then_skin = (flags & PT_MORPH_THEN_SKIN) != 0;
    plan.bones = skin || plan.morph_then_skin;
    return PT_PLAN_OK;
}

namespace {

__global__ void __launch_bounds__(PT_BLOCK) pt_select_kernel(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, const uint8_t* __restrict__ owner,
                                                             uint32_t id, uint32_t n) {
    const size_t total = 3 * size_t(n), step = size_t(gridDim.x) * PT_BLOCK;
    for (size_t j = size_t(blockIdx.x) * PT_BLOCK + threadIdx.x; j < total; j += step)
        if (owner[j / 3] == id) dst[j] = src[j];
}

}  // namespace

hipError_t launch_pt_select(const double* src, double* dst, const uint8_t* owner, uint32_t id, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t total = 3 * size_t(n), blocks = (total + PT_BLOCK - 1) / PT_BLOCK;
    const dim3 grid(uint32_t(blocks > PT_MAX_BLOCKS ? PT_MAX_BLOCKS : blocks));
    hipLaunchKernelGGL(pt_select_kernel, grid, dim3(PT_BLOCK), 0, stream, reinterpret_cast<const uint64_t*>(src), reinterpret_cast<uint64_t*>(dst), owner, id, n);
    return hipGetLastError();
}
