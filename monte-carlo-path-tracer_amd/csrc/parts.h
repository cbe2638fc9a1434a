// Launcher and host helpers of the parts update (parts.hip), called from mcpt_api.cpp: mcpt_update_parts runs several deformers in one call, each
// into a scratch pair, and copies from there the records that the deformer OWNS into the context's current vertices and normals, in front of ONE
// normals pass and ONE refit.  DESIGN.md §23 has the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>

#define PT_BLOCK 256                   // threads per block of the select kernel (4 wave64)
#define PT_MAX_BLOCKS 2048             // its grid-stride loop: at most 8 blocks per CU of an MI355X, as keyframes.hip's KF_MAX_BLOCKS
#define PT_OWNERS 5                    // owner ids: 0 none, 1 groups, 2 skin, 3 morph, 4 keyframes (mcpt.h's MCPT_OWNER_*)
#define PT_ROUTES 0x1eu                // every route bit, 1u << owner id for the ids 1 .. 4 (mcpt.h's MCPT_ROUTE_*)
#define PT_MORPH_THEN_SKIN 0x1u        // the one flag (mcpt.h's MCPT_PARTS_MORPH_THEN_SKIN)

// The host functions here touch no device; tests/parts_host_check.cpp runs them stand-alone.
// mcpt_set_vertex_owners' rules for its arrays, in the documented order: counts that differ from the scene's, a null normal_owner with n_normal > 0,
// an id >= PT_OWNERS (vertices first, each array in record order).  true: vertex_count / normal_count hold the records per owner id.  false: `err`
// names the fault (and the record), the counts are not meaningful.  vertex_owner is not null (null drops the owners before this is asked).
struct PtCounts { uint32_t vertex[PT_OWNERS], normal[PT_OWNERS]; };
bool pt_check_owners(const uint8_t* vertex_owner, uint32_t n_vertex, const uint8_t* normal_owner, uint32_t n_normal, uint32_t scene_vertex,
                     uint32_t scene_normal, PtCounts& counts, std::string& err);

// What one mcpt_update_parts call runs: the owner ids of its routes in ascending order; is the morph followed by the skin; do the bones travel
// (the skin route, or the skin behind the morph: staged once for both).
struct PtPlan { uint32_t n_steps, step[PT_OWNERS - 1]; bool morph_then_skin, bones; };
// The plan of `routes` / `flags`, or why there is none: no route, an unknown route bit, an unknown flag bit, PT_MORPH_THEN_SKIN without the morph
// route -- judged in this order.
enum PtPlanStatus { PT_PLAN_OK = 0, PT_PLAN_NO_ROUTE, PT_PLAN_UNKNOWN_ROUTE, PT_PLAN_UNKNOWN_FLAG, PT_PLAN_SKIN_WITHOUT_MORPH };
PtPlanStatus pt_plan(uint32_t routes, uint32_t flags, PtPlan& plan);

// dst[i] = src[i] (the record's three doubles, moved as 64-bit integers: every bit pattern survives) for every record i < n with owner[i] == id;
// nothing else of dst is touched.  One lane per double, grid-stride.  n == 0 launches nothing.  `src` and `dst` must not overlap.
hipError_t launch_pt_select(const double* src, double* dst, const uint8_t* owner, uint32_t id, uint32_t n, hipStream_t stream);
