// Host-side scene preparation: the MI355X replacement for Render::tranform_triangle (Render.cpp:12-44) and
// BVH::BVH / BVH::build (BVH.cpp:6-54).  Output = the flat arrays of device_scene.h, ready for one hipMemcpy each.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>
#include "../../include/mcpt.h"
#include "device_scene.h"

struct f4h { float x, y, z, w; };   // host mirror of float4 (16 B)

// What a material record needs of its texture: where its texels start in DevScene::texels, its size, and its first texel (the constant colour of a
// 1x1 texture).  mcpt_create keeps the table, mcpt_update_texture edits it.
struct TexInfo { int32_t off, w, h; float rgb[3]; };

struct HostScene {
    std::vector<f4h> nodes;          // 4 per inner node (binary tree: megakernel + probes)
    std::vector<f4h> nodes8;         // 5 per node of the 8-wide compressed tree (wavefront trace kernel)
    std::vector<f4h> tri_isect;      // 3 per triangle (leaf order)
    std::vector<f4h> tri_shade;      // MCPT_TRI_SHADE_F4 = 8 per triangle: shading record (4) + fp64 plane (2) + spare (2), device_scene.h
    std::vector<double> tri_pos64;   // 9 per triangle
    std::vector<int32_t> tri_face;   // leaf order -> input face index
    std::vector<DevMaterial> mats;
    std::vector<DevLight> lights;
    std::vector<double> light_pos64; // 9 per light
    std::vector<f4h> texels;
    std::vector<TexInfo> tex_info;   // per texture of the description
    std::vector<uint32_t> mat_faces; // per material: the faces that use it
    DevCamera cam;
    double centre[3] = {0.0, 0.0, 0.0};   // the point every coordinate above is relative to (device_scene.h: DevScene::centre)
    uint32_t bvh_depth = 0, max_leaf = 0, bvh8_depth = 0;
    uint32_t bvh_builder = 0;        // out: mcpt_scene_info::bvh_builder (0 host SAH, 1 custom builder's tree kept, 2 custom builder's result discarded)
    std::vector<int> subtree_begin;  // binary nodes: first index of every depth-first-numbered subtree below the breadth-first top levels (ascending)
    bool reference_tie_order = false; // in: MCPT_FLAG_REFERENCE_TIE_ORDER -- the tie rank of a triangle (low 28 bits of tri_isect[3 i].w) is its position in the
                                     //     reference's BVH::triangles after BVH::build instead of its position in this library's leaf order
    bool allow_deep_binary = false;  // in: the caller never traverses `nodes` (wavefront pipeline only) -> a device tree deeper than MCPT_STACK_DEPTH is fine
    bool binary_ok = true;           // out: `nodes` fits the binary-tree kernels' stack
    double bvh_build_ms = 0.0;
    bool keep_dynamic = false;       // in: MCPT_FLAG_DYNAMIC -- also fill dyn_idx
    std::vector<int32_t> dyn_idx;    // 6 per triangle (leaf order): its three vertex indices, then its three normal indices
};

// Optional replacement for the host SAH builder (bvh_gpu.hip): gets one fp32 box per face (lo xyz, hi xyz, rounded outward) and
// fills the binary tree in the host builder's node layout, the leaf order, the depth in inner levels and the largest leaf.  false = an error
// (build_host_scene fails with it); true with `nodes` left empty = the builder gave up on this input and the host builder takes over.
using BvhBuildFn = std::function<bool(const float* boxes, uint32_t n, std::vector<f4h>& nodes, std::vector<int>& order, uint32_t& depth,
                                      uint32_t& max_leaf, std::string& err)>;

// Optional replacement for the host's 8-wide collapse + quantisation (bvh_gpu.hip: gpu_collapse_bvh8): binary nodes (renumbered, root = 0) in, nodes8 + depth
// out; rewrites the binary tree's leaf codes and the leaf order like build_bvh8 does.
using Collapse8Fn = std::function<bool(std::vector<f4h>& nodes2, std::vector<int>& order, std::vector<f4h>& nodes8, uint32_t& depth8, std::string& err)>;

// What the builders see of a face, in centred coordinates: its fp64 bound and centroid (host builder) ...
struct BTri { double lo[3], hi[3], c[3]; };
// ... given in Model::face order by two providers that are asked only when their builder runs (mcpt_rebuild_trees fetches them from the device):
// bounds64 for the host builder, boxes32 -- lo xyz, hi xyz, the fp64 bound rounded outward -- for the custom one.  nullptr = failed, `err` filled.
struct TreeInput {
    uint32_t n_face;
    std::function<const BTri*()> bounds64;
    std::function<const float*()> boxes32;
};
// Both trees of a scene: the custom builder (when given and the scene has more than one leaf) with its fallbacks or the host builder, the
// renumbering, the 8-wide collapse.  Reads out.allow_deep_binary; fills out.nodes, nodes8, bvh_depth, max_leaf, bvh8_depth, subtree_begin,
// bvh_builder, binary_ok, bvh_build_ms and `order` (leaf position -> face).  build_host_scene and mcpt_rebuild_trees both build through it.
mcpt_status build_trees(const TreeInput& in, HostScene& out, std::vector<int>& order, std::string& err, const BvhBuildFn& custom_bvh = nullptr,
                        const Collapse8Fn& custom_collapse8 = nullptr);

// Validates the description (indices in range, sizes non-zero), flattens faces, collects lights, builds the BVH.
// Returns MCPT_OK or an error code with `err` filled.
mcpt_status build_host_scene(const mcpt_scene_desc* d, HostScene& out, std::string& err, const BvhBuildFn& custom_bvh = nullptr,
                             const Collapse8Fn& custom_collapse8 = nullptr);

// Host-side soundness check of the quantised 8-wide tree (empty string = sound); run by mcpt_check_scene.
std::string validate_bvh8(const HostScene& hs);
// The same containment walk over the binary tree `nodes`.
std::string validate_bvh2(const HostScene& hs);
inline std::string validate_wide_bvh(const HostScene& hs) { return validate_bvh8(hs); }
// Level structure of both trees, one refit launch per level: the binary nodes sorted by height (bin_order, bin_level), the 8-wide records by depth (wide_level).
bool rf_levels(const std::vector<f4h>& n2, const std::vector<f4h>& n8, std::vector<uint32_t>& bin_order, std::vector<uint32_t>& bin_level,
               std::vector<uint32_t>& wide_level, std::string& err);

// The DevMaterial of `m` over its texture `t` (t = tex_info[m.map_kd], range-checked by the caller): used by mcpt_create, mcpt_update_materials and
// mcpt_update_texture.
DevMaterial device_material(const mcpt_material& m, const TexInfo& t);
// DevCamera of `camera` for a scene centred at `centre` (fp64, the reference's operation order): used by mcpt_create and mcpt_set_camera.
void camera_constants(const mcpt_camera& camera, const double* centre, DevCamera& out);
// Why camera_constants cannot make rays of `camera` (cross(front, up) zero or not finite: `up` parallel to the view, eye == lookat, a field that is
// not finite), or the empty string: asked by mcpt_create, mcpt_check_scene and every call that takes a camera for a live context.
std::string camera_defect(const mcpt_camera& camera);
// The coordinate bound build_host_scene enforces on every vertex a face uses.
constexpr double MCPT_MAX_COORD = 1e18;
