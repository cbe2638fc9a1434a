// `Render` with the reference's surface (src/Render.h:51-69) on top of the C ABI (include/mcpt.h).  No HIP here.
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/mcpt.h"
#include "Model.h"
#include "Scene.h"

// One morph target: the records it displaces, strictly ascending, and 3 doubles of displacement per record.
struct MorphTarget { std::vector<uint32_t> index; std::vector<double> delta; };
// One parts update: the routes that run (MCPT_ROUTE_*), the flags (MCPT_PARTS_MORPH_THEN_SKIN) and the payloads of those routes --
// update_transforms' matrices, update_skin's (also the skin behind the morph), update_morph's weights, update_keyframes' time.
struct PartsUpdate { uint32_t routes = 0, flags = 0; std::vector<double> group_matrices, bone_matrices, morph_weights; double time = 0.0; };

class Render : public FilmSource {
public:
    explicit Render(Model& m_model);                  // Render.cpp:5-10: flatten + BVH + upload (inside mcpt_create)
    Render(Model& m_model, const mcpt_opts& opts);
    Render(Render& same_scene, int device);           // the same scene on another GPU: copied device to device, nothing is built again
    ~Render();
    void render(Scene& scene);                        // Render.cpp:56-69: adds exactly ONE sample to every pixel of `scene`
    void render(Scene& scene, uint32_t spp);          // the same `spp` times in one call
    // The samples stay in HBM (the Scene is told: Scene::attach) until the Scene is read -- getPixelsColor, save_image, pixels(),
    // Scene::sync -- or rendered into by another Render, or either object goes away.
    void flush_into(Scene& scene) override;
    void scene_gone(Scene& scene) override;
    void displaced(Scene& scene) override;
    const Color3b* tonemapped(Scene& scene) override;
    // Denoised preview of what `scene` holds: the a-trous filter of the film getPixelsColor shows, tonemapped the same
    // way -- width * height pixels in getPixelsColor's orientation, valid until the next call.  The first call renders the feature buffers
    // (4 samples of `seed`).  nullptr on failure.
    const Color3b* denoised(Scene& scene, const mcpt_denoise_opts* opts = nullptr);
    // Adaptive sampling into `scene` (mcpt_render_adaptive): the samples stay on the device like render()'s, and the next frame
    // starts past the largest per-tile count this call reached, so no sample index is used twice.  passes == 0 on failure.
    mcpt_adaptive_stats render_adaptive(Scene& scene, const mcpt_adaptive_opts* opts = nullptr);
    // Live scenes.  set_camera: a new camera of the same film size (mcpt_set_camera).  update: positions, normals and camera
    // re-read from `m_model`, the Model this Render was made from, after the caller edited Model::vertex / normal / camerainfo in place -- same
    // faces and materials; the Render must have been created with MCPT_FLAG_DYNAMIC in its mcpt_opts (mcpt_update_vertices).  Both start the
    // picture again: the device film and `scene` are cleared, the sample numbering restarts at 0, the feature buffers are forgotten -- the
    // reference's loop goes on with render(scene) as before.  false (and an unchanged Render and Scene) on failure.
    bool set_camera(Scene& scene, const CameraInfo& camera);
    // set_camera that carries the picture over instead of starting it again (mcpt_set_camera_reproject): everything `scene` holds
    // is brought to the device (a host part is uploaded), looked up at the new view's surface points and left on the device as `scene`'s film,
    // at most max_history samples per pixel (0 = the library's default); pixels without history start empty.  The sample numbering goes ON, so
    // the next render(scene) adds samples the history has not seen.  Exact for diffuse surfaces only: glossy and mirror radiance lags behind the
    // view until max_history new samples have diluted it.  For update() there is update_reproject below.  false on failure (the Render
    // and the Scene's samples are unchanged, the samples are then all on the host).
    bool set_camera_reproject(Scene& scene, const CameraInfo& camera, float max_history = 0);
    bool update(Scene& scene, Model& m_model);
    // Materials, lights and textures re-read from `m_model` (mcpt_update_materials / mcpt_update_texture) after the caller edited
    // Model::materials in place: Ks, Ns, radiance and the Map_Kd images, each of the size it had when this Render was made; same number of
    // materials.  Works on every Render.  Starts the picture again like update().  false (and an unchanged Render and Scene) on failure.
    bool update_materials(Scene& scene, Model& m_model);
    // update that carries the picture over (mcpt_update_vertices_reproject): positions and normals re-read from `m_model`, the
    // camera kept -- or, second form, replaced by `camera` in the same call (Model::camerainfo is not read).  `scene`'s film is treated as by
    // set_camera_reproject: brought to the device, looked up where the new view's surface points WERE, left there as `scene`'s film with at most
    // max_history samples per pixel; the sample numbering goes on.  The radiance carried over is the old scene's: what moved drags its shadows
    // and reflections along until max_history new samples have diluted them.  false on failure (Render and the Scene's samples unchanged).
    bool update_reproject(Scene& scene, Model& m_model, float max_history = 0);
    bool update_reproject(Scene& scene, Model& m_model, const CameraInfo& camera, float max_history = 0);
    // Rigid parts.  set_groups: one group id per face of `m_model`, the Model this Render was made from (MCPT_FLAG_DYNAMIC); the
    // scene as it is now becomes the rest pose; false when faces of two groups share a vertex or a normal.  The film is not touched.
    // update_transforms: one row-major 3x4 matrix [A | t] per group (12 doubles each), applied to the rest pose on the device
    // (mcpt_update_transforms) -- only the matrices cross the bus, Model::vertex is neither read nor written.  Starts the picture again like
    // update(); update_transforms_reproject carries it over like update_reproject.  false (Render and Scene unchanged) on failure.
    bool set_groups(Scene& scene, Model& m_model, const std::vector<uint32_t>& face_group);
    bool update_transforms(Scene& scene, const std::vector<double>& matrices);
    bool update_transforms_reproject(Scene& scene, const std::vector<double>& matrices, float max_history = 0);
    bool update_transforms_reproject(Scene& scene, const std::vector<double>& matrices, const CameraInfo& camera, float max_history = 0);
    // Deforming parts.  set_skin: four bone ids and four weights per vertex of `m_model`, the Model this Render was made from
    // (MCPT_FLAG_DYNAMIC); every normal takes the influences of the vertex it is paired with in a face corner (bone 0 with weight 1 when no
    // face uses it); the scene as it is now becomes the skin's rest pose; false when two corners pair a normal with vertices whose influences
    // differ.  The film is not touched.  update_skin: one row-major 3x4 matrix [A | t] per bone (12 doubles each), blended per vertex and
    // applied to the rest pose on the device (mcpt_update_skin) -- only the matrices cross the bus.  Starts the picture again like update();
    // update_skin_reproject carries it over like update_reproject.  false (Render and Scene unchanged) on failure.
    bool set_skin(Scene& scene, Model& m_model, const std::vector<uint32_t>& vertex_bone, const std::vector<double>& vertex_weight, uint32_t n_bones);
    bool update_skin(Scene& scene, const std::vector<double>& matrices);
    bool update_skin_reproject(Scene& scene, const std::vector<double>& matrices, float max_history = 0);
    bool update_skin_reproject(Scene& scene, const std::vector<double>& matrices, const CameraInfo& camera, float max_history = 0);
    // Dual-quaternion skinning.  set_skin_mode: MCPT_SKIN_LINEAR (the default) or MCPT_SKIN_DUAL_QUATERNION -- how update_skin,
    // update_skin_reproject and update_morph with bones blend a vertex's bones from now on (mcpt_set_skin_mode; before or after set_skin).  In
    // dual-quaternion mode a twisted part keeps its volume; the bones must be rigid (rotation and translation) and the first of a vertex's four
    // bones is its pivot.  Neither film nor scene is touched.  false (nothing changed) on failure.
    bool set_skin_mode(Scene& scene, uint32_t mode);
    // Morph targets.  set_morph: one MorphTarget per target over the vertices of `m_model`, the Model this Render was made from
    // (MCPT_FLAG_DYNAMIC), and -- optionally, as many -- over its normals (none: the normals are not morphed); the scene as it is now becomes
    // the morph's rest pose.  The film is not touched.  update_morph: one weight per target, the weighted displacements added to the rest pose
    // on the device (mcpt_update_morph) -- only the weights cross the bus; with bone_matrices (12 doubles per bone of the skin set with
    // set_skin) the morphed pose is skinned in the same call: morph, then skin.  Starts the picture again like update();
    // update_morph_reproject carries it over like update_reproject.  false (Render and Scene unchanged) on failure.
    bool set_morph(Scene& scene, Model& m_model, const std::vector<MorphTarget>& vertex_targets, const std::vector<MorphTarget>& normal_targets = {});
    bool update_morph(Scene& scene, const std::vector<double>& weights);
    bool update_morph(Scene& scene, const std::vector<double>& weights, const std::vector<double>& bone_matrices);
    bool update_morph_reproject(Scene& scene, const std::vector<double>& weights, float max_history = 0);
    bool update_morph_reproject(Scene& scene, const std::vector<double>& weights, const CameraInfo& camera, float max_history = 0);
    bool update_morph_reproject(Scene& scene, const std::vector<double>& weights, const std::vector<double>& bone_matrices, float max_history = 0);
    bool update_morph_reproject(Scene& scene, const std::vector<double>& weights, const std::vector<double>& bone_matrices, const CameraInfo& camera, float max_history = 0);
    // Baked vertex animation.  set_keyframes: the keyframes of `m_model`, the Model this Render was made from (MCPT_FLAG_DYNAMIC),
    // uploaded once -- one Model per frame (an OBJ sequence; its vertices and normals are taken, the counts must be m_model's), or one vertex array
    // per frame and, optionally, as many normal arrays (none: every update writes the normals the scene has now).  Frame k lies at
    // start_time + k * frame_time; interpolation MCPT_KEYFRAMES_LINEAR / _CATMULL_ROM, wrap MCPT_KEYFRAMES_CLAMP / _LOOP.  The film is not touched.
    // update_keyframes: the scene at `time`, interpolated on the device (mcpt_update_keyframes) -- only the time crosses the bus.  Starts the
    // picture again like update(); update_keyframes_reproject carries it over like update_reproject.  false (Render and Scene unchanged) on failure.
    bool set_keyframes(Scene& scene, Model& m_model, const std::vector<Model*>& frames, double start_time = 0.0, double frame_time = 1.0,
                       uint32_t interpolation = MCPT_KEYFRAMES_LINEAR, uint32_t wrap = MCPT_KEYFRAMES_CLAMP);
    bool set_keyframes(Scene& scene, Model& m_model, const std::vector<std::vector<dvec3>>& vertex_frames, const std::vector<std::vector<dvec3>>& normal_frames,
                       double start_time = 0.0, double frame_time = 1.0, uint32_t interpolation = MCPT_KEYFRAMES_LINEAR, uint32_t wrap = MCPT_KEYFRAMES_CLAMP);
    bool update_keyframes(Scene& scene, double time);
    bool update_keyframes_reproject(Scene& scene, double time, float max_history = 0);
    bool update_keyframes_reproject(Scene& scene, double time, const CameraInfo& camera, float max_history = 0);
    // Each part driven by its own deformer in one call.  set_owners: one owner id (MCPT_OWNER_*) per face of `m_model`, the Model
    // this Render was made from (MCPT_FLAG_DYNAMIC): the one route of update_parts that writes the vertices and normals the face uses (what no
    // face uses: MCPT_OWNER_NONE); false when faces of two owners share a vertex or a normal.  The film is not touched.  update_parts: the routes
    // of `update` run on the device, each writing only the records it owns, then one normals pass and one refit (mcpt_update_parts).  Starts the
    // picture again like update(); update_parts_reproject carries it over like update_reproject.  false (Render and Scene unchanged) on failure.
    bool set_owners(Scene& scene, Model& m_model, const std::vector<uint8_t>& face_owner);
    bool update_parts(Scene& scene, const PartsUpdate& update);
    bool update_parts_reproject(Scene& scene, const PartsUpdate& update, float max_history = 0);
    bool update_parts_reproject(Scene& scene, const PartsUpdate& update, const CameraInfo& camera, float max_history = 0);
    // Smooth normals recomputed on the device after every update.  set_auto_normals: one flag per face of `m_model`, the Model this
    // Render was made from (MCPT_FLAG_DYNAMIC); the normal records that the flagged faces name (an empty face_mask: all records) are from now
    // on recomputed from the deformed faces by every update*() call -- area-weighted, overriding what the call itself wrote for them, Model::normal
    // included; the scene as it is now is the reference pose that fixes each face's side.  The film is not touched.  update_normals: the pass
    // now, nothing moves; starts the picture again like update().  false (Render and Scene unchanged) on failure.
    bool set_auto_normals(Scene& scene, Model& m_model, const std::vector<uint8_t>& face_mask = {});
    bool update_normals(Scene& scene);
    // Faces shown and hidden (mcpt_set_face_visibility).  set_visible: one byte per face of the Model this Render was made from
    // (MCPT_FLAG_DYNAMIC), != 0 = visible; an empty vector shows every face again and frees the mask.  A hidden face cannot be hit by any ray and
    // is no light; the mask stays in force through every later update*() call.  Refused when no light would stay visible.  Starts the picture
    // again like update(); set_visible_reproject carries it over like update_reproject.  false (Render and Scene unchanged) on failure.
    bool set_visible(Scene& scene, const std::vector<uint8_t>& face_visible);
    bool set_visible_reproject(Scene& scene, const std::vector<uint8_t>& face_visible, float max_history = 0);
    bool set_visible_reproject(Scene& scene, const std::vector<uint8_t>& face_visible, const CameraInfo& camera, float max_history = 0);
    // Camera models.  set_camera_model: thin lens (depth of field), orthographic or panorama instead of the pinhole, for
    // render_camera alone (mcpt_set_camera_model) -- render(), denoised() and the *_reproject calls keep describing the pinhole view.  Works on
    // every Render.  Starts the picture again like set_camera().  render_camera: render(scene, spp) with the model's rays (mcpt_render_camera: one
    // pass per sample; needs the wavefront pipeline); with MCPT_CAMERA_PINHOLE the film is render()'s bit for bit.  autofocus: the focus_distance
    // that makes pixel (px, py) sharp -- the distance of what the pinhole sees there, along the view direction (mcpt_autofocus); touches nothing.
    // false (Render and Scene unchanged) on failure.
    bool set_camera_model(Scene& scene, const mcpt_camera_model& model);
    bool render_camera(Scene& scene, uint32_t spp = 1);
    bool autofocus(Scene& scene, int px, int py, double& focus_distance);
    // Surface baking: lighting seen from the surface -- lightmaps and per-vertex lighting (irradiance probes in free space: the
    // light probes below).  set_bake_points: the
    // points to bake, each a face of the Model this Render was made from, barycentrics and a side (mcpt_set_bake_points; mcpt_lightmap_points
    // makes them for a lightmap); an empty vector drops them; the bake film and the bake's sample numbering start again.  bake: `spp` more
    // samples of `seed` for every point (mcpt_bake: one pass per sample; needs the wavefront pipeline).  read_bake: 4 floats per point,
    // {irradiance or outgoing diffuse radiance, samples} (mcpt_read_bake; empty on failure).  None of them touches `scene`, its film or the
    // camera's sample numbering.  false (Render unchanged) on failure.  set_bake_direct: MCPT_BAKE_DIRECT_MIS samples the lights at the bake
    // point itself, MIS-weighted against the cosine ray (mcpt_set_bake_direct); holds for the bakes after it, with or without points.
    bool set_bake_points(Scene& scene, const std::vector<mcpt_bake_point>& points);
    bool set_bake_direct(Scene& scene, uint32_t mode);
    bool bake(Scene& scene, uint32_t spp = 1);
    std::vector<float> read_bake(Scene& scene, uint32_t mode = MCPT_BAKE_IRRADIANCE);
    // Light probes: what an object moving through the scene is lit by.  set_sh_probes: points in free space, world coordinates,
    // 3 doubles each (mcpt_set_sh_probes; mcpt_sh_grid makes a box of them); an empty vector drops them; the accumulators and the probes' own
    // pass numbering start again.  bake_sh: `passes` more passes of 64 rays of `seed` for every probe (mcpt_bake_sh; needs the wavefront
    // pipeline).  read_sh: 27 floats per probe, 9 spherical-harmonic coefficients per channel, of the radiance around the probe or
    // (MCPT_SH_IRRADIANCE) of the irradiance by normal, mcpt_sh_eval's input (mcpt_read_sh; empty on failure).  read_sh_back_share: per probe the
    // share of its rays that first met a surface from behind -- large for a probe inside geometry.  None of them touches `scene`, its film, the
    // bake film or the other sample numberings.  false (Render unchanged) on failure.
    bool set_sh_probes(Scene& scene, const std::vector<double>& positions);
    bool bake_sh(Scene& scene, uint32_t passes = 1);
    std::vector<float> read_sh(Scene& scene, uint32_t mode = MCPT_SH_RADIANCE);
    std::vector<float> read_sh_back_share(Scene& scene);
    // New trees for the geometry as it is now (mcpt_rebuild_trees): after update() / update_transforms() have moved the scene far
    // (mcpt_update_info::wide_area_ratio says how far) the refitted trees are sound and slow; this builds them anew on the context.  The picture
    // goes ON: `scene`'s film, the sample numbering and the feature buffers stay, the scene looks the same from every pixel.  Synchronous.  false
    // (and an unchanged Render) on failure.
    bool rebuild(Scene& scene, uint32_t builder = MCPT_REBUILD_SAME);
    Render(const Render&) = delete;
    Render& operator=(const Render&) = delete;
    bool ok() const { return ctx != nullptr; }
    mcpt_ctx* handle() { return ctx; }
    uint64_t seed = 20251004;                         // the reference seeds from random_device; here reproducible by default
private:
    mcpt_ctx* ctx = nullptr;
    uint32_t next_sample = 0;
    uint32_t next_bake_sample = 0, bake_points = 0;   // §27: the bake film's own numbering; the length of the list set
    uint32_t next_sh_sample = 0, sh_probes = 0;       // §28: the probes' own numbering; the length of the list set
    std::vector<float> film;
    Scene* target = nullptr;                          // the Scene the device film belongs to
    bool dirty = false;                               // the device film holds samples `target` has not seen
    bool features = false;                            // mcpt_render_features has run for this context
    std::vector<Color3b> denoised_rgb;
    std::vector<int32_t> tex_size;                    // width, height of every material's Map_Kd at creation
    void create(Model& m, const mcpt_opts& opts);
    bool restart(Scene& scene);
    bool render_samples(Scene& scene, uint32_t spp, bool camera_model);
    bool film_to_device(Scene& scene, const char* who, bool& ok);
    bool update_reproject(Scene& scene, Model* m_model, const std::vector<double>* matrices, bool bones, const std::vector<double>* weights, const CameraInfo* camera,
                          float max_history, const double* time = nullptr, const PartsUpdate* parts = nullptr, const std::vector<uint8_t>* visible = nullptr);
    uint32_t face_count() const;                      // of the scene the context holds
};
// Fills an mcpt_scene_desc that points INTO `m` (and into the two scratch vectors); valid while all three live.
void model_to_desc(Model& m, std::vector<mcpt_material>& mats, std::vector<mcpt_texture>& texs, mcpt_scene_desc& d);
