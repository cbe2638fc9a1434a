#include "Render.h"

#include <algorithm>
#include <cstring>
#include <iostream>

void model_to_desc(Model& m, std::vector<mcpt_material>& mats, std::vector<mcpt_texture>& texs, mcpt_scene_desc& d) {
    std::memset(&d, 0, sizeof d);
    mats.resize(m.materials.size()); texs.resize(m.materials.size());
    for (size_t i = 0; i < m.materials.size(); i++) {
        const Material& s = m.materials[i];
        mcpt_material& o = mats[i]; std::memset(&o, 0, sizeof o);
        o.ks[0] = s.Ks.x; o.ks[1] = s.Ks.y; o.ks[2] = s.Ks.z; o.ns = s.Ns;
        o.radiance[0] = s.radiance.x; o.radiance[1] = s.radiance.y; o.radiance[2] = s.radiance.z;
        o.map_kd = int32_t(i);
        texs[i].width = s.Map_Kd->image_w; texs[i].height = s.Map_Kd->image_h;
        texs[i].rgb = reinterpret_cast<const float*>(s.Map_Kd->image_color.data());
    }
    static_assert(sizeof(dvec3) == 24 && sizeof(dvec2) == 16 && sizeof(imat3x4) == 48 && sizeof(Color3f) == 12, "Model arrays are passed through as-is");
    d.vertex = reinterpret_cast<const double*>(m.vertex.data()); d.n_vertex = uint32_t(m.vertex.size());
    d.normal = reinterpret_cast<const double*>(m.normal.data()); d.n_normal = uint32_t(m.normal.size());
    d.texcoord = reinterpret_cast<const double*>(m.texture.data()); d.n_texcoord = uint32_t(m.texture.size());
    d.face = reinterpret_cast<const int32_t*>(m.face.data()); d.n_face = uint32_t(m.face.size());
    d.materials = mats.data(); d.n_materials = uint32_t(mats.size());
    d.textures = texs.data(); d.n_textures = uint32_t(texs.size());
    const CameraInfo& c = m.camerainfo;
    d.camera.eye[0] = c.eye.x; d.camera.eye[1] = c.eye.y; d.camera.eye[2] = c.eye.z;
    d.camera.lookat[0] = c.lookat.x; d.camera.lookat[1] = c.lookat.y; d.camera.lookat[2] = c.lookat.z;
    d.camera.up[0] = c.up.x; d.camera.up[1] = c.up.y; d.camera.up[2] = c.up.z;
    d.camera.fovy = c.fovy; d.camera.width = c.width; d.camera.height = c.height;
}

void Render::create(Model& m, const mcpt_opts& opts) {
    std::vector<mcpt_material> mats; std::vector<mcpt_texture> texs; mcpt_scene_desc d;
    model_to_desc(m, mats, texs, d);
    if (mcpt_create(&d, &opts, &ctx) != MCPT_OK) { std::cerr << "Error: mcpt_create: " << mcpt_last_error() << std::endl; ctx = nullptr; return; }
    film.resize(size_t(d.camera.width) * d.camera.height * 4);
    for (const mcpt_texture& t : texs) { tex_size.push_back(t.width); tex_size.push_back(t.height); }
}
Render::Render(Model& m) { mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; create(m, o); }
Render::Render(Model& m, const mcpt_opts& opts) { create(m, opts); }
Render::Render(Render& other, int device) {
    seed = other.seed;
    if (!other.ctx || mcpt_clone_to_device(other.ctx, device, &ctx) != MCPT_OK) { std::cerr << "Error: mcpt_clone_to_device: " << mcpt_last_error() << std::endl; ctx = nullptr; return; }
    film.resize(other.film.size()); tex_size = other.tex_size;
}
Render::~Render() {
    if (target) { flush_into(*target); target->detach(this); }
    if (ctx) mcpt_destroy(ctx);
}

void Render::render(Scene& scene) { render(scene, 1); }
void Render::render(Scene& scene, uint32_t spp) { (void)render_samples(scene, spp, false); }
bool Render::render_camera(Scene& scene, uint32_t spp) { return render_samples(scene, spp, true); }
bool Render::set_camera_model(Scene& scene, const mcpt_camera_model& model) {
    if (!ctx) return false;
    if (mcpt_set_camera_model(ctx, &model) != MCPT_OK) { std::cerr << "Error: mcpt_set_camera_model: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
bool Render::autofocus(Scene&, int px, int py, double& focus_distance) {
    if (!ctx) return false;
    if (mcpt_autofocus(ctx, px, py, &focus_distance) != MCPT_OK) { std::cerr << "Error: mcpt_autofocus: " << mcpt_last_error() << std::endl; return false; }
    return true;
}
bool Render::set_bake_points(Scene&, const std::vector<mcpt_bake_point>& points) {
    if (!ctx) return false;
    if (mcpt_set_bake_points(ctx, points.data(), uint32_t(points.size())) != MCPT_OK) { std::cerr << "Error: mcpt_set_bake_points: " << mcpt_last_error() << std::endl; return false; }
    bake_points = uint32_t(points.size()); next_bake_sample = 0;
    return true;
}
bool Render::set_bake_direct(Scene&, uint32_t mode) {
    if (!ctx) return false;
    if (mcpt_set_bake_direct(ctx, mode) != MCPT_OK) { std::cerr << "Error: mcpt_set_bake_direct: " << mcpt_last_error() << std::endl; return false; }
    return true;
}
bool Render::bake(Scene&, uint32_t spp) {
    if (!ctx) return false;
    if (mcpt_bake(ctx, spp, seed, next_bake_sample) != MCPT_OK) { std::cerr << "Error: mcpt_bake: " << mcpt_last_error() << std::endl; return false; }
    next_bake_sample += spp;
    return true;
}
std::vector<float> Render::read_bake(Scene&, uint32_t mode) {
    std::vector<float> out(4 * size_t(bake_points));
    if (!ctx || out.empty()) return {};
    if (mcpt_read_bake(ctx, mode, out.data()) != MCPT_OK) { std::cerr << "Error: mcpt_read_bake: " << mcpt_last_error() << std::endl; return {}; }
    return out;
}
bool Render::set_sh_probes(Scene&, const std::vector<double>& positions) {
    if (!ctx) return false;
    if (positions.size() % 3) { std::cerr << "Error: Render::set_sh_probes: 3 doubles per probe" << std::endl; return false; }
    if (mcpt_set_sh_probes(ctx, positions.data(), uint32_t(positions.size() / 3)) != MCPT_OK) { std::cerr << "Error: mcpt_set_sh_probes: " << mcpt_last_error() << std::endl; return false; }
    sh_probes = uint32_t(positions.size() / 3); next_sh_sample = 0;
    return true;
}
bool Render::bake_sh(Scene&, uint32_t passes) {
    if (!ctx) return false;
    if (mcpt_bake_sh(ctx, passes, seed, next_sh_sample) != MCPT_OK) { std::cerr << "Error: mcpt_bake_sh: " << mcpt_last_error() << std::endl; return false; }
    next_sh_sample += passes;
    return true;
}
std::vector<float> Render::read_sh(Scene&, uint32_t mode) {
    std::vector<float> out(27 * size_t(sh_probes));
    if (!ctx || out.empty()) return {};
    if (mcpt_read_sh(ctx, mode, out.data()) != MCPT_OK) { std::cerr << "Error: mcpt_read_sh: " << mcpt_last_error() << std::endl; return {}; }
    return out;
}
std::vector<float> Render::read_sh_back_share(Scene&) {
    std::vector<uint32_t> counts(3 * size_t(sh_probes)); std::vector<float> out(sh_probes);
    if (!ctx || out.empty()) return {};
    if (mcpt_read_sh_film(ctx, nullptr, counts.data()) != MCPT_OK) { std::cerr << "Error: mcpt_read_sh_film: " << mcpt_last_error() << std::endl; return {}; }
    for (size_t p = 0; p < out.size(); p++) out[p] = counts[3 * p] ? float(double(counts[3 * p + 1]) / double(counts[3 * p])) : 0.f;
    return out;
}
// `spp` samples into `scene`: of the pinhole camera (mcpt_render), or -- `camera_model` -- of the model set_camera_model chose (mcpt_render_camera, §25)
bool Render::render_samples(Scene& scene, uint32_t spp, bool camera_model) {
    if (!ctx || spp == 0) return ctx != nullptr;
    if (scene.width() * scene.height() * 4 != int(film.size())) { std::cerr << "Error: Render::render: the Scene's size differs from the camera's" << std::endl; return false; }
    // the film lives in `scene` (several Renders may share one Scene); this Render's share of it stays on the device until read
    if (target != &scene) {
        if (target) { flush_into(*target); target->detach(this); }
        target = &scene;
    }
    scene.attach(this);                               // (flushes whichever other Render held samples for `scene`)
    if ((camera_model ? mcpt_render_camera : mcpt_render)(ctx, spp, seed, next_sample) != MCPT_OK) {
        std::cerr << "Error: " << (camera_model ? "mcpt_render_camera: " : "mcpt_render: ") << mcpt_last_error() << std::endl; return false;
    }
    next_sample += spp; dirty = true;
    return true;
}
mcpt_adaptive_stats Render::render_adaptive(Scene& scene, const mcpt_adaptive_opts* opts) {
    mcpt_adaptive_stats st; std::memset(&st, 0, sizeof st); st.struct_size = sizeof st;
    if (!ctx) return st;
    if (scene.width() * scene.height() * 4 != int(film.size())) { std::cerr << "Error: Render::render_adaptive: the Scene's size differs from the camera's" << std::endl; return st; }
    if (target != &scene) {
        if (target) { flush_into(*target); target->detach(this); }
        target = &scene;
    }
    scene.attach(this);
    if (mcpt_render_adaptive(ctx, seed, next_sample, opts, &st) != MCPT_OK) {
        std::cerr << "Error: mcpt_render_adaptive: " << mcpt_last_error() << std::endl;
        std::memset(&st, 0, sizeof st); st.struct_size = sizeof st; return st;
    }
    // the largest count a tile reached: min_spp doubled once per later pass, the last doubling capped at max_spp
    const uint32_t min_spp = opts && opts->min_spp ? opts->min_spp : 16u, max_spp = opts && opts->max_spp ? opts->max_spp : 1024u;
    uint32_t c = min_spp;
    for (uint32_t p = 1; p < st.passes; p++) c += std::min(c, max_spp - c);
    next_sample += c; dirty = true;
    return st;
}
static mcpt_camera to_camera(const CameraInfo& c) {
    mcpt_camera k; std::memset(&k, 0, sizeof k);
    k.eye[0] = c.eye.x; k.eye[1] = c.eye.y; k.eye[2] = c.eye.z; k.lookat[0] = c.lookat.x; k.lookat[1] = c.lookat.y; k.lookat[2] = c.lookat.z;
    k.up[0] = c.up.x; k.up[1] = c.up.y; k.up[2] = c.up.z; k.fovy = c.fovy; k.width = c.width; k.height = c.height;
    return k;
}
static mcpt_scene_update to_scene_update(const PartsUpdate& u);    // (below, with update_parts)
bool Render::restart(Scene& scene) {
    if (target && target != &scene) { flush_into(*target); target->detach(this); target = nullptr; }   // another Scene's samples are still that Scene's
    scene.clear();                                    // (drops what this Render held for `scene`: scene_gone)
    if (mcpt_clear_accum(ctx) != MCPT_OK) { std::cerr << "Error: mcpt_clear_accum: " << mcpt_last_error() << std::endl; return false; }
    dirty = false; next_sample = 0; features = false;
    return true;
}
bool Render::set_camera(Scene& scene, const CameraInfo& camera) {
    if (!ctx) return false;
    const mcpt_camera k = to_camera(camera);
    if (mcpt_set_camera(ctx, &k) != MCPT_OK) { std::cerr << "Error: mcpt_set_camera: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
bool Render::set_camera_reproject(Scene& scene, const CameraInfo& camera, float max_history) {
    if (!ctx) return false;
    bool ok = false;
    const bool upload = film_to_device(scene, "set_camera_reproject", ok);
    if (!ok) return false;
    const mcpt_camera k = to_camera(camera);
    mcpt_reproject_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.feature_spp = 4; o.feature_seed = seed; o.max_history = max_history;
    if (mcpt_set_camera_reproject(ctx, &k, &o) != MCPT_OK) {
        std::cerr << "Error: mcpt_set_camera_reproject: " << mcpt_last_error() << std::endl;
        if (upload && mcpt_clear_accum(ctx) != MCPT_OK) std::cerr << "Error: mcpt_clear_accum: " << mcpt_last_error() << std::endl;   // the Scene still holds them
        return false;
    }
    if (upload) scene.clear();                        // the samples live on the device now (nothing is held for `scene` at this point: nothing is dropped)
    target = &scene; scene.attach(this);
    dirty = true; features = true;                    // the context holds the new view's features (4 samples of `seed`, what denoised() renders)
    return true;
}
// The whole film of `scene` on the device, as set_camera_reproject needs it: true when a host part had to be uploaded.  `ok` false on failure.
bool Render::film_to_device(Scene& scene, const char* who, bool& ok) {
    ok = false;
    if (scene.width() * scene.height() * 4 != int(film.size())) { std::cerr << "Error: Render::" << who << ": the Scene's size differs from the camera's" << std::endl; return false; }
    if (target && target != &scene) { flush_into(*target); target->detach(this); target = nullptr; }   // another Scene's samples are still that Scene's
    // it is there already unless the Scene holds a host part (or another source does)
    const bool upload = scene.host_samples() || (scene.source() && scene.source() != this);
    if (upload) {
        const float* sum = reinterpret_cast<const float*>(scene.pixels());     // (folds whichever source the Scene has; this Render's device film is empty then)
        if (mcpt_write_accum(ctx, sum) != MCPT_OK) { std::cerr << "Error: mcpt_write_accum: " << mcpt_last_error() << std::endl; return upload; }
    }
    ok = true;
    return upload;
}
bool Render::update_reproject(Scene& scene, Model& m, float max_history) { return update_reproject(scene, &m, nullptr, false, nullptr, nullptr, max_history); }
bool Render::update_reproject(Scene& scene, Model& m, const CameraInfo& camera, float max_history) { return update_reproject(scene, &m, nullptr, false, nullptr, &camera, max_history); }
bool Render::update_transforms_reproject(Scene& scene, const std::vector<double>& matrices, float max_history) { return update_reproject(scene, nullptr, &matrices, false, nullptr, nullptr, max_history); }
bool Render::update_transforms_reproject(Scene& scene, const std::vector<double>& matrices, const CameraInfo& camera, float max_history) {
    return update_reproject(scene, nullptr, &matrices, false, nullptr, &camera, max_history);
}
bool Render::update_skin_reproject(Scene& scene, const std::vector<double>& matrices, float max_history) { return update_reproject(scene, nullptr, &matrices, true, nullptr, nullptr, max_history); }
bool Render::update_skin_reproject(Scene& scene, const std::vector<double>& matrices, const CameraInfo& camera, float max_history) {
    return update_reproject(scene, nullptr, &matrices, true, nullptr, &camera, max_history);
}
bool Render::update_morph_reproject(Scene& scene, const std::vector<double>& weights, float max_history) { return update_reproject(scene, nullptr, nullptr, false, &weights, nullptr, max_history); }
bool Render::update_morph_reproject(Scene& scene, const std::vector<double>& weights, const CameraInfo& camera, float max_history) {
    return update_reproject(scene, nullptr, nullptr, false, &weights, &camera, max_history);
}
bool Render::update_morph_reproject(Scene& scene, const std::vector<double>& weights, const std::vector<double>& bone_matrices, float max_history) {
    return update_reproject(scene, nullptr, &bone_matrices, true, &weights, nullptr, max_history);
}
bool Render::update_morph_reproject(Scene& scene, const std::vector<double>& weights, const std::vector<double>& bone_matrices, const CameraInfo& camera, float max_history) {
    return update_reproject(scene, nullptr, &bone_matrices, true, &weights, &camera, max_history);
}
bool Render::update_keyframes_reproject(Scene& scene, double time, float max_history) { return update_reproject(scene, nullptr, nullptr, false, nullptr, nullptr, max_history, &time); }
bool Render::update_keyframes_reproject(Scene& scene, double time, const CameraInfo& camera, float max_history) {
    return update_reproject(scene, nullptr, nullptr, false, nullptr, &camera, max_history, &time);
}
// The geometry comes from `m` (its arrays), from `matrices` (one 3x4 per group, §16, or per bone, §18), from `weights` (one per morph target,
// §19, with or without the bones' matrices), from `time` (the keyframes' clock, §22) or from several of them at once (`parts`, §23): the rest is
// the same.
bool Render::update_reproject(Scene& scene, Model* m, const std::vector<double>* matrices, bool bones, const std::vector<double>* weights, const CameraInfo* camera,
                              float max_history, const double* time, const PartsUpdate* parts, const std::vector<uint8_t>* visible) {
    if (!ctx) return false;
    const char* const who = visible ? "set_visible_reproject" : parts ? "update_parts_reproject" : m ? "update_reproject" : time ? "update_keyframes_reproject" : weights ? "update_morph_reproject" : bones ? "update_skin_reproject" : "update_transforms_reproject";
    if (parts && (parts->group_matrices.size() % 12 || parts->bone_matrices.size() % 12)) { std::cerr << "Error: Render::" << who << ": need 12 doubles per group and per bone" << std::endl; return false; }
    if (!m && matrices && (matrices->size() % 12 || matrices->empty())) { std::cerr << "Error: Render::" << who << ": need 12 doubles per " << (bones ? "bone" : "group") << std::endl; return false; }
    bool ok = false;
    const bool upload = film_to_device(scene, who, ok);
    if (!ok) return false;
    mcpt_camera k; if (camera) k = to_camera(*camera);
    mcpt_reproject_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.feature_spp = 4; o.feature_seed = seed; o.max_history = max_history;
    mcpt_scene_update pu; if (parts) pu = to_scene_update(*parts);
    const mcpt_status st = visible ? mcpt_set_face_visibility_reproject(ctx, visible->empty() ? nullptr : visible->data(), visible->empty() ? face_count() : uint32_t(visible->size()),
                                                                        camera ? &k : nullptr, &o)   // (§24: the mask in place of the geometry; an empty one drops it)
                           : parts ? mcpt_update_parts_reproject(ctx, &pu, camera ? &k : nullptr, &o)
                          : time ? mcpt_update_keyframes_reproject(ctx, *time, camera ? &k : nullptr, &o)
                       : weights ? mcpt_update_morph_reproject(ctx, weights->data(), uint32_t(weights->size()), matrices ? matrices->data() : nullptr,
                                                                 matrices ? uint32_t(matrices->size() / 12) : 0u, camera ? &k : nullptr, &o)
                         : m ? mcpt_update_vertices_reproject(ctx, reinterpret_cast<const double*>(m->vertex.data()), uint32_t(m->vertex.size()),
                                                              reinterpret_cast<const double*>(m->normal.data()), uint32_t(m->normal.size()), camera ? &k : nullptr, &o)
                     : bones ? mcpt_update_skin_reproject(ctx, matrices->data(), uint32_t(matrices->size() / 12), camera ? &k : nullptr, &o)
                             : mcpt_update_transforms_reproject(ctx, matrices->data(), uint32_t(matrices->size() / 12), camera ? &k : nullptr, &o);
    if (st != MCPT_OK) {
        std::cerr << "Error: mcpt_" << (visible ? "set_face_visibility_reproject" : parts ? "update_parts_reproject" : m ? "update_vertices_reproject" : time ? "update_keyframes_reproject" : weights ? "update_morph_reproject" : bones ? "update_skin_reproject" : "update_transforms_reproject") << ": " << mcpt_last_error() << std::endl;
        if (upload && mcpt_clear_accum(ctx) != MCPT_OK) std::cerr << "Error: mcpt_clear_accum: " << mcpt_last_error() << std::endl;   // the Scene still holds them
        return false;
    }
    if (upload) scene.clear();                        // the samples live on the device now
    target = &scene; scene.attach(this);
    dirty = true; features = true;                    // the context holds the new scene's features (4 samples of `seed`, what denoised() renders)
    return true;
}
bool Render::update(Scene& scene, Model& m) {
    if (!ctx) return false;
    const mcpt_camera k = to_camera(m.camerainfo);
    if (mcpt_update_vertices(ctx, reinterpret_cast<const double*>(m.vertex.data()), uint32_t(m.vertex.size()), reinterpret_cast<const double*>(m.normal.data()),
                             uint32_t(m.normal.size())) != MCPT_OK) { std::cerr << "Error: mcpt_update_vertices: " << mcpt_last_error() << std::endl; return false; }
    if (mcpt_set_camera(ctx, &k) != MCPT_OK) { std::cerr << "Error: mcpt_set_camera: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
bool Render::rebuild(Scene&, uint32_t builder) {
    if (!ctx) return false;
    mcpt_rebuild_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.builder = builder;
    if (mcpt_rebuild_trees(ctx, &o) != MCPT_OK) { std::cerr << "Error: mcpt_rebuild_trees: " << mcpt_last_error() << std::endl; return false; }
    return true;
}
// One group per vertex and per normal from one per face: whatever a face of group g uses belongs to g; what no face uses, to group 0.  (§23: the
// same for owners -- `fn` and `kind` name the caller and its ids in the messages.)
static bool groups_of(const std::vector<imat3x4>& face, const std::vector<uint32_t>& face_group, int column, size_t n, const char* what, std::vector<uint32_t>& out,
                      const char* fn = "set_groups", const char* kind = "groups") {
    const uint32_t none = ~0u;
    out.assign(n, none);
    for (size_t f = 0; f < face.size(); f++)
        for (int c = 0; c < 3; c++) {
            const int i = face[f][c][column];
            if (i < 0 || size_t(i) >= n) { std::cerr << "Error: Render::" << fn << ": face " << f << " names a " << what << " out of range" << std::endl; return false; }
            if (out[size_t(i)] != none && out[size_t(i)] != face_group[f]) {
                std::cerr << "Error: Render::" << fn << ": " << what << " " << i << " is used by faces of " << kind << " " << out[size_t(i)] << " and " << face_group[f]
                          << " (duplicate it in the file)" << std::endl;
                return false;
            }
            out[size_t(i)] = face_group[f];
        }
    for (uint32_t& g : out) if (g == none) g = 0;
    return true;
}
bool Render::set_groups(Scene&, Model& m, const std::vector<uint32_t>& face_group) {
    if (!ctx) return false;
    if (face_group.size() != m.face.size() || face_group.empty()) { std::cerr << "Error: Render::set_groups: need one group per face" << std::endl; return false; }
    std::vector<uint32_t> vg, ng;
    if (!groups_of(m.face, face_group, 0, m.vertex.size(), "vertex", vg) || !groups_of(m.face, face_group, 1, m.normal.size(), "normal", ng)) return false;
    const uint32_t n_groups = *std::max_element(face_group.begin(), face_group.end()) + 1;
    if (mcpt_set_vertex_groups(ctx, vg.data(), uint32_t(vg.size()), ng.data(), uint32_t(ng.size()), n_groups) != MCPT_OK) {
        std::cerr << "Error: mcpt_set_vertex_groups: " << mcpt_last_error() << std::endl; return false;
    }
    return true;
}
// §23.  A record no face uses gets owner 0, MCPT_OWNER_NONE: groups_of's default is the right one.
bool Render::set_owners(Scene&, Model& m, const std::vector<uint8_t>& face_owner) {
    if (!ctx) return false;
    if (face_owner.size() != m.face.size() || face_owner.empty()) { std::cerr << "Error: Render::set_owners: need one owner per face" << std::endl; return false; }
    const std::vector<uint32_t> wide(face_owner.begin(), face_owner.end());
    std::vector<uint32_t> vo, no;
    if (!groups_of(m.face, wide, 0, m.vertex.size(), "vertex", vo, "set_owners", "owners") || !groups_of(m.face, wide, 1, m.normal.size(), "normal", no, "set_owners", "owners")) return false;
    const std::vector<uint8_t> v8(vo.begin(), vo.end()), n8(no.begin(), no.end());
    if (mcpt_set_vertex_owners(ctx, v8.data(), uint32_t(v8.size()), n8.data(), uint32_t(n8.size())) != MCPT_OK) {
        std::cerr << "Error: mcpt_set_vertex_owners: " << mcpt_last_error() << std::endl; return false;
    }
    return true;
}
static mcpt_scene_update to_scene_update(const PartsUpdate& u) {
    mcpt_scene_update p; std::memset(&p, 0, sizeof p);
    p.struct_size = sizeof p; p.routes = u.routes; p.flags = u.flags; p.time = u.time;
    p.group_m3x4 = u.group_matrices.empty() ? nullptr : u.group_matrices.data(); p.n_groups = uint32_t(u.group_matrices.size() / 12);
    p.bone_m3x4 = u.bone_matrices.empty() ? nullptr : u.bone_matrices.data(); p.n_bones = uint32_t(u.bone_matrices.size() / 12);
    p.morph_weight = u.morph_weights.empty() ? nullptr : u.morph_weights.data(); p.n_targets = uint32_t(u.morph_weights.size());
    return p;
}
bool Render::update_parts(Scene& scene, const PartsUpdate& update) {
    if (!ctx) return false;
    if (update.group_matrices.size() % 12 || update.bone_matrices.size() % 12) { std::cerr << "Error: Render::update_parts: need 12 doubles per group and per bone" << std::endl; return false; }
    const mcpt_scene_update p = to_scene_update(update);
    if (mcpt_update_parts(ctx, &p) != MCPT_OK) { std::cerr << "Error: mcpt_update_parts: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
bool Render::update_parts_reproject(Scene& scene, const PartsUpdate& update, float max_history) { return update_reproject(scene, nullptr, nullptr, false, nullptr, nullptr, max_history, nullptr, &update); }
bool Render::update_parts_reproject(Scene& scene, const PartsUpdate& update, const CameraInfo& camera, float max_history) {
    return update_reproject(scene, nullptr, nullptr, false, nullptr, &camera, max_history, nullptr, &update);
}
bool Render::update_transforms(Scene& scene, const std::vector<double>& matrices) {
    if (!ctx) return false;
    if (matrices.size() % 12) { std::cerr << "Error: Render::update_transforms: need 12 doubles per group" << std::endl; return false; }
    if (mcpt_update_transforms(ctx, matrices.data(), uint32_t(matrices.size() / 12)) != MCPT_OK) { std::cerr << "Error: mcpt_update_transforms: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
bool Render::set_skin(Scene&, Model& m, const std::vector<uint32_t>& vertex_bone, const std::vector<double>& vertex_weight, uint32_t n_bones) {
    if (!ctx) return false;
    const size_t K = MCPT_SKIN_INFLUENCES, nv = m.vertex.size(), nn = m.normal.size();
    if (vertex_bone.size() != K * nv || vertex_weight.size() != K * nv) { std::cerr << "Error: Render::set_skin: need 4 bone ids and 4 weights per vertex" << std::endl; return false; }
    // every normal takes the influences of the vertex it is paired with in a face corner; bone 0 with weight 1 where no face uses it
    const size_t none = ~size_t(0);
    std::vector<size_t> first(nn, none);
    for (size_t f = 0; f < m.face.size(); f++)
        for (int c = 0; c < 3; c++) {
            const int vi = m.face[f][c][0], ni = m.face[f][c][1];
            if (vi < 0 || size_t(vi) >= nv || ni < 0 || size_t(ni) >= nn) { std::cerr << "Error: Render::set_skin: face " << f << " names a vertex or normal out of range" << std::endl; return false; }
            size_t& v0 = first[size_t(ni)];
            if (v0 == none) { v0 = size_t(vi); continue; }
            if (std::memcmp(&vertex_bone[K * v0], &vertex_bone[K * size_t(vi)], K * sizeof(uint32_t)) || std::memcmp(&vertex_weight[K * v0], &vertex_weight[K * size_t(vi)], K * sizeof(double))) {
                std::cerr << "Error: Render::set_skin: normal " << ni << " is paired with vertices " << v0 << " and " << vi << ", whose influences differ (duplicate it in the file)" << std::endl;
                return false;
            }
        }
    std::vector<uint32_t> nb(K * nn, 0u); std::vector<double> nw(K * nn, 0.0);
    for (size_t i = 0; i < nn; i++) {
        if (first[i] == none) { nw[K * i] = 1.0; continue; }
        std::copy_n(&vertex_bone[K * first[i]], K, &nb[K * i]); std::copy_n(&vertex_weight[K * first[i]], K, &nw[K * i]);
    }
    if (mcpt_set_vertex_skin(ctx, vertex_bone.data(), vertex_weight.data(), uint32_t(nv), nn ? nb.data() : nullptr, nn ? nw.data() : nullptr, uint32_t(nn), n_bones) != MCPT_OK) {
        std::cerr << "Error: mcpt_set_vertex_skin: " << mcpt_last_error() << std::endl; return false;
    }
    return true;
}
bool Render::update_skin(Scene& scene, const std::vector<double>& matrices) {
    if (!ctx) return false;
    if (matrices.size() % 12) { std::cerr << "Error: Render::update_skin: need 12 doubles per bone" << std::endl; return false; }
    if (mcpt_update_skin(ctx, matrices.data(), uint32_t(matrices.size() / 12)) != MCPT_OK) { std::cerr << "Error: mcpt_update_skin: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
bool Render::set_skin_mode(Scene&, uint32_t mode) {
    if (!ctx) return false;
    if (mcpt_set_skin_mode(ctx, mode) != MCPT_OK) { std::cerr << "Error: mcpt_set_skin_mode: " << mcpt_last_error() << std::endl; return false; }
    return true;
}
// One set of targets flattened into what mcpt_morph_targets points to; false when a target's delta count is not 3 per index.
static bool flatten_targets(const std::vector<MorphTarget>& targets, std::vector<uint32_t>& offset, std::vector<uint32_t>& index, std::vector<double>& delta, mcpt_morph_targets& t) {
    offset.assign(1, 0u);
    for (const MorphTarget& g : targets) {
        if (g.delta.size() != 3 * g.index.size()) return false;
        index.insert(index.end(), g.index.begin(), g.index.end()); delta.insert(delta.end(), g.delta.begin(), g.delta.end());
        offset.push_back(uint32_t(index.size()));
    }
    std::memset(&t, 0, sizeof t); t.struct_size = sizeof t; t.n_targets = uint32_t(targets.size());
    t.target_offset = offset.data(); t.index = index.empty() ? nullptr : index.data(); t.delta = delta.empty() ? nullptr : delta.data();
    return true;
}
bool Render::set_morph(Scene&, Model& m, const std::vector<MorphTarget>& vertex_targets, const std::vector<MorphTarget>& normal_targets) {
    if (!ctx) return false;
    std::vector<uint32_t> vo, vi, no, ni; std::vector<double> vd, nd; mcpt_morph_targets vt, nt;
    if (!flatten_targets(vertex_targets, vo, vi, vd, vt) || !flatten_targets(normal_targets, no, ni, nd, nt)) {
        std::cerr << "Error: Render::set_morph: need 3 doubles of displacement per index" << std::endl; return false;
    }
    if (mcpt_set_vertex_morph(ctx, &vt, uint32_t(m.vertex.size()), normal_targets.empty() ? nullptr : &nt, uint32_t(m.normal.size())) != MCPT_OK) {
        std::cerr << "Error: mcpt_set_vertex_morph: " << mcpt_last_error() << std::endl; return false;
    }
    return true;
}
bool Render::update_morph(Scene& scene, const std::vector<double>& weights) {
    if (!ctx) return false;
    if (mcpt_update_morph(ctx, weights.data(), uint32_t(weights.size()), nullptr, 0u) != MCPT_OK) { std::cerr << "Error: mcpt_update_morph: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
bool Render::update_morph(Scene& scene, const std::vector<double>& weights, const std::vector<double>& bone_matrices) {
    if (!ctx) return false;
    if (bone_matrices.empty() || bone_matrices.size() % 12) { std::cerr << "Error: Render::update_morph: need 12 doubles per bone" << std::endl; return false; }
    if (mcpt_update_morph(ctx, weights.data(), uint32_t(weights.size()), bone_matrices.data(), uint32_t(bone_matrices.size() / 12)) != MCPT_OK) {
        std::cerr << "Error: mcpt_update_morph: " << mcpt_last_error() << std::endl; return false;
    }
    return restart(scene);
}
bool Render::set_keyframes(Scene& scene, Model& m, const std::vector<Model*>& frames, double start_time, double frame_time, uint32_t interpolation, uint32_t wrap) {
    std::vector<std::vector<dvec3>> vf, nf;
    for (const Model* f : frames) {
        if (!f) { std::cerr << "Error: Render::set_keyframes: a null frame" << std::endl; return false; }
        vf.push_back(f->vertex); nf.push_back(f->normal);
    }
    return set_keyframes(scene, m, vf, nf, start_time, frame_time, interpolation, wrap);
}
bool Render::set_keyframes(Scene&, Model& m, const std::vector<std::vector<dvec3>>& vertex_frames, const std::vector<std::vector<dvec3>>& normal_frames,
                           double start_time, double frame_time, uint32_t interpolation, uint32_t wrap) {
    if (!ctx) return false;
    const size_t nv = m.vertex.size(), nn = m.normal.size();
    if (!normal_frames.empty() && normal_frames.size() != vertex_frames.size()) { std::cerr << "Error: Render::set_keyframes: need as many normal frames as vertex frames (or none)" << std::endl; return false; }
    std::vector<double> v, n;                                                // frame after frame, as mcpt_set_vertex_keyframes reads them
    for (size_t k = 0; k < vertex_frames.size(); k++) {
        if (vertex_frames[k].size() != nv || (!normal_frames.empty() && normal_frames[k].size() != nn)) {
            std::cerr << "Error: Render::set_keyframes: frame " << k << " has other vertex or normal counts than the scene" << std::endl; return false;
        }
        const double* p = reinterpret_cast<const double*>(vertex_frames[k].data());
        v.insert(v.end(), p, p + 3 * nv);
        if (normal_frames.empty()) continue;
        const double* q = reinterpret_cast<const double*>(normal_frames[k].data());
        n.insert(n.end(), q, q + 3 * nn);
    }
    mcpt_keyframe_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.interpolation = interpolation; o.wrap = wrap; o.start_time = start_time; o.frame_time = frame_time;
    if (mcpt_set_vertex_keyframes(ctx, v.empty() ? nullptr : v.data(), uint32_t(nv), normal_frames.empty() ? nullptr : n.data(), uint32_t(nn), uint32_t(vertex_frames.size()), &o) != MCPT_OK) {
        std::cerr << "Error: mcpt_set_vertex_keyframes: " << mcpt_last_error() << std::endl; return false;
    }
    return true;
}
bool Render::update_keyframes(Scene& scene, double time) {
    if (!ctx) return false;
    if (mcpt_update_keyframes(ctx, time) != MCPT_OK) { std::cerr << "Error: mcpt_update_keyframes: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
bool Render::set_auto_normals(Scene&, Model& m, const std::vector<uint8_t>& face_mask) {
    if (!ctx) return false;
    const size_t nn = m.normal.size();
    if (!face_mask.empty() && face_mask.size() != m.face.size()) { std::cerr << "Error: Render::set_auto_normals: need one flag per face (or none)" << std::endl; return false; }
    std::vector<uint8_t> mask(nn, face_mask.empty() ? 1 : 0);                // the normal records that the chosen faces name
    for (size_t f = 0; f < m.face.size() && !face_mask.empty(); f++)
        for (int c = 0; c < 3 && face_mask[f]; c++) {
            const int ni = m.face[f][c][1];
            if (ni < 0 || size_t(ni) >= nn) { std::cerr << "Error: Render::set_auto_normals: face " << f << " names a normal out of range" << std::endl; return false; }
            mask[size_t(ni)] = 1;
        }
    mcpt_normals_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.mode = MCPT_NORMALS_AREA;
    if (mcpt_set_auto_normals(ctx, mask.data(), uint32_t(nn), &o) != MCPT_OK) { std::cerr << "Error: mcpt_set_auto_normals: " << mcpt_last_error() << std::endl; return false; }
    return true;
}
bool Render::update_normals(Scene& scene) {
    if (!ctx) return false;
    if (mcpt_update_normals(ctx) != MCPT_OK) { std::cerr << "Error: mcpt_update_normals: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
// §24.  An empty mask means "every face visible": the library takes that as a NULL mask with the scene's own face count.
uint32_t Render::face_count() const {
    mcpt_scene_info info;
    return ctx && mcpt_get_scene_info(ctx, &info) == MCPT_OK ? info.n_tris : 0u;
}
bool Render::set_visible(Scene& scene, const std::vector<uint8_t>& face_visible) {
    if (!ctx) return false;
    const bool all = face_visible.empty();
    if (mcpt_set_face_visibility(ctx, all ? nullptr : face_visible.data(), all ? face_count() : uint32_t(face_visible.size())) != MCPT_OK) {
        std::cerr << "Error: mcpt_set_face_visibility: " << mcpt_last_error() << std::endl; return false;
    }
    return restart(scene);
}
bool Render::set_visible_reproject(Scene& scene, const std::vector<uint8_t>& face_visible, float max_history) {
    return update_reproject(scene, nullptr, nullptr, false, nullptr, nullptr, max_history, nullptr, nullptr, &face_visible);
}
bool Render::set_visible_reproject(Scene& scene, const std::vector<uint8_t>& face_visible, const CameraInfo& camera, float max_history) {
    return update_reproject(scene, nullptr, nullptr, false, nullptr, &camera, max_history, nullptr, nullptr, &face_visible);
}
bool Render::update_materials(Scene& scene, Model& m) {
    if (!ctx) return false;
    std::vector<mcpt_material> mats; std::vector<mcpt_texture> texs; mcpt_scene_desc d;
    model_to_desc(m, mats, texs, d);
    // everything that can be refused is checked before anything changes: the texture sizes here, the rest by mcpt_update_materials itself
    if (2 * texs.size() != tex_size.size()) { std::cerr << "Error: Render::update_materials: the number of materials changed" << std::endl; return false; }
    for (size_t i = 0; i < texs.size(); i++)
        if (texs[i].width != tex_size[2 * i] || texs[i].height != tex_size[2 * i + 1]) {
            std::cerr << "Error: Render::update_materials: the image of material " << i << " changed its size" << std::endl; return false;
        }
    if (mcpt_update_materials(ctx, mats.data(), uint32_t(mats.size())) != MCPT_OK) { std::cerr << "Error: mcpt_update_materials: " << mcpt_last_error() << std::endl; return false; }
    for (size_t i = 0; i < texs.size(); i++)
        if (mcpt_update_texture(ctx, uint32_t(i), &texs[i]) != MCPT_OK) { std::cerr << "Error: mcpt_update_texture: " << mcpt_last_error() << std::endl; return false; }
    return restart(scene);
}
void Render::flush_into(Scene& scene) {
    if (!ctx || !dirty || &scene != target) return;
    dirty = false;
    if (mcpt_read_accum(ctx, film.data()) != MCPT_OK || mcpt_clear_accum(ctx) != MCPT_OK) { std::cerr << "Error: film read-back: " << mcpt_last_error() << std::endl; return; }
    scene.add_film(film.data());
}
const Color3b* Render::tonemapped(Scene& scene) {
    static_assert(sizeof(Color3b) == 3, "mcpt_tonemap_map's image is read as Color3b[]");
    if (!ctx || !dirty || &scene != target) return nullptr;          // (nothing held: the host path shows what an empty film shows)
    const uint8_t* px = nullptr;
    if (mcpt_tonemap_map(ctx, 0, &px) != MCPT_OK) { std::cerr << "Error: mcpt_tonemap_map: " << mcpt_last_error() << std::endl; return nullptr; }
    return reinterpret_cast<const Color3b*>(px);
}
const Color3b* Render::denoised(Scene& scene, const mcpt_denoise_opts* opts) {
    if (!ctx) return nullptr;
    if (scene.width() * scene.height() * 4 != int(film.size())) { std::cerr << "Error: Render::denoised: the Scene's size differs from the camera's" << std::endl; return nullptr; }
    if (!features) {
        if (mcpt_render_features(ctx, 4, seed) != MCPT_OK) { std::cerr << "Error: mcpt_render_features: " << mcpt_last_error() << std::endl; return nullptr; }
        features = true;
    }
    mcpt_status st;
    if (&scene == target && dirty && !scene.host_samples()) {
        st = mcpt_denoise(ctx, nullptr, opts);                    // the whole film is this Render's device film: filtered where it lies
    } else {
        // The film is (partly) on the host: fold it the way getPixelsColor does and upload the sum.  This layer has no HIP of its own, so the
        // upload goes through this Render's device film, which holds nothing once its samples have been handed over (flush_into clears it),
        // and is cleared again afterwards.
        if (target && target != &scene) flush_into(*target);
        const float* sum = reinterpret_cast<const float*>(scene.pixels());     // (folds whichever source the Scene has)
        st = mcpt_write_accum(ctx, sum);
        if (st == MCPT_OK) st = mcpt_denoise(ctx, nullptr, opts);
        if (st == MCPT_OK) st = mcpt_clear_accum(ctx);
    }
    void* dev = nullptr;
    denoised_rgb.resize(size_t(scene.width()) * scene.height());
    if (st == MCPT_OK) st = mcpt_denoised_device_ptr(ctx, &dev);
    if (st == MCPT_OK) st = mcpt_tonemap_buffer(ctx, dev, reinterpret_cast<uint8_t*>(denoised_rgb.data()), 0);
    if (st != MCPT_OK) { std::cerr << "Error: Render::denoised: " << mcpt_last_error() << std::endl; return nullptr; }
    return denoised_rgb.data();
}
void Render::displaced(Scene& scene) { if (&scene == target) target = nullptr; }   // (already flushed by Scene::attach)
void Render::scene_gone(Scene& scene) {
    if (&scene != target) return;
    target = nullptr;
    if (ctx && dirty && mcpt_clear_accum(ctx) != MCPT_OK) std::cerr << "Error: mcpt_clear_accum: " << mcpt_last_error() << std::endl;
    dirty = false;
}
