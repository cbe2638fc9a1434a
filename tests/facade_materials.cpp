// Render::update_materials against the facade classes, for tests/test_material_update.py::test_facade_update_materials.
//   facade_materials a.obj b.obj k out_edited.bin out_fresh.bin out_refused.bin out_refused_fresh.bin
// a.obj and b.obj hold the same geometry and the same number of materials; b has other Ks / Ns / radiance / constant colours.  A Render made on A
// renders a few frames, gets B's materials through its own Model (update_materials) and renders k frames; a Render made on B renders k frames.
// Then one more frame and two edits that must be refused (no light left; an image of another size): the Scene's film as it is afterwards, and the
// k + 1 frames of a Render made on B that it must equal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "Model.h"
#include "Render.h"
#include "Scene.h"

static bool dump(const char* path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path, "wb"); if (!f) return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes; std::fclose(f); return ok;
}

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    Model a(argv[1], true), b(argv[2], true);
    if (!a.ok || !b.ok) return 3;
    if (a.face.size() != b.face.size() || a.materials.size() != b.materials.size()) return 3;
    const int k = std::atoi(argv[3]);
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h), fresh_scene(w, h);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    for (int i = 0; i < 3; i++) r.render(scene);                        // samples of the old look: the call below must drop them
    for (size_t i = 0; i < a.materials.size(); i++) {
        Material& m = a.materials[i]; const Material& s = b.materials[i];
        m.Ks = s.Ks; m.Ns = s.Ns; m.radiance = s.radiance;
        m.Map_Kd = std::make_shared<Texture>(*s.Map_Kd);                 // (a copy: the edits below must not reach B)
    }
    if (!r.update_materials(scene, a)) return 5;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[4], scene.pixels(), sizeof(Pixels) * n)) return 6;
    {
        Render f(b, o); f.seed = 17;
        if (!f.ok()) return 4;
        for (int i = 0; i < k; i++) f.render(fresh_scene);
        if (!dump(argv[5], fresh_scene.pixels(), sizeof(Pixels) * n)) return 6;
    }
    // ---- refused edits leave the Render and the Scene as they are
    r.render(scene);                                                     // (a sample on the device when the refusals come)
    {
        const std::vector<Material> keep = a.materials;
        for (Material& m : a.materials) m.radiance = dvec3{0.0, 0.0, 0.0};
        if (r.update_materials(scene, a)) return 7;                      // no light left
        a.materials = keep;
        Texture& t = *a.materials[0].Map_Kd;
        t.image_w = 2; t.image_h = 2; t.image_color.assign(4, t.image_color[0]);
        if (r.update_materials(scene, a)) return 7;                      // an image of another size
    }
    {
        Render f(b, o); f.seed = 17;
        if (!f.ok()) return 4;
        fresh_scene.clear();
        for (int i = 0; i < k + 1; i++) f.render(fresh_scene);
        if (!dump(argv[6], scene.pixels(), sizeof(Pixels) * n) || !dump(argv[7], fresh_scene.pixels(), sizeof(Pixels) * n)) return 6;
    }
    std::printf("%d %d %d\n", w, h, k);
    return 0;
}
