// Render::set_visible / set_visible_reproject against the facade classes, for tests/test_visibility.py::test_facade_set_visible.
//   facade_visibility a.obj material k out_hidden.bin out_shown.bin out_reprojected.bin
// A Render made on a.obj renders three frames of the whole scene, hides the faces of `material` (set_visible) and renders k frames; shows them
// again (an empty mask) and renders k frames; then hides them with the film carried over (set_visible_reproject) and adds one frame.  A mask that
// hides every face, a mask of the wrong length and any mask on a Render without MCPT_FLAG_DYNAMIC must be refused.  All three films are written
// as the Scene holds them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "Model.h"
#include "Render.h"
#include "Scene.h"

static bool dump(const char* path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path, "wb"); if (!f) return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes; std::fclose(f); return ok;
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    Model a(argv[1], true);
    if (!a.ok) return 3;
    const int mtl = a.material_index(argv[2]);
    if (mtl < 0) return 3;
    const int k = std::atoi(argv[3]);
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    std::vector<uint8_t> mask(a.face.size(), 1), none(a.face.size(), 0), brief(a.face.size() - 1, 1);
    for (size_t i = 0; i < a.face.size(); i++) if (a.face[i][0][3] == mtl) mask[i] = 0;
    Scene scene(w, h);
    {   mcpt_opts fixed = o; fixed.flags = MCPT_FLAG_DETERMINISTIC;
        Render s(a, fixed);
        if (!s.ok()) return 4;
        if (s.set_visible(scene, mask)) return 5; }                       // not a live scene: refused
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    for (int i = 0; i < 3; i++) r.render(scene);                          // samples of the old picture: set_visible must drop them
    if (r.set_visible(scene, none) || r.set_visible(scene, brief)) return 5;   // no light left; one byte short: refused, the picture goes on
    if (scene.pixels()[0].spp != 3.f) return 5;
    if (!r.set_visible(scene, mask)) return 6;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[4], scene.pixels(), sizeof(Pixels) * n)) return 7;
    if (!r.set_visible(scene, {})) return 6;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[5], scene.pixels(), sizeof(Pixels) * n)) return 7;
    if (!r.set_visible_reproject(scene, mask, 4.f)) return 8;
    r.render(scene);
    if (!dump(argv[6], scene.pixels(), sizeof(Pixels) * n)) return 7;
    std::printf("%d %d %d\n", w, h, k);
    return 0;
}
