// Render::set_camera_model / render_camera / autofocus against the facade classes, for tests/test_camera.py::test_facade_camera_model.
//   facade_camera a.obj k px py out_lens.bin
// A Render made on a.obj renders k frames with render(); then the PINHOLE model is set and k frames are rendered with render_camera(): the
// two films must be equal bit for bit.  A model out of range and a pixel outside the film must be refused and leave the picture alone.  Then the
// lens is focused on pixel (px, py) with radius 0.05 and a five-blade aperture, k frames are rendered and the film is written as the Scene holds
// it.  The last line: width height k focus_distance.
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
    if (argc < 6) return 2;
    Model a(argv[1], true);
    if (!a.ok) return 3;
    const int k = std::atoi(argv[2]), px = std::atoi(argv[3]), py = std::atoi(argv[4]);
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    for (int i = 0; i < k; i++) r.render(scene);
    const std::vector<Pixels> plain(scene.pixels(), scene.pixels() + n);
    mcpt_camera_model m; std::memset(&m, 0, sizeof m); m.struct_size = sizeof m; m.model = MCPT_CAMERA_THIN_LENS; m.lens_radius = 0.05;   // focus_distance 0: refused
    double focus = 0.0;
    if (r.set_camera_model(scene, m) || r.autofocus(scene, w, py, focus)) return 5;
    if (scene.pixels()[0].spp != float(k)) return 5;
    m.model = MCPT_CAMERA_PINHOLE;
    if (!r.set_camera_model(scene, m)) return 6;                           // starts the picture again
    if (scene.pixels()[0].spp != 0.f) return 6;
    for (int i = 0; i < k; i++) if (!r.render_camera(scene)) return 7;
    if (std::memcmp(plain.data(), scene.pixels(), sizeof(Pixels) * n) != 0) return 8;
    if (!r.autofocus(scene, px, py, focus) || !(focus > 0.0)) return 9;
    m.model = MCPT_CAMERA_THIN_LENS; m.focus_distance = focus; m.blades = 5;
    if (!r.set_camera_model(scene, m)) return 6;
    if (!r.render_camera(scene, uint32_t(k))) return 7;
    if (!dump(argv[5], scene.pixels(), sizeof(Pixels) * n)) return 10;
    std::printf("%d %d %d %.17g\n", w, h, k, focus);
    return 0;
}
