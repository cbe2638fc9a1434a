// Render::render_adaptive against the facade classes, for tests/test_adaptive.py::test_facade_render_adaptive: one adaptive call into a Scene,
// the device film as mcpt_read_accum returns it and the Scene's pixels after it, then one uniform frame (Render::render) on top.
//   facade_adaptive scene.obj min_spp max_spp threshold out_device.bin out_scene.bin out_next.bin
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
    if (argc < 8) return 2;
    Model model(argv[1], true);
    if (!model.ok) return 3;
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC;
    const int w = model.camerainfo.width, h = model.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h);
    Render a(model, o); a.seed = 17;
    if (!a.ok()) return 4;
    mcpt_adaptive_opts ao; std::memset(&ao, 0, sizeof ao); ao.struct_size = sizeof ao;
    ao.min_spp = uint32_t(std::atoi(argv[2])); ao.max_spp = uint32_t(std::atoi(argv[3])); ao.threshold = float(std::atof(argv[4]));
    const mcpt_adaptive_stats st = a.render_adaptive(scene, &ao);
    if (st.passes == 0) return 5;
    std::vector<float> film(4 * n);
    if (mcpt_read_accum(a.handle(), film.data()) != MCPT_OK || !dump(argv[5], film.data(), film.size() * 4)) return 6;
    if (!dump(argv[6], scene.pixels(), sizeof(Pixels) * n)) return 7;    // folds the device film into the Scene
    float largest = 0.f;
    for (size_t i = 0; i < n; i++) largest = std::max(largest, film[4 * i + 3]);
    a.render(scene);
    if (!dump(argv[7], scene.pixels(), sizeof(Pixels) * n)) return 8;
    std::printf("%d %d %u %.0f\n", w, h, st.passes, largest);
    return 0;
}
