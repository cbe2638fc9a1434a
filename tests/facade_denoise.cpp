// Render::denoised against the facade classes, for tests/test_denoise.py::test_facade_denoised_matches_the_reference_filter: 8 frames of the
// reference's loop (render(scene) per frame), then the denoised preview twice -- first while the whole film is on the device, then after the
// Scene has folded it into its host part -- plus the film and the features it was filtered with.
//   facade_denoise scene.obj frames depth out_device.rgb out_host.rgb out_film.bin out_feat.bin
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
    const int frames = std::atoi(argv[2]);
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = uint32_t(std::atoi(argv[3])); o.flags = MCPT_FLAG_CORRECT_SHADOW_T2;
    const int w = model.camerainfo.width, h = model.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h);
    Render a(model, o); a.seed = 21;
    if (!a.ok()) return 4;
    for (int f = 0; f < frames; f++) a.render(scene);
    const Color3b* px = a.denoised(scene);                               // the film is on the device: filtered there
    if (!px || !dump(argv[4], px, 3 * n)) return 5;
    std::vector<float> feat(8 * n);
    if (mcpt_read_features(a.handle(), feat.data()) != MCPT_OK || !dump(argv[7], feat.data(), feat.size() * 4)) return 6;
    if (!dump(argv[6], scene.pixels(), sizeof(Pixels) * n)) return 7;    // folds the device film into the Scene's host part
    px = a.denoised(scene);                                              // host part now: uploaded and filtered
    if (!px || !dump(argv[5], px, 3 * n)) return 8;
    std::printf("%d %d %.0f\n", w, h, scene.pixels()[0].spp);
    return 0;
}
