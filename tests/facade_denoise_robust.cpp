// Render::denoised with both opt-in flags of mcpt_denoise_opts against the facade classes, for
// tests/test_denoise_robust.py::test_facade_robust_matches_the_restatement: `frames` frames of the reference's loop (render(scene) per frame),
// then the denoised preview with the emission split and the firefly clamp at firefly_clamp -- plus the film, the features and the emission it
// was filtered with (mcpt_read_features / mcpt_read_emission of the plain C ABI).
//   facade_denoise_robust scene.obj frames depth firefly_clamp out.rgb out_film.bin out_feat.bin out_emis.bin
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
    if (argc < 9) return 2;
    Model model(argv[1], true);
    if (!model.ok) return 3;
    const int frames = std::atoi(argv[2]);
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = uint32_t(std::atoi(argv[3])); o.flags = MCPT_FLAG_CORRECT_SHADOW_T2;
    mcpt_denoise_opts d; std::memset(&d, 0, sizeof d); d.struct_size = sizeof d;
    d.flags = MCPT_DENOISE_SPLIT_EMISSION | MCPT_DENOISE_CLAMP_FIREFLIES; d.firefly_clamp = float(std::atof(argv[4]));
    const int w = model.camerainfo.width, h = model.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h);
    Render a(model, o); a.seed = 21;
    if (!a.ok()) return 4;
    for (int f = 0; f < frames; f++) a.render(scene);
    std::vector<float> emis(4 * n), feat(8 * n);
    if (mcpt_read_emission(a.handle(), emis.data()) != MCPT_ERR_INVALID_ARG) return 5;      // nothing asked for the split yet
    const Color3b* px = a.denoised(scene, &d);                          // the film is on the device: filtered there
    if (!px || !dump(argv[5], px, 3 * n)) return 6;
    if (mcpt_read_features(a.handle(), feat.data()) != MCPT_OK || !dump(argv[7], feat.data(), feat.size() * 4)) return 7;
    if (mcpt_read_emission(a.handle(), emis.data()) != MCPT_OK || !dump(argv[8], emis.data(), emis.size() * 4)) return 8;
    if (!dump(argv[6], scene.pixels(), sizeof(Pixels) * n)) return 9;   // folds the device film into the Scene's host part
    std::printf("%d %d %.0f\n", w, h, scene.pixels()[0].spp);
    return 0;
}
