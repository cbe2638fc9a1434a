// Render::set_bake_direct against the facade classes, for tests/test_bake_direct.py::test_facade_bake_direct.
//   facade_bake_direct a.obj W H spp out.bin
// A Render made on a.obj refuses an unknown mode, takes MCPT_BAKE_DIRECT_MIS before any point is set, bakes the W x H lightmap of
// mcpt_lightmap_points with `spp` samples and writes read_bake(MCPT_BAKE_DIFFUSE), 4 floats per covered texel.  The last line: n_points n_texels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "Model.h"
#include "Render.h"
#include "Scene.h"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    Model a(argv[1], true);
    if (!a.ok) return 3;
    const uint32_t W = uint32_t(std::atoi(argv[2])), H = uint32_t(std::atoi(argv[3])), spp = uint32_t(std::atoi(argv[4]));
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC;
    Scene scene(a.camerainfo.width, a.camerainfo.height);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    std::vector<mcpt_material> mats; std::vector<mcpt_texture> texs; mcpt_scene_desc d;
    model_to_desc(a, mats, texs, d);
    uint32_t n = 0;
    mcpt_lightmap_points(&d, W, H, 0, nullptr, nullptr, &n);
    std::vector<mcpt_bake_point> points(n); std::vector<uint32_t> texel(n);
    if (mcpt_lightmap_points(&d, W, H, n, points.data(), texel.data(), &n) != MCPT_OK || n != points.size() || n == 0) return 5;
    if (r.set_bake_direct(scene, 5u)) return 6;                                // an unknown mode: refused
    if (!r.set_bake_direct(scene, MCPT_BAKE_DIRECT_MIS)) return 7;             // no points yet: the mode is the context's
    if (!r.set_bake_points(scene, points)) return 8;
    if (!r.bake(scene, spp)) return 9;
    const std::vector<float> lit = r.read_bake(scene, MCPT_BAKE_DIFFUSE);
    if (lit.size() != 4 * size_t(n)) return 10;
    for (uint32_t k = 0; k < n; k++) if (lit[4 * size_t(k) + 3] != float(spp)) return 11;
    if (scene.pixels()[0].spp != 0.f) return 12;                                // the picture is not the bake's
    FILE* f = std::fopen(argv[5], "wb"); if (!f) return 13;
    std::fwrite(lit.data(), sizeof(float), lit.size(), f); std::fclose(f);
    std::printf("%u %u\n", n, W * H);
    return 0;
}
