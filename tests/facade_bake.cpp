// Render::set_bake_points / bake / read_bake against the facade classes, for tests/test_bake.py::test_facade_bake.
//   facade_bake a.obj W H spp out.bin
// A Render made on a.obj bakes the W x H lightmap of mcpt_lightmap_points with `spp` samples in two calls (spp - 1, then 1: the bake's own sample
// numbering goes on) and writes read_bake(MCPT_BAKE_DIFFUSE), 4 floats per covered texel, then the texels.  A point outside its triangle must be
// refused and leave the list alone; the Scene's film must stay empty throughout.  The last line: n_points n_texels.
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
    if (mcpt_lightmap_points(&d, W, H, 0, nullptr, nullptr, &n) == MCPT_OK && n != 0) return 5;     // the count: capacity 0 is refused unless nothing is covered
    std::vector<mcpt_bake_point> points(n); std::vector<uint32_t> texel(n);
    if (mcpt_lightmap_points(&d, W, H, n, points.data(), texel.data(), &n) != MCPT_OK || n != points.size() || n == 0) return 5;
    if (r.bake(scene, 1)) return 6;                                            // no points yet: refused
    if (!r.set_bake_points(scene, points)) return 7;
    std::vector<mcpt_bake_point> bad(points); bad[n / 2].u = 0.75f; bad[n / 2].v = 0.5f;
    if (r.set_bake_points(scene, bad)) return 8;
    if (spp > 1 && !r.bake(scene, spp - 1)) return 9;
    if (!r.bake(scene, 1)) return 9;
    const std::vector<float> lit = r.read_bake(scene, MCPT_BAKE_DIFFUSE);
    if (lit.size() != 4 * size_t(n)) return 10;
    for (uint32_t k = 0; k < n; k++) if (lit[4 * size_t(k) + 3] != float(spp)) return 11;
    if (scene.pixels()[0].spp != 0.f) return 12;                                // the picture is not the bake's
    FILE* f = std::fopen(argv[5], "wb"); if (!f) return 13;
    std::fwrite(lit.data(), sizeof(float), lit.size(), f); std::fwrite(texel.data(), sizeof(uint32_t), texel.size(), f); std::fclose(f);
    std::printf("%u %u\n", n, W * H);
    return 0;
}
