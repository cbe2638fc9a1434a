// Render::set_sh_probes / bake_sh / read_sh against the facade classes, for tests/test_shprobe.py::test_facade_sh.
//   facade_sh a.obj out.bin
// A Render made on a.obj sets the first five probes of the test's list, bakes 2 passes in two calls (the probes' own pass numbering goes on) and
// writes read_sh(MCPT_SH_RADIANCE), then read_sh(MCPT_SH_IRRADIANCE), 27 floats per probe each.  A probe at NaN must be refused and leave the list
// alone; baking without probes must be refused; the Scene's film must stay empty throughout.  The last line: n_probes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "Model.h"
#include "Render.h"
#include "Scene.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    Model a(argv[1], true);
    if (!a.ok) return 3;
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC;
    Scene scene(a.camerainfo.width, a.camerainfo.height);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    const std::vector<double> probes = {0.5, 0.5, 0.5, 0.45, 0.9993, 0.56, 0.5, 0.5, 1.6, 0.5, 1.2, 0.5, 1.3, 0.5, 0.5};
    if (r.bake_sh(scene, 1)) return 5;                                          // no probes yet: refused
    if (!r.set_sh_probes(scene, probes)) return 6;
    std::vector<double> bad(probes); bad[7] = std::nan("");
    if (r.set_sh_probes(scene, bad)) return 7;
    if (!r.bake_sh(scene, 1) || !r.bake_sh(scene, 1)) return 8;
    const std::vector<float> rad = r.read_sh(scene, MCPT_SH_RADIANCE), irr = r.read_sh(scene, MCPT_SH_IRRADIANCE), back = r.read_sh_back_share(scene);
    if (rad.size() != 27 * 5 || irr.size() != rad.size() || back.size() != 5) return 9;
    if (!(back[1] >= 0.4f && back[1] <= 0.6f) || back[0] != 0.f) return 10;     // the probe in the gap above the lamp: its lower half sees the lamp's back
    if (r.read_sh(scene, 2).size() != 0) return 11;                             // an unknown mode
    if (scene.pixels()[0].spp != 0.f) return 12;                                // the picture is not the probes'
    FILE* f = std::fopen(argv[2], "wb"); if (!f) return 13;
    std::fwrite(rad.data(), sizeof(float), rad.size(), f); std::fwrite(irr.data(), sizeof(float), irr.size(), f); std::fclose(f);
    std::printf("%u\n", 5u);
    return 0;
}
