// Render::update_reproject against the facade classes, for tests/test_reproject_motion.py::test_facade_update_reproject.
//   facade_update_reproject a.obj b.obj k H out_before.bin out_same.bin out_moved.bin out_final.bin
// a.obj and b.obj hold the same faces with different vertices (and cameras).  A dynamic Render made on A renders k frames (before), is given A's
// own vertices again with a history cap of H (same: the film read through the Scene, so the call has to bring a host film back to the device),
// then B's vertices and B's camera in one call (moved: the film still on the device) and renders k more frames (final).  All four films are
// written as the Scene holds them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "Model.h"
#include "Render.h"
#include "Scene.h"

static bool dump(const char* path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path, "wb"); if (!f) return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes; std::fclose(f); return ok;
}

int main(int argc, char** argv) {
    if (argc < 9) return 2;
    Model a(argv[1], true), b(argv[2], true);
    if (!a.ok || !b.ok || a.vertex.size() != b.vertex.size() || a.normal.size() != b.normal.size()) return 3;
    const int k = std::atoi(argv[3]); const float H = float(std::atof(argv[4]));
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    {   // a Render without MCPT_FLAG_DYNAMIC refuses, and the Scene keeps its samples
        mcpt_opts plain = o; plain.flags = MCPT_FLAG_DETERMINISTIC;
        Scene s0(w, h);
        Render p(a, plain);
        if (!p.ok()) return 4;
        p.render(s0);
        if (p.update_reproject(s0, a, H)) return 5;
        if (s0.pixels()[0].spp != 1.f || s0.pixels()[n - 1].spp != 1.f) return 5;
    }
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[5], scene.pixels(), sizeof(Pixels) * n)) return 6;       // (pixels() folds the device film into the Scene: the film is on the host now)
    CameraInfo bad = a.camerainfo; bad.width = w + 1;
    if (r.update_reproject(scene, a, bad, H)) return 5;                     // refused: the Scene keeps its samples
    if (!scene.host_samples() || scene.pixels()[0].spp != float(k) || scene.pixels()[n - 1].spp != float(k)) return 5;
    if (!r.update_reproject(scene, a, H)) return 7;
    if (scene.host_samples()) return 7;                                     // the film went back to the device
    mcpt_reproject_info info; mcpt_update_info upd;
    if (mcpt_get_reproject_info(r.handle(), &info) != MCPT_OK || info.reprojections != 1) return 7;
    if (mcpt_get_update_info(r.handle(), &upd) != MCPT_OK || upd.updates != 1) return 7;
    const unsigned long long reused_same = info.pixels_reused;
    if (!r.denoised(scene)) return 7;                                       // the features of the new scene are there
    if (!r.update_reproject(scene, b, b.camerainfo, H)) return 8;           // vertices and camera in one call, from the device film
    if (!dump(argv[7], scene.pixels(), sizeof(Pixels) * n)) return 8;
    {   // the identity update again on a fresh pair, so that `same` is what ONE call leaves
        Scene s2(w, h);
        Render f(a, o); f.seed = 17;
        if (!f.ok()) return 4;
        for (int i = 0; i < k; i++) f.render(s2);
        if (!f.update_reproject(s2, a, H)) return 9;                        // (device film, no upload)
        if (!dump(argv[6], s2.pixels(), sizeof(Pixels) * n)) return 9;
    }
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[8], scene.pixels(), sizeof(Pixels) * n)) return 10;
    std::printf("%d %d %d %llu\n", w, h, k, reused_same);
    return 0;
}
