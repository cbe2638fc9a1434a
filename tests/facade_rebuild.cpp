// Render::rebuild against the facade classes, for tests/test_rebuild.py::test_facade_rebuild.
//   facade_rebuild a.obj b.obj j k out_rebuilt.bin out_fresh.bin
// a.obj and b.obj hold the same faces, materials and camera; b has other vertex positions.  A Render made on A gets B's vertices through its own
// Model (update), renders j frames on the refitted trees, is rebuilt -- the picture goes on -- and renders k - j more; a Render made on B renders
// k frames.  Both films are written as the Scene holds them.  Last line: w h k, wide_area_ratio before the rebuild, the rebuild count, and
// wide_tree_hash of the rebuilt and of the fresh context.
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
    Model a(argv[1], true), b(argv[2], true);
    if (!a.ok || !b.ok) return 3;
    if (a.vertex.size() != b.vertex.size() || a.normal.size() != b.normal.size() || a.face.size() != b.face.size()) return 3;
    const int j = std::atoi(argv[3]), k = std::atoi(argv[4]);
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h), fresh_scene(w, h);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    {   // a Render without MCPT_FLAG_DYNAMIC refuses and stays usable
        mcpt_opts plain = o; plain.flags = MCPT_FLAG_DETERMINISTIC;
        Scene s0(w, h);
        Render p(a, plain);
        if (!p.ok() || p.rebuild(s0)) return 5;
        p.render(s0);
    }
    a.vertex = b.vertex; a.normal = b.normal;
    if (!r.update(scene, a)) return 6;
    for (int i = 0; i < j; i++) r.render(scene);
    mcpt_update_info ui; mcpt_rebuild_info ri; mcpt_scene_info si, fi;
    if (mcpt_get_update_info(r.handle(), &ui) != MCPT_OK) return 7;
    if (!r.rebuild(scene)) return 7;                                      // the turntable loop's three lines: if (ratio > R) render.rebuild(scene);
    if (mcpt_get_rebuild_info(r.handle(), &ri) != MCPT_OK || mcpt_get_scene_info(r.handle(), &si) != MCPT_OK) return 7;
    for (int i = j; i < k; i++) r.render(scene);
    if (!dump(argv[5], scene.pixels(), sizeof(Pixels) * n)) return 8;
    {
        Render f(b, o); f.seed = 17;
        if (!f.ok() || mcpt_get_scene_info(f.handle(), &fi) != MCPT_OK) return 4;
        for (int i = 0; i < k; i++) f.render(fresh_scene);
        if (!dump(argv[6], fresh_scene.pixels(), sizeof(Pixels) * n)) return 8;
    }
    std::printf("%d %d %d %.17g %u %llu %llu\n", w, h, k, ui.wide_area_ratio, ri.rebuilds, (unsigned long long)si.wide_tree_hash, (unsigned long long)fi.wide_tree_hash);
    return 0;
}
