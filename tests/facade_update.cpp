// Render::set_camera and Render::update against the facade classes, for tests/test_scene_update.py::test_facade_set_camera_and_update.
//   facade_update a.obj b.obj k out_cam_moved.bin out_cam_fresh.bin out_upd_moved.bin out_upd_fresh.bin
// a.obj and b.obj hold the same faces and materials; b has other vertex positions, normals and another camera.  A Render made on A is told
// B's camera (set_camera), renders k frames, then gets B's vertices and normals through its own Model (update) and renders k frames; a Render
// made on B renders k frames.  All four films are written as the Scene holds them.
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
    Model a(argv[1], true), b(argv[2], true);
    if (!a.ok || !b.ok) return 3;
    if (a.vertex.size() != b.vertex.size() || a.normal.size() != b.normal.size() || a.face.size() != b.face.size()) return 3;
    const int k = std::atoi(argv[3]);
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h), fresh_scene(w, h);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    for (int i = 0; i < 3; i++) r.render(scene);                        // samples of the old picture: both calls below must drop them
    // ---- camera alone: A's geometry seen through B's camera
    if (!r.set_camera(scene, b.camerainfo)) return 5;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[4], scene.pixels(), sizeof(Pixels) * n)) return 6;
    {
        Model a_cam(argv[1], true); a_cam.camerainfo = b.camerainfo;
        Render f(a_cam, o); f.seed = 17;
        if (!f.ok()) return 4;
        for (int i = 0; i < k; i++) f.render(fresh_scene);
        if (!dump(argv[5], fresh_scene.pixels(), sizeof(Pixels) * n)) return 6;
    }
    // ---- vertices, normals and camera re-read from the Model
    a.vertex = b.vertex; a.normal = b.normal; a.camerainfo = b.camerainfo;
    if (!r.update(scene, a)) return 7;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[6], scene.pixels(), sizeof(Pixels) * n)) return 8;
    {
        Scene s2(w, h);
        Render f(b, o); f.seed = 17;
        if (!f.ok()) return 4;
        for (int i = 0; i < k; i++) f.render(s2);
        if (!dump(argv[7], s2.pixels(), sizeof(Pixels) * n)) return 8;
    }
    std::printf("%d %d %d\n", w, h, k);
    return 0;
}
