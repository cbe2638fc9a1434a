// Render::set_skin / update_skin / update_skin_reproject against the facade classes, for tests/test_skin.py::test_facade_skin.
//   facade_skin a.obj k bone.bin weight.bin matrix.bin vertex.bin normal.bin out_skinned.bin out_updated.bin out_reprojected.bin
// bone.bin / weight.bin hold four uint32 ids / four doubles per vertex of a.obj (three bones), matrix.bin the three row-major 3x4 matrices;
// vertex.bin / normal.bin hold the arrays the caller expects those to produce (fp64, Model::vertex's and Model::normal's sizes).
// A Render made on a.obj gets the matrices (update_skin) and renders k frames; a second Render made on the same Model gets the arrays (update)
// and renders k frames; the first then carries its film across the way back to the rest pose (update_skin_reproject) and adds one frame.  All
// three films are written as the Scene holds them.
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
static bool slurp(const char* path, void* p, size_t bytes) {
    FILE* f = std::fopen(path, "rb"); if (!f) return false;
    const bool ok = std::fread(p, 1, bytes, f) == bytes; std::fclose(f); return ok;
}

int main(int argc, char** argv) {
    if (argc < 11) return 2;
    Model a(argv[1], true);
    if (!a.ok) return 3;
    const int k = std::atoi(argv[2]);
    const size_t nv = a.vertex.size();
    std::vector<uint32_t> bone(4 * nv); std::vector<double> weight(4 * nv), m(36);
    if (!slurp(argv[3], bone.data(), bone.size() * sizeof(uint32_t)) || !slurp(argv[4], weight.data(), weight.size() * sizeof(double)) ||
        !slurp(argv[5], m.data(), m.size() * sizeof(double))) return 3;
    std::vector<dvec3> vertex(nv), normal(a.normal.size());
    if (!slurp(argv[6], vertex.data(), sizeof(dvec3) * vertex.size()) || !slurp(argv[7], normal.data(), sizeof(dvec3) * normal.size())) return 3;
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h), other(w, h);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    if (r.update_skin(scene, m)) return 5;                              // no skin yet: refused
    if (r.set_skin(scene, a, bone, weight, 2u)) return 5;               // the ids reach bone 2: refused
    std::vector<double> light = weight; light[0] *= 0.5;
    if (r.set_skin(scene, a, bone, light, 3u)) return 5;                // a record that does not sum to 1: refused
    if (!r.set_skin(scene, a, bone, weight, 3u)) return 5;
    for (int i = 0; i < 3; i++) r.render(scene);                        // samples of the old picture: update_skin must drop them
    if (!r.update_skin(scene, m)) return 6;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[8], scene.pixels(), sizeof(Pixels) * n)) return 7;
    {   // ---- the same scene through the arrays
        Render u(a, o); u.seed = 17;
        if (!u.ok()) return 4;
        const std::vector<dvec3> v0 = a.vertex, n0 = a.normal;
        a.vertex = vertex; a.normal = normal;
        const bool ok = u.update(other, a);
        a.vertex = v0; a.normal = n0;
        if (!ok) return 8;
        for (int i = 0; i < k; i++) u.render(other);
        if (!dump(argv[9], other.pixels(), sizeof(Pixels) * n)) return 7;
    }
    // ---- back to the rest pose, the film carried over
    std::vector<double> id(36, 0.0);
    for (int b = 0; b < 3; b++) id[12 * b] = id[12 * b + 5] = id[12 * b + 10] = 1.0;
    if (!r.update_skin_reproject(scene, id, 4.f)) return 9;
    r.render(scene);
    if (!dump(argv[10], scene.pixels(), sizeof(Pixels) * n)) return 7;
    std::printf("%d %d %d\n", w, h, k);
    return 0;
}
