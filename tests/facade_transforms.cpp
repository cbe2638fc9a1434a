// Render::set_groups / update_transforms / update_transforms_reproject against the facade classes, for
// tests/test_transforms.py::test_facade_transforms.
//   facade_transforms a.obj material k matrix.bin vertex.bin normal.bin out_transformed.bin out_updated.bin out_reprojected.bin
// matrix.bin holds 12 doubles, the row-major 3x4 matrix for the faces of `material` (group 1; everything else is group 0 and stays);
// vertex.bin / normal.bin hold the arrays the caller expects that matrix to produce (fp64, Model::vertex's and Model::normal's sizes).
// A Render made on a.obj gets the matrix (update_transforms) and renders k frames; a second Render made on the same Model gets the arrays
// (update) and renders k frames; the first then carries its film across the way back to the rest pose (update_transforms_reproject) and adds
// one frame.  All three films are written as the Scene holds them.
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
    if (argc < 10) return 2;
    Model a(argv[1], true);
    if (!a.ok) return 3;
    const int mtl = a.material_index(argv[2]);
    if (mtl < 0) return 3;
    const int k = std::atoi(argv[3]);
    std::vector<double> m(24, 0.0);
    m[0] = m[5] = m[10] = 1.0;
    if (!slurp(argv[4], m.data() + 12, 12 * sizeof(double))) return 3;
    std::vector<dvec3> vertex(a.vertex.size()), normal(a.normal.size());
    if (!slurp(argv[5], vertex.data(), sizeof(dvec3) * vertex.size()) || !slurp(argv[6], normal.data(), sizeof(dvec3) * normal.size())) return 3;
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    std::vector<uint32_t> face_group(a.face.size(), 0u), striped(a.face.size());
    for (size_t i = 0; i < a.face.size(); i++) { face_group[i] = a.face[i][0][3] == mtl ? 1u : 0u; striped[i] = uint32_t(i & 1); }
    Scene scene(w, h), other(w, h);
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    if (r.update_transforms(scene, m)) return 5;                        // no groups yet: refused
    if (r.set_groups(scene, a, striped)) return 5;                      // neighbouring faces share vertices: refused
    if (!r.set_groups(scene, a, face_group)) return 5;
    for (int i = 0; i < 3; i++) r.render(scene);                        // samples of the old picture: update_transforms must drop them
    if (!r.update_transforms(scene, m)) return 6;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[7], scene.pixels(), sizeof(Pixels) * n)) return 7;
    {   // ---- the same scene through the arrays
        Render u(a, o); u.seed = 17;
        if (!u.ok()) return 4;
        const std::vector<dvec3> v0 = a.vertex, n0 = a.normal;
        a.vertex = vertex; a.normal = normal;
        const bool ok = u.update(other, a);
        a.vertex = v0; a.normal = n0;
        if (!ok) return 8;
        for (int i = 0; i < k; i++) u.render(other);
        if (!dump(argv[8], other.pixels(), sizeof(Pixels) * n)) return 7;
    }
    // ---- back to the rest pose, the film carried over
    std::vector<double> id(24, 0.0);
    id[0] = id[5] = id[10] = id[12] = id[17] = id[22] = 1.0;
    if (!r.update_transforms_reproject(scene, id, 4.f)) return 9;
    r.render(scene);
    if (!dump(argv[9], scene.pixels(), sizeof(Pixels) * n)) return 7;
    std::printf("%d %d %d\n", w, h, k);
    return 0;
}
