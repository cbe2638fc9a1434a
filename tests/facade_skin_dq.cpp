// Render::set_skin_mode against the facade classes, for tests/test_skin_dq.py::test_facade_skin_dq.
//   facade_skin_dq a.obj k bone.bin weight.bin matrix.bin vertex.bin normal.bin out_skinned.bin out_updated.bin out_reprojected.bin
// bone.bin / weight.bin hold four uint32 ids / four doubles per vertex of a.obj (three bones), matrix.bin the three row-major 3x4 matrices, all
// rigid; vertex.bin / normal.bin hold the arrays the caller expects DUAL-QUATERNION skinning to make of those (fp64, Model::vertex's and
// Model::normal's sizes).  A Render made on a.obj is put into dual-quaternion mode BEFORE its skin is set, gets the matrices (update_skin) and
// renders k frames; a second Render made on the same Model gets the arrays (update) and renders k frames; the first then carries its film across
// the way back to the rest pose (update_skin_reproject) and adds one frame.  All three films are written as the Scene holds them.
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
    {   // a context without MCPT_FLAG_DYNAMIC has no skinning mode to set
        mcpt_opts fixed = o; fixed.flags = MCPT_FLAG_DETERMINISTIC;
        Render s(a, fixed);
        if (!s.ok()) return 4;
        if (s.set_skin_mode(scene, MCPT_SKIN_DUAL_QUATERNION)) return 5;
    }
    Render r(a, o); r.seed = 17;
    if (!r.ok()) return 4;
    if (r.set_skin_mode(scene, 7u)) return 5;                           // an unknown mode: refused
    if (!r.set_skin_mode(scene, MCPT_SKIN_DUAL_QUATERNION)) return 5;   // before the skin is set
    uint32_t mode = 99u;
    if (mcpt_get_skin_mode(r.handle(), &mode) != MCPT_OK || mode != MCPT_SKIN_DUAL_QUATERNION) return 5;
    if (!r.set_skin(scene, a, bone, weight, 3u)) return 5;
    if (mcpt_get_skin_mode(r.handle(), &mode) != MCPT_OK || mode != MCPT_SKIN_DUAL_QUATERNION) return 5;   // the skin did not reset it
    std::vector<double> scaled = m;
    for (int c = 0; c < 3; c++) scaled[24 + 4 * c + c] *= 0.9;          // bone 2 no longer rigid: refused in this mode ...
    if (r.update_skin(scene, scaled)) return 5;
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
    if (!r.set_skin_mode(scene, MCPT_SKIN_LINEAR) || !r.update_skin(scene, scaled)) return 10;   // ... and taken again by linear blending
    std::printf("%d %d %d\n", w, h, k);
    return 0;
}
