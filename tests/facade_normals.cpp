// Render::set_auto_normals / update_normals against the facade classes, for tests/test_normals.py::test_facade_normals.
//   facade_normals a.obj k facemask.bin v1.bin n1.bin n0.bin out_auto.bin out_arrays.bin out_auto_rest.bin out_arrays_rest.bin
// facemask.bin: one byte per face of a.obj; v1.bin: the moved vertices; n1.bin / n0.bin: the normals the caller expects the pass to leave for
// the moved and for the rest vertices (fp64, Model::vertex's and Model::normal's sizes).
// A Render made on a.obj with auto normals on gets v1 with the STALE normals (update) and renders k frames; a second Render, without the feature,
// gets v1 / n1 and renders k frames.  The first then goes back to the rest vertices, runs update_normals on top (which must change nothing) and
// renders k frames; the second gets the rest vertices with n0.  All four films are written as the Scene holds them.
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
    const size_t nv = a.vertex.size(), nn = a.normal.size();
    std::vector<uint8_t> face_mask(a.face.size());
    std::vector<dvec3> v1(nv), n1(nn), n0(nn);
    if (!slurp(argv[3], face_mask.data(), face_mask.size()) || !slurp(argv[4], v1.data(), sizeof(dvec3) * nv) || !slurp(argv[5], n1.data(), sizeof(dvec3) * nn) ||
        !slurp(argv[6], n0.data(), sizeof(dvec3) * nn)) return 3;
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h), other(w, h);
    Render r(a, o); r.seed = 17;
    Render u(a, o); u.seed = 17;
    mcpt_opts fixed = o; fixed.flags = MCPT_FLAG_DETERMINISTIC;
    Render s(a, fixed);
    if (!r.ok() || !u.ok() || !s.ok()) return 4;
    const std::vector<dvec3> v0 = a.vertex, stale = a.normal;
    auto through_arrays = [&](const std::vector<dvec3>& v, const std::vector<dvec3>& nr, const char* path) {   // the same scene through update()
        a.vertex = v; a.normal = nr;
        const bool ok = u.update(other, a);
        a.vertex = v0; a.normal = stale;
        if (!ok) return false;
        for (int i = 0; i < k; i++) u.render(other);
        return dump(path, other.pixels(), sizeof(Pixels) * n);
    };
    if (r.update_normals(scene)) return 5;                               // auto normals are not set: refused
    if (s.set_auto_normals(scene, a, face_mask)) return 5;               // not a dynamic Render: refused
    if (r.set_auto_normals(scene, a, std::vector<uint8_t>(face_mask.size() + 1, 1))) return 5;   // not one flag per face: refused
    if (!r.set_auto_normals(scene, a, face_mask)) return 5;
    for (int i = 0; i < 3; i++) r.render(scene);                         // samples of the old picture: update must drop them
    a.vertex = v1;                                                       // Model::normal stays the rest pose's: the pass replaces the flagged records
    if (!r.update(scene, a)) return 6;
    a.vertex = v0;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[7], scene.pixels(), sizeof(Pixels) * n)) return 7;
    if (!through_arrays(v1, n1, argv[8])) return 8;
    // ---- back to the rest vertices, then the pass alone on top: idempotent
    if (!r.update(scene, a)) return 6;
    if (!r.update_normals(scene)) return 6;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[9], scene.pixels(), sizeof(Pixels) * n)) return 7;
    if (!through_arrays(v0, n0, argv[10])) return 8;
    mcpt_normals_info info;
    if (mcpt_get_normals_info(r.handle(), &info) != MCPT_OK) return 9;
    std::printf("%d %d %d %u %u\n", w, h, k, info.records, info.updates);
    return 0;
}
