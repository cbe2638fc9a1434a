// Render::set_morph / update_morph / update_morph_reproject against the facade classes, for tests/test_morph.py::test_facade_morph.
//   facade_morph a.obj k voff.bin vidx.bin vdelta.bin noff.bin nidx.bin ndelta.bin weight.bin bone.bin boneweight.bin matrix.bin
//                v1.bin n1.bin v2.bin n2.bin out_morphed.bin out_updated.bin out_skinned.bin out_updated2.bin out_reprojected.bin
// voff / vidx / vdelta hold the vertex targets as mcpt_morph_targets lays them out (offsets, indices, 3 doubles per entry), noff / nidx / ndelta
// the normal targets, weight.bin one double per target; bone.bin / boneweight.bin four uint32 ids / four doubles per vertex of a.obj (three
// bones), matrix.bin the three row-major 3x4 matrices.  v1 / n1 hold the arrays the caller expects the weights to produce, v2 / n2 those of the
// weights followed by the bones (fp64, Model::vertex's and Model::normal's sizes).
// A Render made on a.obj gets the weights (update_morph) and renders k frames; a second Render gets v1 / n1 (update) and renders k frames.  The
// first then gets a skin and the weights WITH the bones; the second gets v2 / n2.  The first then carries its film across the way back to the
// rest pose (update_morph_reproject, all weights 0, no bones) and adds one frame.  All five films are written as the Scene holds them.
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
template <class T> static bool slurp_all(const char* path, std::vector<T>& v) {
    FILE* f = std::fopen(path, "rb"); if (!f) return false;
    std::fseek(f, 0, SEEK_END); const long bytes = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize(size_t(bytes) / sizeof(T));
    const bool ok = v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); std::fclose(f); return ok;
}
static bool read_targets(const char* off, const char* idx, const char* dlt, std::vector<MorphTarget>& out) {
    std::vector<uint32_t> o, i; std::vector<double> d;
    if (!slurp_all(off, o) || !slurp_all(idx, i) || !slurp_all(dlt, d) || o.empty() || o.back() != i.size() || d.size() != 3 * i.size()) return false;
    out.resize(o.size() - 1);
    for (size_t k = 0; k + 1 < o.size(); k++) {
        out[k].index.assign(i.begin() + o[k], i.begin() + o[k + 1]); out[k].delta.assign(d.begin() + 3 * size_t(o[k]), d.begin() + 3 * size_t(o[k + 1]));
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 22) return 2;
    Model a(argv[1], true);
    if (!a.ok) return 3;
    const int k = std::atoi(argv[2]);
    const size_t nv = a.vertex.size(), nn = a.normal.size();
    std::vector<MorphTarget> vt, nt; std::vector<double> weight;
    if (!read_targets(argv[3], argv[4], argv[5], vt) || !read_targets(argv[6], argv[7], argv[8], nt) || !slurp_all(argv[9], weight) || weight.size() != vt.size()) return 3;
    std::vector<uint32_t> bone(4 * nv); std::vector<double> bone_weight(4 * nv), m(36);
    if (!slurp(argv[10], bone.data(), bone.size() * sizeof(uint32_t)) || !slurp(argv[11], bone_weight.data(), bone_weight.size() * sizeof(double)) ||
        !slurp(argv[12], m.data(), m.size() * sizeof(double))) return 3;
    std::vector<dvec3> v1(nv), n1(nn), v2(nv), n2(nn);
    if (!slurp(argv[13], v1.data(), sizeof(dvec3) * nv) || !slurp(argv[14], n1.data(), sizeof(dvec3) * nn) || !slurp(argv[15], v2.data(), sizeof(dvec3) * nv) ||
        !slurp(argv[16], n2.data(), sizeof(dvec3) * nn)) return 3;
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h), other(w, h);
    Render r(a, o); r.seed = 17;
    Render u(a, o); u.seed = 17;
    if (!r.ok() || !u.ok()) return 4;
    const std::vector<dvec3> v0 = a.vertex, n0 = a.normal;
    auto through_arrays = [&](const std::vector<dvec3>& v, const std::vector<dvec3>& nr, const char* path) {   // the same scene through update()
        a.vertex = v; a.normal = nr;
        const bool ok = u.update(other, a);
        a.vertex = v0; a.normal = n0;
        if (!ok) return false;
        for (int i = 0; i < k; i++) u.render(other);
        return dump(path, other.pixels(), sizeof(Pixels) * n);
    };
    if (r.update_morph(scene, weight)) return 5;                         // no morph yet: refused
    std::vector<MorphTarget> bad = vt;
    for (MorphTarget& t : bad) if (t.index.size() > 1) { std::swap(t.index[0], t.index[1]); break; }
    if (r.set_morph(scene, a, bad, nt)) return 5;                        // indices not ascending inside a target: refused
    bad = vt; bad[0].delta.push_back(0.0);
    if (r.set_morph(scene, a, bad, nt)) return 5;                        // not 3 doubles per index: refused
    if (r.set_morph(scene, a, vt, std::vector<MorphTarget>(nt.begin(), nt.end() - 1))) return 5;   // another number of normal targets: refused
    if (!r.set_morph(scene, a, vt, nt)) return 5;
    if (r.update_morph(scene, weight, m)) return 5;                      // no skin yet: refused
    for (int i = 0; i < 3; i++) r.render(scene);                         // samples of the old picture: update_morph must drop them
    if (!r.update_morph(scene, weight)) return 6;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[17], scene.pixels(), sizeof(Pixels) * n)) return 7;
    if (!through_arrays(v1, n1, argv[18])) return 8;
    // ---- morph, then skin
    if (!r.set_skin(scene, a, bone, bone_weight, 3u)) return 5;          // (its rest pose is the morphed scene: this call does not read it)
    if (!r.update_morph(scene, weight, m)) return 6;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[19], scene.pixels(), sizeof(Pixels) * n)) return 7;
    if (!through_arrays(v2, n2, argv[20])) return 8;
    // ---- back to the rest pose, the film carried over
    if (!r.update_morph_reproject(scene, std::vector<double>(weight.size(), 0.0), 4.f)) return 9;
    r.render(scene);
    if (!dump(argv[21], scene.pixels(), sizeof(Pixels) * n)) return 7;
    std::printf("%d %d %d\n", w, h, k);
    return 0;
}
