// Render::set_keyframes / update_keyframes / update_keyframes_reproject against the facade classes, for tests/test_keyframes.py::test_facade_keyframes.
//   facade_keyframes a.obj k n_frames interpolation wrap start_time frame_time t1 t2 vframes.bin nframes.bin v1.bin n1.bin v2.bin n2.bin
//                    out_played.bin out_updated.bin out_played_reprojected.bin out_updated_reprojected.bin
// vframes / nframes hold n_frames vertex and normal arrays of a.obj's sizes (fp64, frame after frame); v1 / n1 the arrays the caller expects at
// time t1, v2 / n2 those at t2.
// A Render made on a.obj gets the keyframes and plays t1 (update_keyframes), then renders k frames; a second Render gets v1 / n1 (update) and
// renders k frames.  Then both carry their film over to t2 -- update_keyframes_reproject on the first, update_reproject with v2 / n2 on the
// second -- and add one frame.  All four films are written as the Scenes hold them.
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
    if (argc < 20) return 2;
    Model a(argv[1], true);
    if (!a.ok) return 3;
    const int k = std::atoi(argv[2]);
    const size_t n_frames = size_t(std::atoi(argv[3]));
    const uint32_t interpolation = uint32_t(std::atoi(argv[4])), wrap = uint32_t(std::atoi(argv[5]));
    const double start_time = std::atof(argv[6]), frame_time = std::atof(argv[7]), t1 = std::atof(argv[8]), t2 = std::atof(argv[9]);
    const size_t nv = a.vertex.size(), nn = a.normal.size();
    std::vector<dvec3> vflat(n_frames * nv), nflat(n_frames * nn), v1(nv), n1(nn), v2(nv), n2(nn);
    if (!slurp(argv[10], vflat.data(), sizeof(dvec3) * vflat.size()) || !slurp(argv[11], nflat.data(), sizeof(dvec3) * nflat.size()) ||
        !slurp(argv[12], v1.data(), sizeof(dvec3) * nv) || !slurp(argv[13], n1.data(), sizeof(dvec3) * nn) ||
        !slurp(argv[14], v2.data(), sizeof(dvec3) * nv) || !slurp(argv[15], n2.data(), sizeof(dvec3) * nn)) return 3;
    std::vector<std::vector<dvec3>> vf(n_frames), nf(n_frames);
    for (size_t f = 0; f < n_frames; f++) { vf[f].assign(vflat.begin() + f * nv, vflat.begin() + (f + 1) * nv); nf[f].assign(nflat.begin() + f * nn, nflat.begin() + (f + 1) * nn); }
    mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.max_depth = 6; o.flags = MCPT_FLAG_DETERMINISTIC | MCPT_FLAG_DYNAMIC;
    const int w = a.camerainfo.width, h = a.camerainfo.height;
    const size_t n = size_t(w) * h;
    Scene scene(w, h), other(w, h);
    Render r(a, o); r.seed = 17;
    Render u(a, o); u.seed = 17;
    if (!r.ok() || !u.ok()) return 4;
    const std::vector<dvec3> v0 = a.vertex, n0 = a.normal;
    if (r.update_keyframes(scene, t1)) return 5;                        // no keyframes yet: refused
    std::vector<std::vector<dvec3>> bad = vf; bad[1].pop_back();
    if (r.set_keyframes(scene, a, bad, nf, start_time, frame_time, interpolation, wrap)) return 5;      // a frame of another size: refused
    if (r.set_keyframes(scene, a, vf, std::vector<std::vector<dvec3>>(nf.begin(), nf.end() - 1), start_time, frame_time, interpolation, wrap)) return 5;   // fewer normal frames
    if (r.set_keyframes(scene, a, vf, nf, start_time, 0.0, interpolation, wrap)) return 5;              // frame_time 0: the library's refusal
    if (r.set_keyframes(scene, a, std::vector<Model*>{&a}, start_time, frame_time, interpolation, wrap)) return 5;   // one frame: the library's refusal
    if (!r.set_keyframes(scene, a, std::vector<Model*>{&a, &a}, start_time, frame_time, interpolation, wrap)) return 5;   // Models as frames; replaced below
    if (!r.set_keyframes(scene, a, vf, nf, start_time, frame_time, interpolation, wrap)) return 5;
    for (int i = 0; i < 3; i++) r.render(scene);                         // samples of the old picture: update_keyframes must drop them
    if (!r.update_keyframes(scene, t1)) return 6;
    for (int i = 0; i < k; i++) r.render(scene);
    if (!dump(argv[16], scene.pixels(), sizeof(Pixels) * n)) return 7;
    a.vertex = v1; a.normal = n1;                                        // the same scene through update()
    if (!u.update(other, a)) return 8;
    for (int i = 0; i < k; i++) u.render(other);
    if (!dump(argv[17], other.pixels(), sizeof(Pixels) * n)) return 7;
    // ---- on to t2, the film carried over
    if (!r.update_keyframes_reproject(scene, t2, 4.f)) return 9;
    r.render(scene);
    if (!dump(argv[18], scene.pixels(), sizeof(Pixels) * n)) return 7;
    a.vertex = v2; a.normal = n2;
    if (!u.update_reproject(other, a, 4.f)) return 9;
    u.render(other);
    if (!dump(argv[19], other.pixels(), sizeof(Pixels) * n)) return 7;
    a.vertex = v0; a.normal = n0;
    std::printf("%d %d %d\n", w, h, k);
    return 0;
}
