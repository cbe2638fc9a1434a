// Stand-alone host check of csrc/bake_plan.h for tests/test_bake_ref.py: no device is touched, nothing is loaded into Python.
// in.bin: u32 n_cases, then per case u32 {width, height, n_texcoord, n_face}, 2 n_texcoord f64 texcoords, 12 n_face i32 face records.
// out.bin: per case u32 status (0 = ok) and u32 n, then n 16-byte points and n u32 texels.  After the map every point is put through
// bk_check_points, the rule mcpt_set_bake_points applies: a point it refuses ends the program with 5.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bake_plan.h"

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb"); FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<uint32_t> head;
    if (!get(in, head, 1)) return 3;
    for (uint32_t c = 0, n_cases = head[0]; c < n_cases; c++) {
        std::vector<uint32_t> dims; std::vector<double> texcoord; std::vector<int32_t> face;
        if (!get(in, dims, 4) || !get(in, texcoord, 2 * size_t(dims[2])) || !get(in, face, 12 * size_t(dims[3]))) return 3;
        mcpt_scene_desc d; std::memset(&d, 0, sizeof d);
        d.texcoord = texcoord.data(); d.n_texcoord = dims[2]; d.face = face.data(); d.n_face = dims[3];
        std::vector<mcpt_bake_point> points; std::vector<uint32_t> texel;
        const std::string bad = bk_lightmap_points(&d, dims[0], dims[1], points, texel);
        if (points.size() != texel.size()) return 4;
        if (!bk_check_points(points.data(), uint32_t(points.size()), dims[3]).empty()) return 5;
        const uint32_t r[2] = {bad.empty() ? 0u : 1u, uint32_t(points.size())};
        std::fwrite(r, sizeof(uint32_t), 2, out);
        if (!points.empty()) { std::fwrite(points.data(), sizeof(mcpt_bake_point), points.size(), out); std::fwrite(texel.data(), sizeof(uint32_t), texel.size(), out); }
    }
    std::fclose(in); std::fclose(out);
    return 0;
}
