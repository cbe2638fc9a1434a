// Stand-alone host check of csrc/visibility_plan.h for tests/test_visibility.py: no device is touched, nothing is loaded into
// Python.  in.bin: u32 n_cases, then per case u32 {n_face, n_materials, has_mask}, n_face mask bytes (when has_mask), n_face u32 face materials,
// n_materials emit bytes.  out.bin: per case u32 {n_hidden, n_hidden_emitters, n_lights} and n_materials u32 visible faces.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "visibility_plan.h"

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb"); FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<uint32_t> head;
    if (!get(in, head, 1)) return 3;
    for (uint32_t c = 0, n = head[0]; c < n; c++) {
        std::vector<uint32_t> dims, face_material; std::vector<uint8_t> mask, emits;
        if (!get(in, dims, 3) || !get(in, mask, dims[2] ? dims[0] : 0) || !get(in, face_material, dims[0]) || !get(in, emits, dims[1])) return 3;
        const VsPlan p = vs_plan(dims[2] ? mask.data() : nullptr, face_material.data(), dims[0], emits.data(), dims[1]);
        const uint32_t r[3] = {p.n_hidden, p.n_hidden_emitters, p.n_lights};
        if (p.visible_faces.size() != dims[1]) return 4;
        std::fwrite(r, sizeof(uint32_t), 3, out);
        if (dims[1]) std::fwrite(p.visible_faces.data(), sizeof(uint32_t), dims[1], out);
    }
    std::fclose(in); std::fclose(out);
    return 0;
}
