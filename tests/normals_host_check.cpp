// Stand-alone check of the host half of automatic normals: nr_per_record of csrc/normals.hip on the cases that
// tests/test_normals.py writes, its offsets, entries and the largest valence written back for the comparison with tests/normals_ref.py.
// No device is touched.  Built by the test, once plainly and once under the host's address and undefined-behaviour sanitizers.
//   in:  u32 n_cases; per case u32 n_face, n_normal, n_vertex, has_mask; i32 face_vertex[3 n_face]; i32 face_normal[3 n_face];
//        u8 mask[n_normal] (when has_mask); f64 vertex[3 n_vertex]; f64 normal[3 n_normal]
//   out: per case u32 offset[n_normal + 1]; u32 entry[4 total]; u32 max_valence
#include <cstdio>
#include <cstdint>
#include <vector>
#include "normals.h"

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: normals_host_check in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, in) != 1) return 3;
    for (uint32_t k = 0; k < n_cases; k++) {
        uint32_t h[4];
        if (fread(h, 4, 4, in) != 4) return 3;
        std::vector<int32_t> fv, fn; std::vector<uint8_t> mask; std::vector<double> vertex, normal;
        if (!get(in, fv, 3 * size_t(h[0])) || !get(in, fn, 3 * size_t(h[0])) || !get(in, mask, h[3] ? h[1] : 0) || !get(in, vertex, 3 * size_t(h[2])) ||
            !get(in, normal, 3 * size_t(h[1]))) return 3;
        std::vector<uint32_t> offset; std::vector<NrEntry> entry;
        const uint32_t max_valence = nr_per_record(fv.data(), fn.data(), h[0], h[1], h[3] ? mask.data() : nullptr, vertex.data(), normal.data(), offset, entry);
        fwrite(offset.data(), 4, offset.size(), out);
        if (!entry.empty()) fwrite(entry.data(), sizeof(NrEntry), entry.size(), out);
        fwrite(&max_valence, 4, 1, out);
    }
    fclose(in); fclose(out);
    return 0;
}
