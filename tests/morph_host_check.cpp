// The host half of morph targets -- mo_per_record and mo_reach of csrc/morph.hip, what mcpt_set_vertex_morph lays its lists out with and
// mcpt_update_morph validates with -- as a stand-alone program (no device is touched), for
// tests/test_morph.py::test_host_conversion_and_reach_are_the_restatement_bit_for_bit.  Built from this file and morph.hip; it may be built with
// the host sanitizers (-Xarch_host -fsanitize=address,undefined).
//   morph_host_check in.bin out.bin
// in.bin: n_cases (u32), then per case n_targets, n_records (u32 each), target_offset (n_targets + 1 u32), index (total u32), delta (3 total
// doubles), R, the weights and D_k (1 + 2 n_targets doubles).  out.bin: per case offset (n_records + 1 u32), per entry its target (total u32)
// and its delta (3 total doubles), then the reach (1 double).
#include <cstdio>
#include <vector>
#include "morph.h"

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb"); if (!f) return 3;
    FILE* o = std::fopen(argv[2], "wb"); if (!o) { std::fclose(f); return 3; }
    std::vector<uint32_t> head;
    int rc = get(f, head, 1) ? 0 : 3;
    for (uint32_t c = 0, n_cases = rc ? 0 : head[0]; c < n_cases && !rc; c++) {
        std::vector<uint32_t> dims, target_offset, index, offset, target; std::vector<double> delta, tail, flat; std::vector<MoEntry> entry;
        if (!get(f, dims, 2) || !get(f, target_offset, size_t(dims[0]) + 1)) { rc = 3; break; }
        const uint32_t n_targets = dims[0], n_records = dims[1], total = target_offset[n_targets];
        if (!get(f, index, total) || !get(f, delta, 3 * size_t(total)) || !get(f, tail, 1 + 2 * size_t(n_targets))) { rc = 3; break; }
        mo_per_record(target_offset.data(), index.data(), delta.data(), n_targets, n_records, offset, entry);
        if (offset.size() != size_t(n_records) + 1 || entry.size() != total) { rc = 4; break; }
        for (const MoEntry& e : entry) { target.push_back(e.target); flat.push_back(e.dx); flat.push_back(e.dy); flat.push_back(e.dz); if (e.pad) rc = 4; }
        const std::vector<double> reach{mo_reach(tail[0], tail.data() + 1, tail.data() + 1 + n_targets, n_targets)};
        if (!put(o, offset) || !put(o, target) || !put(o, flat) || !put(o, reach)) rc = 3;
    }
    std::fclose(f); std::fclose(o);
    return rc;
}
