// Stand-alone host check of csrc/shprobe_plan.h for tests/test_shprobe_ref.py: no device is touched, nothing is loaded into Python.
// in.bin: u32 n_grids, then per grid 3 f64 lo, 3 f64 hi, u32 {nx, ny, nz}; u32 n_evals, then per evaluation 27 f32 coefficients and 3 f64 normal.
// out.bin: per grid u32 status (0 = ok) and u32 n, then 3 n f64 positions; per evaluation 3 f64.  Every grid's positions are put through
// sh_check_probes, the rule mcpt_set_sh_probes applies (a list it refuses ends the program with 5), and so is the same list with one coordinate
// made NaN, which it must refuse by naming that probe (6 otherwise).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "shprobe_plan.h"

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb"); FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<uint32_t> head;
    if (!get(in, head, 1)) return 3;
    for (uint32_t c = 0, n_grids = head[0]; c < n_grids; c++) {
        std::vector<double> box; std::vector<uint32_t> dims;
        if (!get(in, box, 6) || !get(in, dims, 3)) return 3;
        std::vector<double> xyz;
        const std::string bad = sh_grid_points(box.data(), box.data() + 3, dims[0], dims[1], dims[2], xyz);
        if (!bad.empty() && !xyz.empty()) return 4;
        const uint32_t n = uint32_t(xyz.size() / 3);
        if (!sh_check_probes(xyz.data(), n).empty()) return 5;
        if (n) {
            std::vector<double> poisoned = xyz;
            const uint32_t at = n / 2;
            poisoned[3 * size_t(at) + 1] = std::numeric_limits<double>::quiet_NaN();
            if (sh_check_probes(poisoned.data(), n).rfind("probe " + std::to_string(at) + ":", 0) != 0) return 6;
        }
        const uint32_t r[2] = {bad.empty() ? 0u : 1u, n};
        std::fwrite(r, sizeof(uint32_t), 2, out);
        if (n) std::fwrite(xyz.data(), sizeof(double), xyz.size(), out);
    }
    if (sh_check_probes(nullptr, 1).empty() || sh_check_probes(nullptr, SH_MAX_PROBES + 1u).empty() || !sh_check_probes(nullptr, 0).empty()) return 7;
    if (!get(in, head, 1)) return 3;
    for (uint32_t e = 0, n_evals = head[0]; e < n_evals; e++) {
        std::vector<float> coeffs; std::vector<double> normal;
        if (!get(in, coeffs, 27) || !get(in, normal, 3)) return 3;
        double rgb[3];
        sh_eval_probe(coeffs.data(), normal.data(), rgb);
        std::fwrite(rgb, sizeof(double), 3, out);
    }
    std::fclose(in); std::fclose(out);
    return 0;
}
