// The host half of the light probes, pure functions without a device: the validation of a probe list, the cell centres of a box
// and the evaluation of a probe's coefficients for a normal.  mcpt_api.cpp calls them; tests/shprobe_host_check.cpp builds them into a
// stand-alone program.  fp64, one rounding per operation (contraction off inside the functions that compute).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/mcpt.h"

#define SH_MAX_PROBES (0x3ffffffu / 64u)   // 1 048 575: a pass is one probe job of 64 items per probe (mcpt_probe_paths' limit)

// mcpt_set_sh_probes' rule for one list: "" or what is wrong with the first bad probe.
inline std::string sh_check_probes(const double* xyz, uint32_t n) {
    if (n > SH_MAX_PROBES) return "more than 1 048 575 probes";
    if (n && !xyz) return "null list";
    for (uint32_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(xyz[3 * size_t(i) + a])) return "probe " + std::to_string(i) + ": a coordinate is not finite";
    return "";
}

// The centres of the nx x ny x nz cells of the box [lo, hi], x fastest: cell (i, j, k) is probe (k ny + j) nx + i at
// lo + ((i + 0.5) / nx) (hi - lo) per axis.  Returns "" or what is wrong with the description.
inline std::string sh_grid_points(const double* lo, const double* hi, uint32_t nx, uint32_t ny, uint32_t nz, std::vector<double>& xyz) {
#pragma clang fp contract(off)
    xyz.clear();
    if (!lo || !hi) return "null bounds";
    if (nx == 0 || ny == 0 || nz == 0 || uint64_t(nx) * ny > SH_MAX_PROBES || uint64_t(nx) * ny * nz > SH_MAX_PROBES) return "the grid has no cells or more than 1 048 575";
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !std::isfinite(hi[a] - lo[a]) || lo[a] > hi[a]) return "the box is not finite or has lo > hi";
    const uint32_t dim[3] = {nx, ny, nz};
    xyz.resize(3 * size_t(nx) * ny * nz);
    size_t at = 0;
    for (uint32_t k = 0; k < nz; k++)
        for (uint32_t j = 0; j < ny; j++)
            for (uint32_t i = 0; i < nx; i++) {
                const uint32_t cell[3] = {i, j, k};
                for (int a = 0; a < 3; a++) xyz[at++] = lo[a] + ((double(cell[a]) + 0.5) / double(dim[a])) * (hi[a] - lo[a]);
            }
    return "";
}

// The nine real spherical harmonics of bands 0 .. 2 at the unit vector (x, y, z), k = l (l + 1) + m: the projection kernel's formulas in fp64.
inline void sh_basis64(double x, double y, double z, double Y[9]) {
#pragma clang fp contract(off)
    const double c1 = 0.4886025119029199, c2 = 1.0925484305920792;
    Y[0] = 0.28209479177387814; Y[1] = c1 * y; Y[2] = c1 * z; Y[3] = c1 * x; Y[4] = c2 * (x * y); Y[5] = c2 * (y * z);
    Y[6] = 0.31539156525252005 * (3.0 * (z * z) - 1.0); Y[7] = c2 * (x * z); Y[8] = 0.5462742152960396 * ((x * x) - (y * y));
}

// out[c] = sum over k = 0 .. 8, in that order, of coeffs[9 c + k] Y_k(normal / |normal|); 0 for a normal of length 0 or not finite.
inline void sh_eval_probe(const float* coeffs27, const double* normal, double* out_rgb) {
#pragma clang fp contract(off)
    out_rgb[0] = out_rgb[1] = out_rgb[2] = 0.0;
    const double len = std::sqrt((normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return;
    double Y[9];
    sh_basis64(normal[0] / len, normal[1] / len, normal[2] / len, Y);
    for (int c = 0; c < 3; c++) {
        double s = 0.0;
        for (int k = 0; k < 9; k++) s = s + double(coeffs27[9 * c + k]) * Y[k];
        out_rgb[c] = s;
    }
}
