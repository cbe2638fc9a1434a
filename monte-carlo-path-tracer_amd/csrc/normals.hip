// gfx950 kernel of automatic smooth normals: while mcpt_set_auto_normals is in force, every scene update -- caller arrays, rigid
// groups, skin, morph, morph then skin -- is followed by one pass that recomputes the chosen normal records from the faces as they are NOW, so the
// normals belong to the deformed surface and nothing but the route's own payload crosses the bus.  The pass runs after the route has written
// rf_vtx / rf_nrm and in front of the refit of refit.hip, on the same stream.
//
// The per-record face lists are an inverted index built once on the host (nr_per_record): every record sums the area-weighted normals of its own
// faces in a fixed order (ascending face index), without atomics, so the result is bitwise reproducible.  Floating-point contraction is OFF in this
// file, as in morph.hip: every difference, product, sum, quotient and root below is one correctly rounded fp64 operation, so tests/normals_ref.py
// (numpy, the same order) gives the same array bit for bit.  The kernel reads only the vertices and writes only the normals: it works in place on
// rf_nrm.  Plain C++ loads and vector stores only.
#include "normals.h"

#pragma clang fp contract(off)

uint32_t nr_per_record(const int32_t* face_vertex, const int32_t* face_normal, uint32_t n_face, uint32_t n_normal, const uint8_t* mask,
                       const double* vertex, const double* normal, std::vector<uint32_t>& offset, std::vector<NrEntry>& entry) {
    // the records a face contributes to: its distinct normal indices that the mask lets through, at most three
    auto records = [&](uint32_t f, uint32_t out[3]) {
        const int32_t* c = face_normal + 3 * size_t(f);
        uint32_t n = 0;
        for (int k = 0; k < 3; k++) {
            const uint32_t r = uint32_t(c[k]);
            bool seen = false;
            for (uint32_t j = 0; j < n; j++) seen = seen || out[j] == r;
            if (!seen && (!mask || mask[r])) out[n++] = r;
        }
        return n;
    };
    offset.assign(size_t(n_normal) + 1, 0);
    for (uint32_t f = 0; f < n_face; f++) {
        uint32_t r[3];
        const uint32_t n = records(f, r);
        for (uint32_t j = 0; j < n; j++) offset[size_t(r[j]) + 1]++;
    }
    uint32_t max_valence = 0;
    for (uint32_t i = 0; i < n_normal; i++) { max_valence = offset[size_t(i) + 1] > max_valence ? offset[size_t(i) + 1] : max_valence; offset[size_t(i) + 1] += offset[i]; }
    entry.assign(offset[n_normal], NrEntry{0, 0, 0, 0});
    std::vector<uint32_t> next(offset.begin(), offset.end() - 1);            // per record the place of its next entry
    for (uint32_t f = 0; f < n_face; f++) {                                  // faces ascending: a record's entries come out in that order
        uint32_t r[3];
        const uint32_t n = records(f, r);
        if (!n) continue;
        const int32_t* c = face_vertex + 3 * size_t(f);
        const double* p0 = vertex + 3 * size_t(c[0]); const double* p1 = vertex + 3 * size_t(c[1]); const double* p2 = vertex + 3 * size_t(c[2]);
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2], bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        const double gx = ay * bz - az * by, gy = az * bx - ax * bz, gz = ax * by - ay * bx;
        for (uint32_t j = 0; j < n; j++) {
            const double* m = normal + 3 * size_t(r[j]);
            const double dot = (gx * m[0] + gy * m[1]) + gz * m[2];
            entry[next[r[j]]++] = NrEntry{uint32_t(c[0]), uint32_t(c[1]), uint32_t(c[2]), dot < 0.0 ? 1u : 0u};   // (a NaN dot compares false: 0)
        }
    }
    return max_valence;
}

namespace {

__global__ void __launch_bounds__(NR_BLOCK) nr_normals_kernel(const double* __restrict__ vertex, const uint32_t* __restrict__ offset, const NrEntry* __restrict__ entry,
                                                              double* __restrict__ normal, uint32_t n) {
    const uint32_t i = blockIdx.x * NR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t first = offset[i], last = offset[i + 1];
    if (last <= first) return;                                                      // masked out or unused: the record keeps what the route wrote
    const uint4* e = reinterpret_cast<const uint4*>(entry);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t k = first; k < last; k++) {
        const uint4 q = e[k];                                                       // {v0, v1, v2, flip}
        const double* p0 = vertex + 3 * (size_t)q.x; const double* p1 = vertex + 3 * (size_t)q.y; const double* p2 = vertex + 3 * (size_t)q.z;
        const double x0 = p0[0], y0 = p0[1], z0 = p0[2];
        const double ax = p1[0] - x0, ay = p1[1] - y0, az = p1[2] - z0, bx = p2[0] - x0, by = p2[1] - y0, bz = p2[2] - z0;
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double sigma = q.w ? -1.0 : 1.0;                                      // (a product with +-1 is exact: s + sigma c is one rounded sum)
        sx = sx + sigma * cx; sy = sy + sigma * cy; sz = sz + sigma * cz;
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    if (!(len > 0.0 && len < INFINITY)) return;                                     // (NaN fails both) all faces degenerate: nothing is written
    double* o = normal + 3 * (size_t)i;
    o[0] = sx / len; o[1] = sy / len; o[2] = sz / len;
}

}  // namespace

hipError_t launch_nr_normals(const double* vertex, const uint32_t* offset, const NrEntry* entry, double* normal, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(nr_normals_kernel, dim3((n + NR_BLOCK - 1) / NR_BLOCK), dim3(NR_BLOCK), 0, stream, vertex, offset, entry, normal, n);
    return hipGetLastError();
}
