// gfx950 kernels of morph targets: mcpt_update_morph deforms a live scene by one weight per target.  The morph's rest pose
// (vertices and normals as they were when mcpt_set_vertex_morph was called) and, per vertex and per normal, the list of the displacements that
// touch it stay on the device; per call only the table of weights crosses the bus.  The two kernels here write the context's CURRENT arrays
// (rf_vtx / rf_nrm) -- or the scratch arrays that skin.hip's kernels then read as their rest pose -- and the refit of refit.hip follows on the same
// stream, exactly as after mcpt_update_vertices' upload.
//
// The lists are an inverted index: every destination sums its own entries in a fixed order (ascending target id), without atomics, so the result
// is bitwise reproducible.  Floating-point contraction is OFF in this file, as in skin.hip: every product, sum, quotient and root below is one
// correctly rounded fp64 operation, so tests/morph_ref.py (numpy, the same order) gives the same arrays bit for bit.  Every entry is accumulated,
// one whose weight is 0 included: leaving it out would change the sign of a zero.  Plain C++ loads and vector stores only; the weights are
// gathered from global memory (at most 512 KB, read-mostly).
#include "morph.h"

#pragma clang fp contract(off)

void mo_per_record(const uint32_t* target_offset, const uint32_t* index, const double* delta, uint32_t n_targets, uint32_t n_records,
                   std::vector<uint32_t>& offset, std::vector<MoEntry>& entry) {
    const uint32_t total = n_targets ? target_offset[n_targets] : 0;
    offset.assign(size_t(n_records) + 1, 0);
    for (uint32_t e = 0; e < total; e++) offset[size_t(index[e]) + 1]++;
    for (uint32_t i = 0; i < n_records; i++) offset[size_t(i) + 1] += offset[i];
    entry.assign(total, MoEntry{0.0, 0.0, 0.0, 0, 0});
    std::vector<uint32_t> next(offset.begin(), offset.end() - 1);            // per record the place of its next entry
    for (uint32_t k = 0; k < n_targets; k++)                                 // targets ascending: a record's entries come out in that order
        for (uint32_t e = target_offset[k]; e < target_offset[k + 1]; e++) {
            const double* d = delta + 3 * size_t(e);
            entry[next[index[e]]++] = MoEntry{d[0], d[1], d[2], k, 0};
        }
}

double mo_reach(double radius, const double* weight, const double* target_delta, uint32_t n_targets) {
    const double slack = 1.0 + 0x1p-16;
    double sum = radius;
    for (uint32_t k = 0; k < n_targets; k++) sum = sum + fabs(weight[k]) * target_delta[k];
    return slack * sum;
}

namespace {

// A record's morphed position: the rest record plus its entries in stored order.  An entry comes as two 16-byte loads, {dx, dy} and {dz, target};
// the target id lies in the low word of the second one's last double.
struct MoSum {
    double x, y, z; bool touched;
    __device__ MoSum(const double* __restrict__ rest, const uint32_t* __restrict__ offset, const MoEntry* __restrict__ entry, const double* __restrict__ weight, uint32_t i) {
        const uint32_t first = offset[i], last = offset[i + 1];
        const double* p = rest + 3 * (size_t)i;
        x = p[0]; y = p[1]; z = p[2];
        touched = last > first;
        const double2* e = reinterpret_cast<const double2*>(entry);
        for (uint32_t k = first; k < last; k++) {
            const double2 a = e[2 * (size_t)k], b = e[2 * (size_t)k + 1];
            const double w = weight[(uint32_t)__double2loint(b.y)];
            x = x + w * a.x; y = y + w * a.y; z = z + w * b.x;
        }
    }
};

__global__ void __launch_bounds__(MO_BLOCK) mo_vertices_kernel(const double* __restrict__ rest, const uint32_t* __restrict__ offset, const MoEntry* __restrict__ entry,
                                                               const double* __restrict__ weight, double* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const MoSum s(rest, offset, entry, weight, i);
    double* o = out + 3 * (size_t)i;
    o[0] = s.x; o[1] = s.y; o[2] = s.z;
}

__global__ void __launch_bounds__(MO_BLOCK) mo_normals_kernel(const double* __restrict__ rest, const uint32_t* __restrict__ offset, const MoEntry* __restrict__ entry,
                                                              const double* __restrict__ weight, double* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const MoSum s(rest, offset, entry, weight, i);
    const double len = sqrt((s.x * s.x + s.y * s.y) + s.z * s.z);
    const bool unit = s.touched && len > 0.0 && len < INFINITY;                     // (NaN fails both; an untouched record stays the rest pose's bits)
    double* o = out + 3 * (size_t)i;
    o[0] = unit ? s.x / len : s.x; o[1] = unit ? s.y / len : s.y; o[2] = unit ? s.z / len : s.z;
}

inline dim3 mo_grid(uint32_t n) { return dim3((n + MO_BLOCK - 1) / MO_BLOCK); }

}  // namespace

hipError_t launch_mo_vertices(const double* rest, const uint32_t* offset, const MoEntry* entry, const double* weight, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mo_vertices_kernel, mo_grid(n), dim3(MO_BLOCK), 0, stream, rest, offset, entry, weight, out, n);
    return hipGetLastError();
}

hipError_t launch_mo_normals(const double* rest, const uint32_t* offset, const MoEntry* entry, const double* weight, double* out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mo_normals_kernel, mo_grid(n), dim3(MO_BLOCK), 0, stream, rest, offset, entry, weight, out, n);
    return hipGetLastError();
}
