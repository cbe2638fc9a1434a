// The host half of keyframe playback -- kf_segment, kf_weights and kf_reach of csrc/keyframes.hip, what mcpt_update_keyframes turns its time into
// and mcpt_set_vertex_keyframes bounds its frames with -- as a stand-alone program (no device is touched), for
// tests/test_keyframes.py::test_host_segment_weights_and_reach_are_the_restatement_bit_for_bit.  Built from this file and keyframes.hip; it may be
// built with the host sanitizers (-Xarch_host -fsanitize=address,undefined).
//   keyframes_host_check in.bin out.bin
// in.bin: n_cases (u32, then 4 bytes of padding), then per case time, start_time, frame_time, R (4 doubles) and n_frames, interpolation, wrap, 0
// (4 u32).  out.bin: per case k, taps, tap[0..3] (6 u32) and u, w[0..3], the reach (6 doubles).
#include <cstdio>
#include <cstring>
#include <vector>
#include "keyframes.h"

struct Case { double time, start_time, frame_time, radius; uint32_t n_frames, interpolation, wrap, pad; };
struct Answer { uint32_t k, taps, tap[4]; double u, w[4], reach; };
static_assert(sizeof(Case) == 48 && sizeof(Answer) == 72, "the layouts the test writes and reads");

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb"); if (!f) return 3;
    FILE* o = std::fopen(argv[2], "wb"); if (!o) { std::fclose(f); return 3; }
    uint32_t head[2] = {0, 0};
    int rc = std::fread(head, sizeof head, 1, f) == 1 ? 0 : 3;
    std::vector<Case> cases(rc ? 0 : head[0]);
    if (!rc && !cases.empty() && std::fread(cases.data(), sizeof(Case), cases.size(), f) != cases.size()) rc = 3;
    for (size_t c = 0; c < cases.size() && !rc; c++) {
        const Case& q = cases[c];
        const KfBlend b = kf_segment(q.time, q.start_time, q.frame_time, q.n_frames, q.interpolation, q.wrap);
        Answer a; std::memset(&a, 0, sizeof a);
        a.k = b.k; a.taps = b.taps; std::memcpy(a.tap, b.tap, sizeof a.tap);
        for (int t = 0; t < 4; t++) if (b.w[t] != 0.0 || (uint32_t(t) >= b.taps && b.tap[t] != 0)) rc = 4;   // kf_segment leaves the weights 0, and the taps beyond `taps`
        a.u = b.u; kf_weights(b.u, q.interpolation, a.w); a.reach = kf_reach(q.radius, q.interpolation);
        if (std::fwrite(&a, sizeof a, 1, o) != 1) rc = 3;
    }
    std::fclose(f); std::fclose(o);
    return rc;
}
