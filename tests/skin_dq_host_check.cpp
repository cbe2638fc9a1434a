// The host half of dual-quaternion skinning -- sk_bone_dualquat, sk_bone_gram, sk_bone_rigid and sk_dq_reach of csrc/skin.hip, what mcpt_update_skin
// validates and stages with in MCPT_SKIN_DUAL_QUATERNION mode -- as a stand-alone program (no device is touched), for
// tests/test_skin_dq.py::test_host_dual_quaternions_rigid_check_and_reach_are_the_restatement_bit_for_bit.  Built from this file, skin.hip and
// transform.hip; it may be built with the host sanitizers (-Xarch_host -fsanitize=address,undefined).
//   skin_dq_host_check in.bin out.bin
// in.bin: per bone 12 doubles [A | t] and a radius; out.bin: per bone the 8 doubles of its dual quaternion, the 6 entries of A^T A, 1.0 or 0.0 for
// "rigid", and the reach.
#include <cstdio>
#include <vector>
#include "skin.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb"); if (!f) return 3;
    std::vector<double> in; double x[13];
    while (std::fread(x, sizeof(double), 13, f) == 13) in.insert(in.end(), x, x + 13);
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb"); if (!o) return 3;
    for (size_t i = 0; i < in.size(); i += 13) {
        double out[16];
        sk_bone_dualquat(&in[i], out);
        sk_bone_gram(&in[i], out + 8);
        out[14] = sk_bone_rigid(&in[i]) ? 1.0 : 0.0;
        out[15] = sk_dq_reach(&in[i], in[i + 12]);
        if (std::fwrite(out, sizeof(double), 16, o) != 16) { std::fclose(o); return 3; }
    }
    std::fclose(o);
    return 0;
}
