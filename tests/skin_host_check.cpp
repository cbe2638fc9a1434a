// The host half of linear-blend skinning -- sk_bone_det and sk_row_reach of csrc/skin.hip, what mcpt_update_skin validates with -- as a stand-alone
// program (no device is touched), for tests/test_skin.py::test_host_determinant_and_reach_are_the_restatement_bit_for_bit.  Built from this file,
// skin.hip and transform.hip; it may be built with the host sanitizers (-Xarch_host -fsanitize=address,undefined).
//   skin_host_check in.bin out.bin
// in.bin: per bone 12 doubles [A | t] and a radius; out.bin: per bone det A and the three rows' reach.
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
        double out[4];
        out[0] = sk_bone_det(&in[i]);
        for (int r = 0; r < 3; r++) out[1 + r] = sk_row_reach(&in[i] + 4 * r, in[i + 12]);
        if (std::fwrite(out, sizeof(double), 4, o) != 4) { std::fclose(o); return 3; }
    }
    std::fclose(o);
    return 0;
}
