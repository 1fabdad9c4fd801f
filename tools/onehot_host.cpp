// The host-callable arithmetic of csrc/resample_onehot.h behind a line protocol, for tests/test_onehot_resample_cpu.py (built there
// with the host compiler, -ffp-contract=off and its sanitizers).  stdin, one request per line, one line of answers each:
//   tab n_in n_out active         -> for every output index: i0 i1 and the 64 bits of w0 and w1 as decimals (onehot_axis_tap)
//   vol I0 I1 I2 O0 O1 O2 sep v.. -> the O0 * O1 * O2 labels of the resampled [I0][I1][I2] volume v (memory order, sep as
//                                    boa_resample_onehot_u8 takes it), voxel by voxel as k_resample_onehot computes them
// A request outside the ranges the host entry admits (extents 1 .. 4096 here, sep -1 .. 2, labels below 256, a whole volume) ends
// the program with status 2.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "resample_onehot.h"

static unsigned long long bits_of(double d) {
    unsigned long long u;
    std::memcpy(&u, &d, 8);
    return u;
}

static bool extent_ok(long long v) { return v >= 1 && v <= 4096; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "tab") {
            long long n_in = 0, n_out = 0, active = -1;
            in >> n_in >> n_out >> active;
            if (!in || !extent_ok(n_in) || !extent_ok(n_out) || (active != 0 && active != 1)) return 2;
            for (int k = 0; k < (int)n_out; ++k) {
                const OnehotTap t = onehot_axis_tap(k, onehot_zoom_factor((int)n_in, (int)n_out), (int)n_in, (int)n_out, active == 1);
                std::printf("%d %d %llu %llu ", t.i0, t.i1, bits_of(t.w0), bits_of(t.w1));
            }
        } else if (cmd == "vol") {
            long long d[7];
            for (auto& v : d) {
                v = 0;
                if (!(in >> v)) return 2;
            }
            for (int a = 0; a < 6; ++a)
                if (!extent_ok(d[a])) return 2;
            if (d[6] < -1 || d[6] > 2) return 2;
            const size_t ni = (size_t)d[0] * (size_t)d[1] * (size_t)d[2], no = (size_t)d[3] * (size_t)d[4] * (size_t)d[5];
            if (ni > (1u << 22) || no > (1u << 22)) return 2;
            std::vector<uint8_t> v;
            long long x;
            while (in >> x) {
                if (x < 0 || x > 255) return 2;
                v.push_back((uint8_t)x);
            }
            if (!in.eof() || v.size() != ni) return 2;
            const int I[3] = {(int)d[0], (int)d[1], (int)d[2]}, O[3] = {(int)d[3], (int)d[4], (int)d[5]}, sep = (int)d[6];
            std::vector<OnehotTap> tab[3];
            for (int a = 0; a < 3; ++a)
                for (int k = 0; k < O[a]; ++k) tab[a].push_back(onehot_axis_tap(k, onehot_zoom_factor(I[a], O[a]), I[a], O[a], sep != a));
            const bool copy = I[0] == O[0] && I[1] == O[1] && I[2] == O[2];
            for (int o0 = 0; o0 < O[0]; ++o0)
                for (int o1 = 0; o1 < O[1]; ++o1) {
                    const uint8_t* row[4];
                    onehot_rows(v.data(), I[1], I[2], tab[0][(size_t)o0], tab[1][(size_t)o1], row);
                    for (int o2 = 0; o2 < O[2]; ++o2) {
                        const int l = copy ? v[((size_t)o0 * (size_t)I[1] + (size_t)o1) * (size_t)I[2] + (size_t)o2]
                                           : onehot_voxel(row, tab[0][(size_t)o0], tab[1][(size_t)o1], tab[2][(size_t)o2]);
                        std::printf("%d ", l);
                    }
                }
        } else {
            return 2;
        }
        std::printf("\n");
    }
    return 0;
}
