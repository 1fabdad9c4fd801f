// The host-callable arithmetic of csrc/j2k_dwt97.h behind a line protocol, for tests/test_j2k_dwt97_host_cpu.py (built there
// with the host compiler, -ffp-contract=off and its sanitizers).  Floats travel as the decimal value of their 32 bits.
// stdin, one request per line, one line of answers each:
//   blast kf bf m ...                     -> the lowest coded plane of every magnitude m (j2k_b_last)
//   deq step_half t b_last t b_last ...   -> the dequantised coefficient of every pair (j2k97_dequant)
//   syn n x ...                           -> the synthesis of n subband samples, low-pass half first (j2k97_pair over every k)
//   sam P signed x ...                    -> the samples (j2k97_sample)
//   frame rows cols levels P signed x ... -> the samples of a coefficient plane in Mallat layout: per level rows, then columns,
//                                            strung together as the kernels of j2k.hip do, then j2k97_sample
// A request outside the ranges the host entry of j2k.hip admits ends the program with status 2.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "j2k_dwt97.h"

static float as_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static int ceil_shift(int n, int d) { return d >= 16 ? 1 : (n + (1 << d) - 1) >> d; }

// n samples at src (stride s_in), low-pass half first -> interleaved at dst (stride s_out); the buffers do not overlap
static void synth(const float* src, size_t s_in, float* dst, size_t s_out, int n) {
    const int nl = (n + 1) / 2;
    for (int k = 0; k < nl; ++k) {
        float e, o;
        j2k97_pair([&](int i) { return src[(size_t)((i & 1) ? nl + (i >> 1) : (i >> 1)) * s_in]; }, k, n, e, o);
        dst[(size_t)(2 * k) * s_out] = e;
        if (2 * k + 1 < n) dst[(size_t)(2 * k + 1) * s_out] = o;
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "blast") {
            int kf = -1, bf = -1;
            long long m;
            in >> kf >> bf;
            if (kf < 0 || kf > 2 || bf < 0 || bf > 29) return 2;
            while (in >> m) {
                if (m < 1 || m >= (1ll << 30)) return 2;
                std::printf("%d ", j2k_b_last((int)m, kf, bf));
            }
        } else if (cmd == "deq") {
            uint32_t sh = 0;
            long long t;
            int bl;
            in >> sh;
            while (in >> t >> bl) {
                const long long m = t < 0 ? -t : t;
                if (m >= (1ll << 30) || bl < 0 || bl > 30 || (m & ((1ll << bl) - 1))) return 2;
                std::printf("%u ", bits_of(j2k97_dequant((int)t, bl, as_float(sh))));
            }
        } else if (cmd == "syn") {
            int n = 0;
            in >> n;
            if (n < 1 || n > 65535) return 2;
            std::vector<float> x(n), y(n);
            for (int i = 0; i < n; ++i) {
                uint32_t u;
                if (!(in >> u)) return 2;
                x[i] = as_float(u);
            }
            synth(x.data(), 1, y.data(), 1, n);
            for (int i = 0; i < n; ++i) std::printf("%u ", bits_of(y[i]));
        } else if (cmd == "sam") {
            int P = 0, sg = -1;
            uint32_t u;
            in >> P >> sg;
            if (P < 1 || P > 16 || (sg & ~1)) return 2;
            while (in >> u) std::printf("%u ", (unsigned)j2k97_sample(as_float(u), P, sg));
        } else if (cmd == "frame") {
            int rows = 0, cols = 0, L = -1, P = 0, sg = -1;
            in >> rows >> cols >> L >> P >> sg;
            if (rows < 1 || rows > 65535 || cols < 1 || cols > 65535 || L < 0 || L > 32 || P < 1 || P > 16 || (sg & ~1)) return 2;
            std::vector<float> a((size_t)rows * cols), b((size_t)rows * cols);
            for (float& v : a) {
                uint32_t u;
                if (!(in >> u)) return 2;
                v = as_float(u);
            }
            for (int r = 1; r <= L; ++r) {
                const int d = L - r, wr = ceil_shift(cols, d), hr = ceil_shift(rows, d);
                for (int y = 0; y < hr; ++y) synth(a.data() + (size_t)y * cols, 1, b.data() + (size_t)y * cols, 1, wr);
                for (int x = 0; x < wr; ++x) synth(b.data() + x, cols, a.data() + x, cols, hr);
            }
            for (float v : a) std::printf("%u ", (unsigned)j2k97_sample(v, P, sg));
        } else {
            return 2;
        }
        std::printf("\n");
    }
    return 0;
}
