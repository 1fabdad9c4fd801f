// The host-callable arithmetic of csrc/softmax_codes.h behind a line protocol, for tests/test_softmax_codes_host_cpu.py (built
// there with the host compiler, -ffp-contract=off and its sanitizers).  Halves travel as the decimal value of their 16 bits, floats
// as the decimal value of their 32 bits.  stdin, one request per line, one line of answers each:
//   col C h ...       -> for every full column of C halves: the label, then the C probabilities (smx_column, classes 1 apart)
//   planes C n h ...  -> the same for n columns stored as C planes of n (classes n apart): n labels, then the C planes of n
//   cvt h ...         -> the fp32 of every half (smx_half_bits_to_float)
// A request outside the ranges the host entry of prob.hip admits (C in 1 .. 255, halves below 65536, whole columns) ends the
// program with status 2.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "softmax_codes.h"

static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static bool read_halves(std::istringstream& in, std::vector<uint16_t>& h) {
    long long v;
    while (in >> v) {
        if (v < 0 || v > 65535) return false;
        h.push_back((uint16_t)v);
    }
    return in.eof();
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        std::vector<uint16_t> h;
        if (cmd == "col") {
            int C = 0;
            in >> C;
            if (C < 1 || C > SMX_MAX_CLASSES || !read_halves(in, h) || h.empty() || h.size() % (size_t)C) return 2;
            std::vector<float> p((size_t)C);
            for (size_t k = 0; k < h.size(); k += (size_t)C) {
                const int label = smx_column(h.data() + k, 1, C, p.data(), 1);
                std::printf("%d ", label);
                for (float v : p) std::printf("%u ", bits_of(v));
            }
        } else if (cmd == "planes") {
            int C = 0;
            long long n = 0;
            in >> C >> n;
            if (C < 1 || C > SMX_MAX_CLASSES || n < 1 || n > 65536 || !read_halves(in, h) || h.size() != (size_t)C * (size_t)n) return 2;
            std::vector<float> p(h.size());
            std::vector<int> labels((size_t)n);
            for (long long k = 0; k < n; ++k) labels[(size_t)k] = smx_column(h.data() + k, (size_t)n, C, p.data() + k, (size_t)n);
            for (int l : labels) std::printf("%d ", l);
            for (float v : p) std::printf("%u ", bits_of(v));
        } else if (cmd == "cvt") {
            if (!read_halves(in, h)) return 2;
            for (uint16_t v : h) std::printf("%u ", bits_of(smx_half_bits_to_float(v)));
        } else {
            return 2;
        }
        std::printf("\n");
    }
    return 0;
}
