// The host-callable parts of csrc/deflate_codes.h behind a line protocol, for tests/test_deflate_codes_host_cpu.py (built there
// with the host compiler and its sanitizers).  stdin, one request per line:
//   len                       -> "sym ebits eval" for every match length 3 .. 258
//   dist                      -> "sym ebits eval" for every distance 1 .. 32768
//   order                     -> the 19 positions of the code-length code's lengths
//   codes n l0 .. l(n-1)      -> per symbol "bits length" of its table entry (stream bits, i.e. the code reversed)
//   rle n l0 .. l(n-1)        -> "count", then "symbol extra" per entry, then the 19 counts
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "deflate_codes.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "len") {
            for (unsigned l = 3; l <= 258; ++l) {
                int eb;
                unsigned ev;
                const unsigned s = dfl_len_symbol(l, &eb, &ev);
                std::printf("%u %d %u\n", s, eb, ev);
            }
        } else if (cmd == "dist") {
            for (unsigned d = 1; d <= 32768; ++d) {
                int eb;
                unsigned ev;
                const unsigned s = dfl_dist_symbol(d, &eb, &ev);
                std::printf("%u %d %u\n", s, eb, ev);
            }
        } else if (cmd == "order") {
            for (int k = 0; k < DFL_NCL; ++k) std::printf("%u\n", dfl_cl_order(k));
        } else if (cmd == "codes" || cmd == "rle") {
            int n = 0;
            in >> n;
            std::vector<unsigned char> len((size_t)n);          // exactly n: a read past the end is the sanitizer's to find
            for (int i = 0; i < n; ++i) {
                int v;
                in >> v;
                len[(size_t)i] = (unsigned char)v;
            }
            if (cmd == "codes") {
                for (int s = 0; s < n; ++s) {
                    const unsigned e = dfl_code_entry(len.data(), n, s);
                    std::printf("%u %u\n", e & 0xffffu, e >> 16);
                }
            } else {
                std::vector<unsigned short> out((size_t)n);
                unsigned hist[DFL_NCL] = {};
                const int k = dfl_rle_lengths(len.data(), n, out.data(), hist);
                std::printf("%d\n", k);
                for (int i = 0; i < k; ++i) std::printf("%u %u\n", out[(size_t)i] & 0xffu, out[(size_t)i] >> 8);
                for (int s = 0; s < DFL_NCL; ++s) std::printf("%u\n", hist[s]);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
