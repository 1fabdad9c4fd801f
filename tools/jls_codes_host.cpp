// The host-callable parts of csrc/jls_codes.h behind a line protocol, for tests/test_jls_codes_host_cpu.py (built there with the
// host compiler and its sanitizers).  Every buffer has exactly the size the kernels of jls.hip give it.  stdin, one request per line:
//   scan HEX                                     -> (nothing) the bytes of the current scan (no HEX: the empty scan)
//   defaults maxval near                         -> "T1 T2 T3"
//   derive maxval near t1 t2 t3 reset            -> "valid RANGE qbpp bpp LIMIT A0"
//   plain rows cols maxval near t1 t2 t3 reset   -> "status hash": the plain loop of k_jls_serial (jls_decode_plain)
//   wave rows cols maxval near t1 t2 t3 reset    -> "status hash": the rows as k_jls_wave strings them together: the pre words of
//                                                   a whole row first, the chain through them, run fills lane by lane, the row
//                                                   taken over only when it is complete
// hash: FNV-1a over the samples (little-endian uint16, zero where nothing was written).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "jls_codes.h"

static unsigned long long fnv(const std::vector<uint16_t>& v) {
    unsigned long long h = 1469598103934665603ull;
    for (uint16_t s : v) {
        h = (h ^ (s & 0xFFu)) * 1099511628211ull;
        h = (h ^ (s >> 8)) * 1099511628211ull;
    }
    return h;
}

// the row policy of k_jls_wave on plain arrays, its lanes one after the other
struct HostWaveRow {
    const uint32_t* pre;
    const uint16_t* prev;
    uint16_t* cur;
    int above(int x) const { return prev[x]; }
    uint32_t look(int x, int, int* Rb) const {
        *Rb = (int)(pre[x] & 0xFFFFu);
        return pre[x];
    }
    void put(int x, int v) { cur[x] = (uint16_t)v; }
    void fill(int x0, int x1, int v) {
        for (int lane = 0; lane < 64; ++lane)
            for (int i = x0 + lane; i < x1; i += 64) cur[i] = (uint16_t)v;
    }
};

static int decode_wave(const uint32_t* words, uint32_t len, const JlsParams& p, int rows, int cols, std::vector<uint16_t>& out) {
    std::vector<JlsCtx> ctx(JLS_CONTEXTS);
    for (int i = 0; i < JLS_CONTEXTS; ++i) ctx[i] = jls_ctx_init(p);
    std::vector<uint32_t> pre((size_t)cols);
    std::vector<uint16_t> a((size_t)cols, 0), c((size_t)cols, 0);
    uint16_t *prev = a.data(), *cur = c.data();
    JlsBits b = jls_bits_open<false>(words, len);
    int runindex = 0, corner = 0, bad = 0;
    for (int r = 0; r < rows; ++r) {
        const int Ra0 = prev[0];
        for (int x = 0; x < cols; ++x) {
            const int Rb = prev[x], Rc = x ? (int)prev[x - 1] : corner, Rd = x + 1 < cols ? (int)prev[x + 1] : Rb;
            pre[x] = jls_pre_word(Rb, Rc, Rd, p);
        }
        HostWaveRow row{pre.data(), prev, cur};
        bad = jls_row<false>(b, p, ctx.data(), row, cols, Ra0, corner, &runindex);
        corner = Ra0;
        if (bad) break;
        for (int x = 0; x < cols; ++x) out[(size_t)r * cols + x] = cur[x];
        uint16_t* t = prev;
        prev = cur;
        cur = t;
    }
    return jls_status(b, bad);
}

int main() {
    std::string line;
    std::vector<uint32_t> words;
    uint32_t len = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "scan") {
            std::string hex;
            in >> hex;
            len = (uint32_t)(hex.size() / 2);
            words.assign((len + 3) / 4, 0u);                           // the kernels' guarantee: whole words, nothing behind them
            words.shrink_to_fit();
            for (uint32_t i = 0; i < len; ++i)
                words[i >> 2] |= (uint32_t)std::stoi(hex.substr(2 * (size_t)i, 2), nullptr, 16) << (8 * (i & 3));
            continue;
        }
        if (cmd == "defaults") {
            int maxval = 0, near_ = 0, t1 = 0, t2 = 0, t3 = 0;
            in >> maxval >> near_;
            jls_default_thresholds(maxval, near_, &t1, &t2, &t3);
            std::printf("%d %d %d\n", t1, t2, t3);
            continue;
        }
        int rows = 1, cols = 1, v[6] = {0, 0, 0, 0, 0, 0};
        if (cmd != "derive") in >> rows >> cols;
        for (int& x : v) in >> x;
        const bool valid = jls_params_valid(v[0], v[1], v[2], v[3], v[4], v[5]);
        if (cmd == "derive") {
            if (!valid) {
                std::printf("0 0 0 0 0 0\n");
                continue;
            }
            const JlsParams p = jls_derive(v[0], v[1], v[2], v[3], v[4], v[5]);
            std::printf("1 %d %d %d %d %d\n", p.range, p.qbpp, p.bpp, p.limit, p.a0);
            continue;
        }
        if (!valid || rows < 1 || cols < 1) return 2;
        const JlsParams p = jls_derive(v[0], v[1], v[2], v[3], v[4], v[5]);
        std::vector<uint16_t> out((size_t)rows * cols, 0);
        int st;
        if (cmd == "plain") {
            std::vector<JlsCtx> ctx(JLS_CONTEXTS);
            st = jls_decode_plain(words.data(), len, p, rows, cols, out.data(), ctx.data());
        } else if (cmd == "wave") {
            st = decode_wave(words.data(), len, p, rows, cols, out);
        } else {
            return 2;
        }
        std::printf("%d %llu\n", st, fnv(out));
    }
    return 0;
}
