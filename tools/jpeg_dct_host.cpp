// The host-callable parts of csrc/jpeg_dct_codes.h (and csrc/jpeg_huff.h under it) behind a line protocol, for
// tests/test_jpeg_dct_codes_host_cpu.py (built there with the host compiler and its sanitizers).  The stream buffer has exactly
// the size the kernels of jpeg_dct.hip are given: whole words, nothing behind them.  stdin, one request per line:
//   tab dc|ac HEX            -> (nothing) an expanded Huffman table (BOA_LJ_TABLE_WORDS little-endian words)
//   qt HEX                   -> (nothing) a quantisation table, 64 little-endian uint16 in natural order
//   seg HEX                  -> (nothing) the un-stuffed bytes of the current restart interval (no HEX: empty)
//   step pos k P             -> "status len knext zz val": one codeword at bit `pos` (jd_step)
//   serial P blocks          -> "status hash": the loop of k_jd_serial over the interval, DC prediction included
//   parallel P blocks sub    -> "status hash": the phases A-E of k_jd_parallel with subsequences of `sub` bytes, thread by thread
//   pixels P rows cols       -> "status hash": `serial`, then jd_block and the crop of k_jd_idct
//   block P c0 .. c63        -> 64 samples: jd_block of these coefficients (natural order)
// hash: FNV-1a over the values as little-endian uint16.  Requests outside the admitted ranges end the program with status 2.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "jpeg_dct_codes.h"

static const int TW = 384;

static unsigned long long fnv(const uint16_t* v, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) {
        h = (h ^ (v[i] & 0xFFu)) * 1099511628211ull;
        h = (h ^ (v[i] >> 8)) * 1099511628211ull;
    }
    return h;
}

static std::vector<unsigned char> unhex(const std::string& hex) {
    std::vector<unsigned char> out(hex.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (unsigned char)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
    return out;
}

struct State {
    std::vector<uint32_t> dc, ac, words;
    std::vector<uint16_t> q;
    unsigned len = 0;
    const unsigned char* bytes() const { return (const unsigned char*)words.data(); }
};

static int serial(const State& s, int P, int blocks, std::vector<short>& cf) {
    const unsigned seg_bits = 8u * s.len;
    BitReader br(s.bytes(), s.len);
    unsigned pos = 0;
    int pred = 0, err = 0;
    for (int b = 0; b < blocks && !err; ++b) {
        int k = 0;
        do {
            JdStep st;
            err = pos >= seg_bits ? JD_ST_TRUNCATED : jd_step(s.dc.data(), s.ac.data(), br.peek(pos), k, P, seg_bits - pos, st);
            if (err) break;
            if (k == 0) {
                pred += st.val;
                cf[(size_t)b * 64] = (short)pred;
            } else if (st.zz >= 0 && st.val) {
                cf[(size_t)b * 64 + jd_natural(st.zz)] = (short)st.val;
            }
            pos += (unsigned)st.len;
            k = st.knext;
        } while (k);
    }
    if (!err && seg_bits - pos >= 8u) err = JD_ST_TRAILING;
    return err;
}

static const unsigned long long BAD = ~0ull;

static unsigned run(const State& s, unsigned long long& state, unsigned stop, int P) {
    const unsigned seg_bits = 8u * s.len;
    BitReader br(s.bytes(), s.len);
    unsigned pos = (unsigned)(state >> 6), n = 0;
    int k = (int)(state & 63u);
    while (pos < stop) {
        JdStep st;
        if (jd_step(s.dc.data(), s.ac.data(), br.peek(pos), k, P, seg_bits - pos, st)) {
            state = BAD;
            return n;
        }
        pos += (unsigned)st.len;
        k = st.knext;
        n += k == 0;
    }
    state = ((unsigned long long)pos << 6) | (unsigned)k;
    return n;
}

static int parallel(const State& s, int P, int blocks, int sub, std::vector<short>& cf) {
    const unsigned seg_bits = 8u * s.len;
    const int ns = std::max(1, (int)((s.len + sub - 1) / sub));
    std::vector<unsigned long long> ex(ns), su(ns);
    std::vector<unsigned> cnt(ns), fs(ns), nbad(ns);
    auto stop_of = [&](int i) { return i + 1 < ns ? 8u * (unsigned)((i + 1) * sub) : seg_bits; };
    for (int i = 0; i < ns; ++i) {
        unsigned long long st = ((unsigned long long)(8u * (unsigned)(i * sub))) << 6;
        su[i] = st;
        cnt[i] = run(s, st, stop_of(i), P);
        ex[i] = st;
    }
    for (int it = 0; it <= ns; ++it) {                                  // Jacobi sweeps, one subsequence per thread
        std::vector<unsigned long long> nx(ex);
        bool changed = false;
        for (int i = 1; i < ns; ++i) {
            const unsigned long long p = ex[i - 1];
            if (p != su[i] && p != BAD) {
                su[i] = p;
                unsigned long long e = p;
                cnt[i] = run(s, e, stop_of(i), P);
                nx[i] = e;
                changed = true;
            }
        }
        ex = nx;
        if (!changed) break;
        if (it == ns) return JD_ST_INVALID_CODE;
    }
    unsigned a = 0, b = 0;
    for (int i = 0; i < ns; ++i) {
        fs[i] = a;
        nbad[i] = b;
        a += cnt[i];
        b += ex[i] == BAD;
    }
    int status = 0;
    const unsigned n = (unsigned)blocks;
    for (int i = 0; i < ns; ++i) {
        const unsigned j0 = fs[i];
        if (j0 >= n || nbad[i]) continue;
        const unsigned stop = stop_of(i);
        BitReader br(s.bytes(), s.len);
        unsigned pos = (unsigned)(su[i] >> 6), j = j0;
        int k = (int)(su[i] & 63u), err = 0;
        while (pos < stop && j < n) {
            JdStep st;
            err = jd_step(s.dc.data(), s.ac.data(), br.peek(pos), k, P, seg_bits - pos, st);
            if (err) break;
            if (st.zz >= 0 && st.val) cf[(size_t)j * 64 + jd_natural(st.zz)] = (short)st.val;
            pos += (unsigned)st.len;
            k = st.knext;
            j += k == 0;
        }
        if (!err) {
            if (j == n && seg_bits - pos >= 8u) err = JD_ST_TRAILING;
            else if (j < n && stop == seg_bits) err = JD_ST_TRUNCATED;
        }
        if (err && !status) status = err;
    }
    unsigned dcv = 0;
    for (int bk = 0; bk < blocks; ++bk) {
        dcv += (unsigned)(unsigned short)cf[(size_t)bk * 64];
        cf[(size_t)bk * 64] = (short)(unsigned short)dcv;
    }
    return status;
}

int main() {
    State s;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, arg;
        in >> cmd;
        if (cmd == "tab") {
            std::string which;
            in >> which >> arg;
            const std::vector<unsigned char> b = unhex(arg);
            if (b.size() != (size_t)TW * 4 || (which != "dc" && which != "ac")) return 2;
            std::vector<uint32_t>& T = which == "dc" ? s.dc : s.ac;
            T.assign(TW, 0u);
            for (size_t i = 0; i < b.size(); ++i) T[i >> 2] |= (uint32_t)b[i] << (8 * (i & 3));
            for (int li = 0; li < (1 << JH_LB); ++li) {                 // what boa_jdct_decode checks of a table
                const unsigned e = (T[li >> 1] >> ((li & 1) * 16)) & 0xffffu;
                if (e && (e >> 8 < 1 || e >> 8 > JH_LB)) return 2;
            }
            continue;
        }
        if (cmd == "qt") {
            in >> arg;
            const std::vector<unsigned char> b = unhex(arg);
            if (b.size() != 128) return 2;
            s.q.assign(64, 0);
            for (int i = 0; i < 64; ++i) s.q[i] = (uint16_t)(b[2 * i] | (b[2 * i + 1] << 8));
            continue;
        }
        if (cmd == "seg") {
            in >> arg;
            const std::vector<unsigned char> b = unhex(arg);
            s.len = (unsigned)b.size();
            s.words.assign((s.len + 3) / 4, 0u);
            s.words.shrink_to_fit();
            for (unsigned i = 0; i < s.len; ++i) s.words[i >> 2] |= (uint32_t)b[i] << (8 * (i & 3));
            continue;
        }
        if (s.dc.empty() || s.ac.empty()) return 2;
        if (cmd == "block") {
            int P = 0;
            in >> P;
            short c[64];
            uint16_t px[64];
            for (short& v : c) {
                int x = 0;
                in >> x;
                if (x < -32768 || x > 32767) return 2;
                v = (short)x;
            }
            if ((P != 8 && P != 12) || s.q.size() != 64 || !in) return 2;
            jd_block(c, s.q.data(), P, px);
            for (int i = 0; i < 64; ++i) std::printf("%d%c", px[i], i == 63 ? '\n' : ' ');
            continue;
        }
        if (cmd == "step") {
            long long pos = -1;
            int k = -1, P = 0;
            in >> pos >> k >> P;
            if (pos < 0 || pos >= 8ll * s.len || k < 0 || k > 63 || (P != 8 && P != 12)) return 2;
            BitReader br(s.bytes(), s.len);
            JdStep st{0, 0, 0, 0};
            const int err = jd_step(s.dc.data(), s.ac.data(), br.peek((unsigned)pos), k, P, 8u * s.len - (unsigned)pos, st);
            std::printf("%d %d %d %d %d\n", err, st.len, st.knext, st.zz, st.val);
            continue;
        }
        int P = 0, a = 0, b = 0;
        in >> P >> a >> b;
        if (P != 8 && P != 12) return 2;
        if (cmd == "serial" || cmd == "parallel") {
            if (a < 1 || a > (1 << 20) || (cmd == "parallel" && (b < 4 || b > (1 << 20)))) return 2;
            std::vector<short> cf((size_t)a * 64, 0);
            const int st = cmd == "serial" ? serial(s, P, a, cf) : parallel(s, P, a, b, cf);
            std::printf("%d %llu\n", st, fnv((const uint16_t*)cf.data(), cf.size()));
        } else if (cmd == "pixels") {
            if (a < 1 || a > 4096 || b < 1 || b > 4096 || s.q.size() != 64) return 2;
            const int bw = (b + 7) / 8, nb = bw * ((a + 7) / 8);
            std::vector<short> cf((size_t)nb * 64, 0);
            const int st = serial(s, P, nb, cf);
            std::vector<uint16_t> out((size_t)a * b, 0);
            for (int k = 0; k < nb; ++k) {
                uint16_t px[64];
                jd_block(cf.data() + (size_t)k * 64, s.q.data(), P, px);
                const int y0 = (k / bw) * 8, x0 = (k % bw) * 8;
                for (int y = 0; y < 8 && y0 + y < a; ++y)
                    for (int x = 0; x < 8 && x0 + x < b; ++x) out[(size_t)(y0 + y) * b + x0 + x] = px[8 * y + x];
            }
            std::printf("%d %llu\n", st, fnv(out.data(), out.size()));
        } else {
            return 2;
        }
    }
    return 0;
}
