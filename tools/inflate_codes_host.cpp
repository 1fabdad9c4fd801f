// The host-callable parts of csrc/inflate_codes.h behind a line protocol, for tests/test_inflate_codes_host_cpu.py (built there
// with the host compiler and its sanitizers).  stdin, one request per line:
//   stream HEX                -> (nothing) the bytes of the current stream, held in a buffer of exactly that size
//   start b0 b1 ..            -> "0" / "1" per bit offset: the block-start test
//   header bit                -> "status"; for status 0 then four lines: the 16 counts and the symbols in canonical order of the
//                                literal/length code, the same of the distance code (the header's three block bits start at `bit`)
//   chunk start stop          -> "status end final bytes hash" of the count pass, then the same of the store pass (hash: FNV-1a over
//                                the 16-bit symbols)
//   pipeline chunk_bytes      -> "status chunks candidates rejected rounds live bytes crc32": find, count, walk and repair, store,
//                                windows and resolve as the kernels of inflate.hip do them, on the host
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "inflate_codes.h"

static unsigned long long fnv(const std::vector<uint16_t>& v, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ v[i]) * 1099511628211ull;
    return h;
}

static unsigned crc32_of(const std::vector<uint8_t>& v) {
    unsigned c = 0xffffffffu;
    for (uint8_t b : v) {
        c ^= b;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? DFL_CRC_POLY : 0u);
    }
    return c ^ 0xffffffffu;
}

static void pipeline(const std::vector<uint8_t>& s, size_t chunk_bytes) {
    const size_t n = (s.size() + chunk_bytes - 1) / chunk_bytes;
    std::vector<InfChunk> ch(n);
    InfTables T;
    unsigned candidates = 0, rejected = 0, rounds = 0;
    for (size_t k = 0; k < n; ++k) {
        ch[k] = InfChunk{};
        ch[k].src_len = s.size();
        ch[k].nominal = 8ull * k * chunk_bytes;
        ch[k].search_end = std::min<uint64_t>(ch[k].nominal + 8ull * chunk_bytes, 8ull * s.size());
        if (k == 0) {
            ch[k].flags = INF_F_LIVE | INF_F_REDO;
            continue;
        }
        for (uint64_t bit = ch[k].nominal; bit < ch[k].search_end; ++bit)
            if (inf_block_start(s.data(), s.size(), bit)) {
                ch[k].start = bit;
                ch[k].flags = INF_F_LIVE | INF_F_REDO | INF_F_CAND;
                ++candidates;
                break;
            }
    }
    uint64_t stop = INF_NO_STOP;
    for (size_t k = n; k-- > 0;)
        if (ch[k].flags & INF_F_LIVE) {
            ch[k].stop = stop;
            stop = ch[k].start;
        }
    int status = INF_OK;
    for (;;) {
        for (auto& c : ch)
            if ((c.flags & INF_F_LIVE) && (c.flags & INF_F_REDO)) {
                InfCount sink;
                int final = 0;
                c.status = (uint32_t)inf_decode_chunk(s.data(), s.size(), c.start, c.stop, &T, sink, &c.end, &final);
                c.nbytes = sink.n;
                c.final = (uint32_t)final;
                c.flags &= ~INF_F_REDO;
            }
        const InfWalk w = inf_walk(ch.data(), 0, (unsigned)n);
        rejected += w.rejected;
        status = w.status;
        if (status != INF_OK || !w.redo) break;
        if (++rounds > 8) {
            status = INF_REPAIR;
            break;
        }
    }
    std::vector<uint8_t> out;
    unsigned live = 0;
    if (status == INF_OK) {
        std::vector<uint8_t> window;                           // of the chunk before
        for (auto& c : ch) {
            if (!(c.flags & INF_F_LIVE)) continue;
            ++live;
            std::vector<uint16_t> sym((size_t)c.nbytes);      // exactly the counted length
            InfStore sink{sym.data(), c.nbytes};
            uint64_t end = 0;
            int final = 0;
            const int st = inf_decode_chunk(s.data(), s.size(), c.start, c.stop, &T, sink, &end, &final);
            if (st != INF_OK || sink.n != c.nbytes || end != c.end) {
                status = st ? st : INF_OVERRUN;
                break;
            }
            const size_t rel = out.size();
            for (uint16_t v : sym) {
                if (v & 0x8000u) {
                    const unsigned k = v & 0x7fffu;
                    if (rel + k < INF_WINDOW) {
                        status = INF_FAR;
                        break;
                    }
                    out.push_back(window[k]);
                } else
                    out.push_back((uint8_t)v);
            }
            if (status != INF_OK) break;
            window.assign(INF_WINDOW, 0);                      // the 32 KiB that end with this chunk's last byte
            for (size_t k = 0; k < INF_WINDOW; ++k)
                if (out.size() + k >= INF_WINDOW) window[k] = out[out.size() + k - INF_WINDOW];
        }
    }
    std::printf("%d %zu %u %u %u %u %zu %u\n", status, n, candidates, rejected, rounds, live, out.size(), crc32_of(out));
}

int main() {
    std::string line;
    std::vector<uint8_t> s;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "stream") {
            std::string hex;
            in >> hex;
            s.assign(hex.size() / 2, 0);
            for (size_t i = 0; i < s.size(); ++i) s[i] = (uint8_t)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
            s.shrink_to_fit();
        } else if (cmd == "start") {
            unsigned long long bit;
            while (in >> bit) std::printf("%d\n", inf_block_start(s.data(), s.size(), bit) ? 1 : 0);
        } else if (cmd == "header") {
            unsigned long long bit = 0;
            in >> bit;
            InfBits b;
            InfTables T = {};
            inf_bits_init(&b, s.data(), s.size(), bit);
            inf_get(&b, 3);
            const int st = inf_dynamic_header(&b, 8ull * s.size(), &T);
            std::printf("%d\n", st);
            if (st == INF_OK) {
                for (int pass = 0; pass < 2; ++pass) {
                    const uint16_t* count = pass ? T.dcount : T.lcount;
                    const uint16_t* symbol = pass ? T.dsym : T.lsym;
                    int used = 0;
                    for (int l = 0; l < 16; ++l) {
                        std::printf("%u ", count[l]);
                        if (l) used += count[l];
                    }
                    std::printf("\n");
                    for (int k = 0; k < used; ++k) std::printf("%u ", symbol[k]);
                    std::printf("\n");
                }
            }
        } else if (cmd == "chunk") {
            unsigned long long start = 0, stop = 0;
            in >> start >> stop;
            InfTables T;
            InfCount count;
            uint64_t end = 0;
            int final = 0;
            int st = inf_decode_chunk(s.data(), s.size(), start, stop, &T, count, &end, &final);
            std::printf("%d %llu %d %llu 0\n", st, (unsigned long long)end, final, (unsigned long long)count.n);
            std::vector<uint16_t> sym((size_t)count.n);
            InfStore store{sym.data(), count.n};
            st = inf_decode_chunk(s.data(), s.size(), start, stop, &T, store, &end, &final);
            std::printf("%d %llu %d %llu %llu\n", st, (unsigned long long)end, final, (unsigned long long)store.n, fnv(sym, (size_t)store.n));
        } else if (cmd == "pipeline") {
            size_t chunk_bytes = 0;
            in >> chunk_bytes;
            if (chunk_bytes < 64) return 2;
            pipeline(s, chunk_bytes);
        } else {
            return 2;
        }
    }
    return 0;
}
