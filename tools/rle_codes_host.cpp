// The host-callable parts of csrc/rle_codes.h behind a line protocol, for tests/test_rle_codes_host_cpu.py (built there with the
// host compiler and its sanitizers).  Every buffer has exactly the size the kernels of rle.hip give it.  stdin, one request per line:
//   seg HEX                   -> (nothing) the bytes of the current segment (no HEX: the empty segment)
//   map chunk_bytes           -> per chunk one line: the 129 table words of its entry map
//   chain chunk_bytes wanted  -> "total chunks", then the entry offset of every chunk (-1: not live), then the output bases
//   runs chunk_bytes wanted   -> per live chunk one line: its index, then position and output offset of every run
//   expand chunk_bytes wanted -> "status bytes hash": map, chain, then every live chunk's runs and the lookup of the run of every
//                                output byte, as the kernels string them together (hash: FNV-1a over the `wanted` output bytes)
//   serial wanted             -> "status bytes hash" of the plain loop
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rle_codes.h"

static unsigned long long fnv(const std::vector<uint8_t>& v) {
    unsigned long long h = 1469598103934665603ull;
    for (uint8_t b : v) h = (h ^ b) * 1099511628211ull;
    return h;
}

struct Chain {
    std::vector<uint32_t> table, entry, base;
    uint32_t n_chunks = 0;
    uint64_t total = 0;
};

static Chain chain_of(const std::vector<uint8_t>& s, uint32_t cb, uint32_t wanted) {
    Chain c;
    c.n_chunks = (uint32_t)((s.size() + cb - 1) / cb);
    c.table.assign((size_t)c.n_chunks * RLE_ENTRIES, 0);
    c.entry.assign(c.n_chunks, 0);
    c.base.assign(c.n_chunks, 0);
    std::vector<uint32_t> a(rle_nodes(cb)), b(rle_nodes(cb));
    for (uint32_t k = 0; k < c.n_chunks; ++k)
        rle_entry_map(s.data(), (uint32_t)s.size(), k, cb, a.data(), b.data(), c.table.data() + (size_t)k * RLE_ENTRIES);
    c.total = rle_chain(c.table.data(), c.n_chunks, wanted, c.entry.data(), c.base.data());
    return c;
}

// the run list of chunk k entered at e, as k_rle_expand builds it; *staged: the chunk's bytes as the kernel holds them
static std::vector<uint32_t> runs_of(const std::vector<uint8_t>& s, uint32_t cb, uint32_t k, uint32_t e, std::vector<uint8_t>* staged,
                                     uint32_t* produced) {
    const uint32_t n = rle_nodes(cb), start = k * cb, rest = (uint32_t)s.size() - start;
    const uint32_t len = rest < cb ? rest : cb, avail = rest < cb + RLE_MAX_STEP - 1u ? rest : cb + RLE_MAX_STEP - 1u;
    staged->assign(s.begin() + start, s.begin() + start + avail);
    staged->shrink_to_fit();
    std::vector<uint32_t> a(n), b(n), mark(n, RLE_NOT_LIVE);
    for (uint32_t i = 0; i < n; ++i) a[i] = rle_node(staged->data(), rest, len, n - 1u, i);
    mark[e] = 0;
    for (int r = rle_rounds(cb); r > 0; --r) {
        rle_mark_round(a.data(), mark.data(), n, 0u, 1u);
        rle_double_round(a.data(), b.data(), n, 0u, 1u);
        a.swap(b);
    }
    *produced = rle_count(a[e]);
    std::vector<uint32_t> runs;
    for (uint32_t p = 0; p < cb; ++p) {
        const uint32_t w = rle_run_at(staged->data(), rest, len, n - 1u, mark.data(), p);
        if (w != RLE_NOT_LIVE) runs.push_back(w);
    }
    return runs;
}

int main() {
    std::string line;
    std::vector<uint8_t> s;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "seg") {
            std::string hex;
            in >> hex;
            s.assign(hex.size() / 2, 0);
            for (size_t i = 0; i < s.size(); ++i) s[i] = (uint8_t)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
            s.shrink_to_fit();
            continue;
        }
        if (cmd == "serial") {
            uint32_t wanted = 0;
            in >> wanted;
            std::vector<uint8_t> out(wanted, 0);
            const uint32_t n = rle_decode_serial(s.data(), (uint32_t)s.size(), out.data(), wanted);
            std::printf("%d %u %llu\n", n < wanted ? 1 : 0, n, fnv(out));
            continue;
        }
        uint32_t cb = 0, wanted = 0;
        in >> cb;
        if (cb < RLE_CHUNK_MIN || cb > RLE_CHUNK_MAX || (cb & (cb - 1u))) return 2;
        if (cmd != "map") in >> wanted;
        const Chain c = chain_of(s, cb, cmd == "map" ? 0u : wanted);
        if (cmd == "map") {
            for (uint32_t k = 0; k < c.n_chunks; ++k) {
                for (uint32_t e = 0; e < RLE_ENTRIES; ++e) std::printf("%u ", c.table[(size_t)k * RLE_ENTRIES + e]);
                std::printf("\n");
            }
        } else if (cmd == "chain") {
            std::printf("%llu %u\n", (unsigned long long)c.total, c.n_chunks);
            for (uint32_t k = 0; k < c.n_chunks; ++k) std::printf("%lld ", c.entry[k] == RLE_NOT_LIVE ? -1ll : (long long)c.entry[k]);
            std::printf("\n");
            for (uint32_t k = 0; k < c.n_chunks; ++k) std::printf("%u ", c.base[k]);
            std::printf("\n");
        } else if (cmd == "runs" || cmd == "expand") {
            std::vector<uint8_t> out(wanted, 0), staged;
            for (uint32_t k = 0; k < c.n_chunks; ++k) {
                if (c.entry[k] == RLE_NOT_LIVE) continue;
                uint32_t produced = 0;
                const std::vector<uint32_t> runs = runs_of(s, cb, k, c.entry[k], &staged, &produced);
                if (cmd == "runs") {
                    std::printf("%u ", k);
                    for (uint32_t w : runs) std::printf("%u %u ", rle_pos(w), rle_count(w));
                    std::printf("\n");
                    continue;
                }
                const uint32_t room = wanted - c.base[k], n_out = runs.empty() ? 0u : (produced < room ? produced : room);
                for (uint32_t o = 0; o < n_out; ++o)
                    out[c.base[k] + o] = rle_run_byte(staged.data(), rle_find_run(runs.data(), (uint32_t)runs.size(), o), o);
            }
            if (cmd == "expand")
                std::printf("%d %llu %llu\n", c.total < wanted ? 1 : 0, (unsigned long long)(c.total < wanted ? c.total : wanted),
                            fnv(out));
        } else {
            return 2;
        }
    }
    return 0;
}
