// csrc/tile_grid.h behind a line protocol, for tests/test_tile_grid_host_cpu.py (built there with the host compiler and its
// sanitizers).  stdin, one request per line; every array lives in a heap buffer of exactly its size:
//   origins x y z x y z ..     -> (nothing) the tile origins of the requests that follow
//   grid                       -> "ok n0 n1 n2", then the steps of the three axes, one line per axis (grid_origins)
//   steps a v0 v1 ..           -> (nothing) the tile origins along axis a, for `walk`
//   walk e0 e1 e2 PV0 PV1 PV2  -> "walk_table_ints length", then the table on one line (tiles of extent e in a padded volume PV)
//   defer patch0 d0 d1 ..      -> "consistent x0 x_split x_end dp0 n_def", then the deferring rows (defer_plan on the origins)
//   offsets act n F ss16 ints  -> "ss ss16 ssp tab bytes" (stash_offsets)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tile_grid.h"

static std::vector<int> rest(std::istringstream& in) {
    std::vector<int> v;
    int x;
    while (in >> x) v.push_back(x);
    v.shrink_to_fit();
    return v;
}

static void print(const std::vector<int>& v) {
    for (int x : v) std::printf("%d ", x);
    std::printf("\n");
}

int main() {
    std::string line;
    std::vector<int> origins, steps[3];
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "origins") {
            origins = rest(in);
            if (origins.size() % 3) return 2;
        } else if (cmd == "grid") {
            std::vector<int> s[3];
            const bool ok = grid_origins(origins.data(), (int)(origins.size() / 3), s);
            std::printf("%d %zu %zu %zu\n", ok ? 1 : 0, s[0].size(), s[1].size(), s[2].size());
            for (int a = 0; a < 3; ++a) print(s[a]);
        } else if (cmd == "steps") {
            int a = -1;
            in >> a;
            if (a < 0 || a > 2) return 2;
            steps[a] = rest(in);
        } else if (cmd == "walk") {
            const std::vector<int> v = rest(in);
            if (v.size() != 6) return 2;
            const std::vector<int> tab = walk_table(steps[0], steps[1], steps[2], v.data(), v.data() + 3);
            std::printf("%zu %zu\n", walk_table_ints((int)steps[0].size(), (int)steps[1].size(), (int)steps[2].size(), v.data() + 3), tab.size());
            print(tab);
        } else if (cmd == "defer") {
            int patch0 = 0;
            in >> patch0;
            const std::vector<int> defer = rest(in);
            if (defer.size() * 3 != origins.size()) return 2;
            const DeferPlan p = defer_plan(origins.data(), defer.data(), (int)defer.size(), patch0);
            std::printf("%d %d %d %d %d %d\n", p.consistent ? 1 : 0, p.x0, p.x_split, p.x_end, p.dp0, p.n_def);
            print(p.def_rows);
        } else if (cmd == "offsets") {
            size_t act = 0, ints = 0;
            int n = 0, F = 0, ss16 = 0;
            in >> act >> n >> F >> ss16 >> ints;
            const StashOffsets o = stash_offsets(act, n, F, ss16 != 0, ints);
            std::printf("%zu %zu %zu %zu %zu\n", o.ss, o.ss16, o.ssp, o.tab, o.bytes);
        } else {
            return 2;
        }
    }
    return 0;
}
