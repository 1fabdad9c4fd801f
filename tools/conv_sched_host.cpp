// csrc/conv_sched.h behind a line protocol, for tests/test_conv_sched_host_cpu.py (built there with the host compiler and its
// sanitizers).  stdin, one request per line:
//   layer T cu cy_fast t0 t1 t2 ncy e0 e1 e2 nmax
// a layer of T = t0 t1 t2 ncy tiles per sample (tile extent e) on cu compute units.  stdout, all integers: "vw nslots", the run table
// (conv_sched_runs, vw x 8) on one line, then for every batch N = 1 .. nmax one line "grid row" followed by the tile count of each of
// the grid workgroups (conv_sched_grid, conv_sched_desc_row, conv_sched_wg_tiles).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "conv_sched.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        int T = 0, cu = 0, nmax = 0;
        ConvSchedGeom g = {};
        in >> cmd >> T >> cu >> g.cy_fast >> g.t[0] >> g.t[1] >> g.t[2] >> g.ncy >> g.ext[0] >> g.ext[1] >> g.ext[2] >> nmax;
        if (cmd != "layer" || !in || T < 1 || cu < 1 || (long long)g.t[0] * g.t[1] * g.t[2] * g.ncy != T) return 2;
        const int vw = conv_ws_vw(T, cu);
        std::vector<int> runs = conv_sched_runs(g, T, vw);
        runs.shrink_to_fit();
        std::printf("%d %d\n", vw, conv_ws_nslots(T, cu));
        for (int x : runs) std::printf("%d ", x);
        std::printf("\n");
        for (int N = 1; N <= nmax; ++N) {
            const int grid = conv_sched_grid(vw, N, cu);
            std::printf("%d %d", grid, conv_sched_desc_row(N, vw, grid, T));
            for (int b = 0; b < grid; ++b) std::printf(" %lld", conv_sched_wg_tiles(runs, vw, N, grid, b));
            std::printf("\n");
        }
    }
    return 0;
}
