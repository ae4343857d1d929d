// CPU test of csrc/gemm_tile_walk.h (tests/test_gemm_tile_walk_cpu.py builds this with g++ -fsanitize=undefined and runs it): the header
// alone, compiled as host code.  Sweeps tiles_m 1..MAX_M, tiles_n 1..MAX_N, group_n 1..tiles_n, rev 0/1 and writes, for every block id
// of every grid in that order, the pair (tm, tn) as two int32 to stdout.  The program itself fails (exit 1) on a pair outside the grid
// or a tile taken twice; the Python side checks the same again and the order against the expression the kernels used to carry.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemm_tile_walk.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const int max_m = atoi(argv[1]), max_n = atoi(argv[2]);
    std::vector<int32_t> out;
    std::vector<char> seen;
    for (int tiles_m = 1; tiles_m <= max_m; ++tiles_m)
        for (int tiles_n = 1; tiles_n <= max_n; ++tiles_n)
            for (int group_n = 1; group_n <= tiles_n; ++group_n)
                for (int rev = 0; rev < 2; ++rev) {
                    const int tiles = tiles_m * tiles_n;
                    seen.assign(tiles, 0);
                    out.clear();
                    for (int bid = 0; bid < tiles; ++bid) {
                        const TileIndex t = tile_walk(bid, tiles_m, tiles_n, group_n, rev);
                        if (t.tm < 0 || t.tm >= tiles_m || t.tn < 0 || t.tn >= tiles_n || seen[t.tm * tiles_n + t.tn]++) {
                            fprintf(stderr, "tiles_m %d tiles_n %d group_n %d rev %d: block %d -> (%d, %d) is outside the grid or taken twice\n",
                                    tiles_m, tiles_n, group_n, rev, bid, t.tm, t.tn);
                            return 1;
                        }
                        out.push_back(t.tm);
                        out.push_back(t.tn);
                    }
                    if (fwrite(out.data(), sizeof(int32_t), out.size(), stdout) != out.size()) return 3;
                }
    return 0;
}
