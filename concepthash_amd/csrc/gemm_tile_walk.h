// The order in which the workgroups of a bf16 GEMM launch take the output tiles: block id -> (m-tile, n-tile).  Plain C++ (no HIP
// header), so that the host can compile it too: tests/test_gemm_tile_walk_cpu.py proves the map a bijection over a sweep of grids.
#pragma once

#if defined(__HIPCC__)
#define CH_TILE_FN __host__ __device__ __forceinline__
#else
#define CH_TILE_FN inline
#endif

// XCD-aware, bijective block remap: blocks b and b+8 share an XCD (observed round-robin dispatch; speed only), so XCD x gets the
// contiguous chunk of ceil or floor(nwg / 8) remapped ids that starts where XCD x-1's chunk ends.
CH_TILE_FN int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, local = bid >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + local;
}

struct TileIndex {
    int tm, tn;
};
// Tile order inside an XCD's contiguous chunk: n-tiles are taken in groups of group_n (the last group may be partial) whose weight
// panels stay L2-resident (<= ~2.0 MB) while the m-tiles sweep past; inside a group n is fastest, so the co-resident workgroups of
// an XCD share activation panels too.  rev walks the m-tiles from the last row tile to the first (serpentine launch order).
// 1 <= group_n <= tiles_n (host: ch_gemm_group_n).
CH_TILE_FN TileIndex tile_walk(int bid, int tiles_m, int tiles_n, int group_n, int rev) {
    const int wg = xcd_remap(bid, tiles_m * tiles_n);
    const int per_group = tiles_m * group_n;
    const int g = wg / per_group, rem = wg - g * per_group;
    const int left = tiles_n - g * group_n, gn = group_n < left ? group_n : left;
    const int tm_fwd = rem / gn, tn = g * group_n + (rem - tm_fwd * gn);
    return {rev ? tiles_m - 1 - tm_fwd : tm_fwd, tn};
}
