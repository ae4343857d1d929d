// Device-side pieces the bf16 GEMM kernels share: the LDS-DMA address spaces, the block's tile origin, the accumulator reset.
// Only text that is the same in two or more kernels AND leaves their registers and non-integer instructions as they were lives
// here (profiles/gemm_tile_registers.txt has the comparison, and what stayed written out in the kernels with its cost).
#pragma once
#include "ch_common.h"
#include "kernels.h"
#include "gemm_tile_walk.h"

typedef __attribute__((address_space(3))) void lds_void_t;         // __builtin_amdgcn_global_load_lds destination
typedef __attribute__((address_space(1))) const void gbl_void_t;   // ... and source

struct TileOrigin {
    int m0, n0;
};
// first row / column of the BM x BN output tile that block `bid` of the launch computes (gemm_tile_walk.h has the order)
template <int BM, int BN>
__device__ __forceinline__ TileOrigin tile_origin(const GemmParams &p, int bid) {
    const TileIndex t = tile_walk(bid, (p.M + BM - 1) / BM, p.N / BN, p.group_n, p.rev);
    return {t.tm * BM, t.tn * BN};
}

template <int NT, int MT>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NT][MT]) {
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
}
