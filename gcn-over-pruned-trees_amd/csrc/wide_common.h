// The core the two wide forms of the layer kernel share (wide_kernels.hip: forward; wide_bwd_kernels.hip: backward-data): the weight-block
// MFMA loop, the epilogue and row stores of a WIDE_COLS block, and one LDS layout for kernels and launchers, so that the k order, and
// with it the bit-identity to the row tile, holds by construction.  Each kernel still writes its chunk gather itself: the gather as a
// shared function cost the bf16 backward instantiations two SGPRs.  Two translation units all the same, so that neither form's
// instantiations change the code the compiler emits for the other's.
#pragma once
#include "rowtile_body.h"

namespace gcnpt {

constexpr int WIDE_THREADS = 256;                       // 4 waves
constexpr int WIDE_WAVES = WIDE_THREADS / WAVE;
constexpr int WIDE_KCHUNK = 256;                        // columns of S per chunk, a multiple of both k-steps: 33 KB of fp32 tile in LDS
constexpr int WIDE_NTW = 2;                             // transform / backward: output column tiles per wave
constexpr int WIDE_COLS = WIDE_WAVES * WIDE_NTW * 16;   // transform / backward: output columns per workgroup
constexpr int WIDE_KB = 8;                              // transform / backward: k-steps of weight fragments per register block (two in flight)

// The LDS of a wide workgroup: the S chunk at 0 (`stride` CT elements per row, the row tile's bank-spreading rule) and the out tile
// in its place after the last k-step (`ostride` OT elements per row; ot_size 0: no out tile, the aggregate); at z the chunk of the
// tile's own dZ rows (z_bytes: 0 unless the backward writes a dZ image), at z + z_bytes the tile's adjacency tables (TileMeta), then
// the forward's bias (bias); bytes in all
struct WideLds { int stride, ostride; size_t z, z_bytes, bytes; };
__host__ __device__ inline WideLds wide_lds(int ct_size, int ot_size, bool z, bool bias) {
    WideLds l;
    l.stride = lds_stride_dw(WIDE_KCHUNK * ct_size / 4) * 4 / ct_size;
    l.ostride = ot_size ? out_stride_dw(WIDE_COLS * ot_size / 4) * 4 / ot_size : 0;
    const size_t g_bytes = (size_t)ROWS * l.stride * ct_size;
    l.z = std::max(g_bytes, (size_t)ROWS * l.ostride * ot_size);
    l.z_bytes = z ? g_bytes : 0;
    l.bytes = l.z + l.z_bytes + (size_t)TILE_META_INTS * sizeof(int) + (bias ? WIDE_COLS * sizeof(float) : 0);
    return l;
}

// The block's WIDE_NTW output column tiles per wave against the tile over all k-steps, in the row tile's k order, into acc.  Weight
// fragments of block b (WIDE_KB k-steps, clamped to the last k-step: always valid memory) meet S on the matrix cores, weights as A (as
// in the row tile: a lane ends up with 4 consecutive columns of one row).  Blocks never straddle a chunk; a block that starts a chunk
// calls bring(kofs) first, which puts the chunk into S (barriers its own).  Two register blocks in turn: block b + 1 is requested before
// the MFMAs of block b, so the weight stream overlaps the matrix work
struct WideAcc { f32x4_t v[2][WIDE_NTW]; };
template <typename CT, typename Bring>
__device__ __forceinline__ WideAcc wide_mfma(const RowTileParams& p, const CT* S, int stride, int wave, int lane, Bring&& bring) {
    constexpr int KSTEP = sizeof(CT) == 2 ? 32 : 16;    // K consumed per fragment
    constexpr int AW = sizeof(CT) == 2 ? 8 : 4;         // CT elements per lane per k-step (16 bytes)
    const int n_tiles = ceil_div(p.NOUT, 16), ksteps = p.Kpad / KSTEP;
    const uint4* wfrag = static_cast<const uint4*>(p.wfrag);
    int tl[WIDE_NTW];                                   // this wave's output column tiles (past the last one: duplicates, not stored)
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) tl[j] = min((int)blockIdx.y * WIDE_WAVES * WIDE_NTW + j * WIDE_WAVES + wave, n_tiles - 1);
    f32x4_t acc[2][WIDE_NTW];
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) { acc[0][j] = (f32x4_t){0, 0, 0, 0}; acc[1][j] = (f32x4_t){0, 0, 0, 0}; }
    const int arow = lane & 15, kgrp = lane >> 4;

    constexpr int CKS = WIDE_KCHUNK / KSTEP;            // k-steps per chunk
    static_assert(CKS % WIDE_KB == 0, "a block of weight fragments never straddles a chunk");
    typedef uint4 WBlock[WIDE_KB][WIDE_NTW];
    auto load_block = [&](WBlock& w, int b) {
#pragma unroll
        for (int ks = 0; ks < WIDE_KB; ++ks)
#pragma unroll
            for (int j = 0; j < WIDE_NTW; ++j) w[ks][j] = wfrag[((size_t)tl[j] * ksteps + min(b * WIDE_KB + ks, ksteps - 1)) * 64 + lane];
    };
    const int n_blk = ceil_div(ksteps, WIDE_KB);
    auto run_block = [&](const WBlock& w, int b) {
        if (b >= n_blk) return;                         // workgroup-uniform
        const int kk0 = b * WIDE_KB;
        if (kk0 % CKS == 0) bring(kk0 * KSTEP);
        const int kl0 = (kk0 % CKS) * KSTEP;            // the block's first column inside the chunk
#pragma unroll
        for (int ks = 0; ks < WIDE_KB; ++ks) {
            if (kk0 + ks < ksteps) {                    // wave-uniform
                const int kl = kl0 + ks * KSTEP + kgrp * AW;
                const uint4 a0u = *reinterpret_cast<const uint4*>(S + (size_t)arow * stride + kl);
                const uint4 a1u = *reinterpret_cast<const uint4*>(S + (size_t)(arow + 16) * stride + kl);
#pragma unroll
                for (int j = 0; j < WIDE_NTW; ++j) {
                    if constexpr (sizeof(CT) == 2) {
                        const bf16x8_t bq = __builtin_bit_cast(bf16x8_t, w[ks][j]);
                        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq, __builtin_bit_cast(bf16x8_t, a0u), acc[0][j], 0, 0, 0);
                        acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq, __builtin_bit_cast(bf16x8_t, a1u), acc[1][j], 0, 0, 0);
                    } else {
                        const f32x4_t bq = __builtin_bit_cast(f32x4_t, w[ks][j]);
                        const f32x4_t a0 = __builtin_bit_cast(f32x4_t, a0u), a1 = __builtin_bit_cast(f32x4_t, a1u);
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[s], a0[s], acc[0][j], 0, 0, 0);
                            acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[s], a1[s], acc[1][j], 0, 0, 0);
                        }
                    }
                }
            }
        }
    };
    WBlock wa, wb;
    load_block(wa, 0);
    for (int b = 0; b < n_blk; b += 2) {
        load_block(wb, b + 1);
        run_block(wa, b);
        load_block(wa, b + 2);
        run_block(wb, b + 1);
    }
    WideAcc r;
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) { r.v[0][j] = acc[0][j]; r.v[1][j] = acc[1][j]; }
    return r;
}

// The row tile's epilogue (BWD: the backward's) on acc into the out tile O (in S's place), then the block's whole rows leave in 16-byte
// pieces (BWD with relu_src: as the layer below's dZ).  sbias: the block's bias in LDS (forward); seed_off: added to the dropout seed
template <typename OT, bool BWD>
__device__ __forceinline__ void wide_store(const RowTileParams& p, const TileMeta& m, const WideAcc& acc, OT* O, int ostride,
                                           const float* sbias, uint64_t seed_off, int tid, int lane, int wave) {
    const int r0 = (int)blockIdx.x * ROWS, c_lo = (int)blockIdx.y * WIDE_COLS, n_tiles = ceil_div(p.NOUT, 16);
    __syncthreads();
    float den[2], inv[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) { den[mt] = m.rden[mt * 16 + (lane & 15)]; inv[mt] = m.rinv[mt * 16 + (lane & 15)]; }
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) {
        const int t = (int)blockIdx.y * WIDE_WAVES * WIDE_NTW + j * WIDE_WAVES + wave;
        if (t >= n_tiles) continue;
        const int col0 = t * 16 + (lane >> 4) * 4;
        const f32x4_t aj[2] = {acc.v[0][j], acc.v[1][j]};
        epilogue_tile<OT, BWD>(p, aj, col0, col0 - c_lo, r0, den, inv, sbias, O, ostride, seed_off, lane);
    }
    __syncthreads();
    store_tile_rows<OT, BWD, WIDE_THREADS>(p, O, ostride, m.rden, r0, c_lo, min(p.NOUT, c_lo + WIDE_COLS) - c_lo, tid);
}

// f(CT{}, IT{}, OT{}) for precision combination c (precision_combo, layer_common.h); a refusal (c < 0) is returned as it is
template <typename F>
static int with_combo(int c, F&& f) {
    switch (c) {
    case 0: return f(float{}, float{}, float{});
    case 1: return f(bf16_t{}, float{}, float{});
    case 2: return f(bf16_t{}, float{}, bf16_t{});
    case 3: return f(bf16_t{}, bf16_t{}, float{});
    case 4: return f(bf16_t{}, bf16_t{}, bf16_t{});
    default: return c;
    }
}

}  // namespace gcnpt
