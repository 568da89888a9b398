// The wide form of the GCN layer forward, reference model/gcn.py:269-271 + 390-393, for inputs whose 32-row tile S = (A+I) h does not fit
// the one-shot row-tile kernel's LDS next to its out tile (rowtile_fwd_too_wide: in fp32 Din > 1024 at H = 200, e.g. the 1084 columns of
// BERT-large vectors + POS + NER that the no-RNN model feeds its first layer, model/gcn.py:136,235-236).  Two launches on the caller's
// stream, no dependence between workgroups, so the pair captures into a hipGraph like every other layer launch:
//   aggregate  one workgroup per (32-row tile, chunk of WIDE_KCHUNK columns): the chunk of S gathered exactly as the row tile gathers it
//              (TileGather with KCHUNK: same ELL heads, same neighbour rounds, same sums), written as its column tiles of the S fragment
//              image (include/gcnpt.h) -- the image gcnpt_layer_bwd_weight reads anyway, here staged through the caller's s_frag;
//   transform  one workgroup per (32-row tile, WIDE_COLS output columns): the tile's image back into LDS row by row, one chunk at a
//              time, against the packed weight image (gcnpt_pack_weights) over all k-steps in the row tile's order, then the row tile's
//              own epilogue (bias, denominators, ReLU, dropout mask) and row stores.
// The same products are summed in the same order as in the row tile, so outputs and S image are bit-identical to it wherever both run
// (GCNPT_OPT_WIDE_FORM = 1 forces this form; tests/test_gpu_wide_layers.py compares the two).
// Both operands of the transform are in fragment order already: every global load is a lane-linear 16-byte load.  A 4-wave workgroup
// owns 128 output columns, so it streams half of the weight image of a 200-column layer (555 KB in fp32 at Din = 1084) and a 32 x Din
// slice of the S image (139 KB) through its CU.
#include "wide_common.h"

namespace gcnpt {

template <typename CT, typename IT, int VEC>
__global__ __launch_bounds__(WIDE_THREADS) void wide_aggregate_kernel(const RowTileParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int NBU = 4, ITEMS = 4;                   // NBU: the forward row tile's neighbour rounds (the same sums in the same order)
    const int tile_id = (int)blockIdx.x, n_blocks = (int)gridDim.x, r0 = tile_id * ROWS;
    const int kofs = (int)blockIdx.y * WIDE_KCHUNK, kw = min(WIDE_KCHUNK, p.Kpad - kofs);       // kw: a multiple of 16, >= 16
    const int stride = wide_s_stride((int)sizeof(CT));
    CT* S = reinterpret_cast<CT*>(smem_raw);
    const TileMeta m = tile_meta(reinterpret_cast<int*>(smem_raw + (size_t)ROWS * stride * sizeof(CT)));
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // the tile's adjacency, parked as the row tile parks it (every wave its own copy, no barrier)
    const TileHeads heads = load_tile_heads(p, r0, lane);
    park_tile_heads<false>(p, m, heads, r0, lane, true);
    wave_lds_fence();

    const int nck = kw / 8;
    const TileGather<CT, IT, false, VEC, NBU, true> G{p, m, S, stride, r0, kofs, nck, 0xffffffffu / (unsigned)nck + 1u};
    // rows that aggregate something: (list slot, 8-column chunk) items over all waves
    const int n_g = *m.gcount * nck;
    for (int base = 0; base < n_g; base += WIDE_THREADS) {
        GatherItem<IT, NBU> g;
        G.issue(n_g, base + tid, g);
        G.finish(n_g, base + tid, g);
    }
    // every other row: a plain copy (rows past the end and columns past K: zeros, as in the row tile)
    const int n_items = ROWS * nck;
    for (int b0 = 0; b0 < n_items; b0 += ITEMS * WIDE_THREADS) {
        raw8<IT> s[ITEMS], sy[ITEMS];
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) G.issue_self(b0 + u * WIDE_THREADS + tid, s[u], sy[u]);
#pragma unroll
        for (int u = 0; u < ITEMS; ++u) G.template copy_item<false>(b0 + u * WIDE_THREADS + tid, s[u], sy[u], nullptr);
    }
    __syncthreads();

    // the chunk's column tiles of the image: tile t of the whole image is tile t - kofs/16 of this chunk
    const int t0 = kofs / 16, nt = min(kw, round_up(p.K, 16) - kofs) / 16;
    const size_t tile_u4 = (size_t)n_blocks * (sizeof(CT) == 2 ? 1 : 2) * 64;       // 16-byte units per column tile of the image
    emit_tile_image(static_cast<uint4*>(p.frag_out) + (size_t)t0 * tile_u4, S, stride, wave, WIDE_WAVES, nt, lane, (size_t)n_blocks, tile_id, false);
}

template <typename CT, typename OT>
__global__ __launch_bounds__(WIDE_THREADS) void wide_transform_kernel(const RowTileParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int KSTEP = sizeof(CT) == 2 ? 32 : 16;    // K consumed per fragment
    constexpr int AW = sizeof(CT) == 2 ? 8 : 4;         // CT elements per lane per k-step (16 bytes)
    constexpr int RKS = sizeof(CT) == 2 ? 1 : 2;        // image k-steps (of rows) per row tile
    const int tile_id = (int)blockIdx.x, n_blocks = (int)gridDim.x, r0 = tile_id * ROWS;
    const int c_lo = (int)blockIdx.y * WIDE_COLS;
    const int stride = wide_s_stride((int)sizeof(CT));
    const int ostride = out_stride_dw(WIDE_COLS * (int)sizeof(OT) / 4) * 4 / (int)sizeof(OT);
    const size_t s_bytes = std::max((size_t)ROWS * stride * sizeof(CT), (size_t)ROWS * ostride * sizeof(OT));
    CT* S = reinterpret_cast<CT*>(smem_raw);
    OT* O = reinterpret_cast<OT*>(smem_raw);            // the out tile takes the S chunk's place after the last k-step
    int* meta = reinterpret_cast<int*>(smem_raw + s_bytes);
    const TileMeta m = tile_meta(meta);
    float* sbias = reinterpret_cast<float*>(meta + TILE_META_INTS);       // [WIDE_COLS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint64_t seed_off = 0;
    if (p.seed_dev) seed_off = *p.seed_dev;

    const TileHeads heads = load_tile_heads(p, r0, lane);       // denominators of the epilogue
    park_tile_heads<false>(p, m, heads, r0, lane, true);
    if (tid < WIDE_COLS) sbias[tid] = p.bias[min(c_lo + tid, p.NOUT - 1)];

    const int n_tiles = ceil_div(p.NOUT, 16), ksteps = p.Kpad / KSTEP, ntk = ceil_div(p.K, 16);
    const uint4* wfrag = static_cast<const uint4*>(p.wfrag);
    const uint4* img = static_cast<const uint4*>(p.frag_out);
    int tl[WIDE_NTW];                                   // this wave's output column tiles (past the last one: duplicates, not stored)
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) tl[j] = min((int)blockIdx.y * WIDE_WAVES * WIDE_NTW + j * WIDE_WAVES + wave, n_tiles - 1);
    f32x4_t acc[2][WIDE_NTW];
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) { acc[0][j] = (f32x4_t){0, 0, 0, 0}; acc[1][j] = (f32x4_t){0, 0, 0, 0}; }
    const int arow = lane & 15, kgrp = lane >> 4;

    // (1) chunk c of the tile's image (16 columns x one k-step of rows per image tile) -> S rows; columns past the image (bf16, Kpad >
    //     round_up(K, 16)) are 0.  Barriers on both sides: every wave is done with the previous chunk, every row is in place after
    auto fill_chunk = [&](int kofs) {
        const int kw = min(WIDE_KCHUNK, p.Kpad - kofs);
        __syncthreads();
        const int t0 = kofs / 16, nct = kw / 16;
        for (int it = wave; it < nct * RKS; it += WIDE_WAVES) {
            const int tc = it / RKS, kk = it - tc * RKS, t = t0 + tc;
            uint4 u = make_uint4(0, 0, 0, 0);
            if (t < ntk) u = img[((size_t)t * n_blocks * RKS + (size_t)tile_id * RKS + kk) * 64 + lane];
            CT* col = S + tc * 16 + (lane & 15);
            if constexpr (sizeof(CT) == 2) {            // lane: rows 8 (lane >> 4) + j, j = 0..7, two per dword
                const int rb = 8 * (lane >> 4);
                const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    col[(size_t)(rb + 2 * q) * stride] = (bf16_t)(w[q] & 0xffffu);
                    col[(size_t)(rb + 2 * q + 1) * stride] = (bf16_t)(w[q] >> 16);
                }
            } else {                                    // lane: rows 16 kk + 4 (lane >> 4) + s, s = 0..3
                const int rb = 16 * kk + 4 * (lane >> 4);
                col[(size_t)(rb + 0) * stride] = __uint_as_float(u.x);
                col[(size_t)(rb + 1) * stride] = __uint_as_float(u.y);
                col[(size_t)(rb + 2) * stride] = __uint_as_float(u.z);
                col[(size_t)(rb + 3) * stride] = __uint_as_float(u.w);
            }
        }
        __syncthreads();
    };
    // (2) the weight fragments of block b (WIDE_KB k-steps, clamped to the last k-step: always valid memory), and the block's k-steps on
    //     the matrix cores, weights as A (as in the row tile: a lane ends up with 4 consecutive columns of one row).  Blocks never straddle
    //     a chunk; a block that starts a chunk brings the chunk into LDS first
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
        if (kk0 % CKS == 0) fill_chunk(kk0 * KSTEP);
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
    // two register blocks in turn: block b + 1 is requested before the MFMAs of block b, so the weight stream overlaps the matrix work
    WBlock wa, wb;
    load_block(wa, 0);
    for (int b = 0; b < n_blk; b += 2) {
        load_block(wb, b + 1);
        run_block(wa, b);
        load_block(wa, b + 2);
        run_block(wb, b + 1);
    }

    // (3) the row tile's epilogue into the out tile (in S's place), then whole rows leave in 16-byte pieces
    __syncthreads();
    float den[2], inv[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) { den[mt] = m.rden[mt * 16 + (lane & 15)]; inv[mt] = m.rinv[mt * 16 + (lane & 15)]; }
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) {
        const int t = (int)blockIdx.y * WIDE_WAVES * WIDE_NTW + j * WIDE_WAVES + wave;
        if (t >= n_tiles) continue;
        const int col0 = t * 16 + (lane >> 4) * 4;
        const f32x4_t aj[2] = {acc[0][j], acc[1][j]};
        epilogue_tile<OT, false>(p, aj, col0, col0 - c_lo, r0, den, inv, sbias, O, ostride, seed_off, lane);
    }
    __syncthreads();
    store_tile_rows<OT, false, WIDE_THREADS>(p, O, ostride, m.rden, r0, c_lo, min(p.NOUT, c_lo + WIDE_COLS) - c_lo, tid);
}

template <typename CT, typename IT, typename OT>
static int wide_launch(hipStream_t s, const RowTileParams& p) {
    GCNPT_REQUIRE(p.frag_out, "layer_fwd: Din=%d, H=%d takes the wide form, which stages S = (A+I)h through s_frag: pass "
                  "gcnpt_frag_bytes(rows, Din, compute_dtype) bytes (gcnpt_layer_fwd_needs_s_frag says where)", p.K, p.NOUT);
    const int n_rt = ceil_div(p.N, ROWS);
    const int stride = wide_s_stride((int)sizeof(CT));
    const size_t meta = (size_t)TILE_META_INTS * sizeof(int);
    const size_t lds_a = (size_t)ROWS * stride * sizeof(CT) + meta;
    const dim3 ga(n_rt, ceil_div(p.Kpad, WIDE_KCHUNK));
    if (p.vec_in == 8) hipLaunchKernelGGL((wide_aggregate_kernel<CT, IT, 8>), ga, dim3(WIDE_THREADS), lds_a, s, p);
    else if (p.vec_in == 4) hipLaunchKernelGGL((wide_aggregate_kernel<CT, IT, 4>), ga, dim3(WIDE_THREADS), lds_a, s, p);
    else hipLaunchKernelGGL((wide_aggregate_kernel<CT, IT, 0>), ga, dim3(WIDE_THREADS), lds_a, s, p);
    GCNPT_HIP_CHECK(hipGetLastError());
    const int ostride = out_stride_dw(WIDE_COLS * (int)sizeof(OT) / 4) * 4 / (int)sizeof(OT);
    const size_t lds_t = std::max((size_t)ROWS * stride * sizeof(CT), (size_t)ROWS * ostride * sizeof(OT)) + meta + WIDE_COLS * sizeof(float);
    const dim3 gt(n_rt, ceil_div(ceil_div(p.NOUT, 16), WIDE_WAVES * WIDE_NTW));
    hipLaunchKernelGGL((wide_transform_kernel<CT, OT>), gt, dim3(WIDE_THREADS), lds_t, s, p);
    note_launch((int)(gt.x * gt.y), WIDE_THREADS, lds_t, sizeof(p));
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

int wide_fwd_launch(hipStream_t s, const RowTileParams& p, int in_dtype, int out_dtype, int compute) {
    if (compute == GCNPT_F32) {
        if (in_dtype != GCNPT_F32 || out_dtype != GCNPT_F32) return fail(GCNPT_E_UNSUPPORTED, "compute_dtype f32 needs f32 activations");
        return wide_launch<float, float, float>(s, p);
    }
    if (in_dtype == GCNPT_F32) return out_dtype == GCNPT_F32 ? wide_launch<bf16_t, float, float>(s, p) : wide_launch<bf16_t, float, bf16_t>(s, p);
    return out_dtype == GCNPT_F32 ? wide_launch<bf16_t, bf16_t, float>(s, p) : wide_launch<bf16_t, bf16_t, bf16_t>(s, p);
}

}  // namespace gcnpt
