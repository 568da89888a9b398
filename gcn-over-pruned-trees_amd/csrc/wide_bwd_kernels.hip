// The wide form of the GCN layer backward-data (wide_bwd_kernel below), next to the wide forward of wide_kernels.hip and built from the same
// phases of the row tile (rowtile_phases.h).
#include "wide_common.h"

namespace gcnpt {

// The wide form of the layer backward-data, dh = ((A+I)^T dZ) W (reference model/gcn.py:269-271 differentiated), for layers whose 32-row
// tile of G = (A+I)^T dZ, H columns wide, does not fit the row tile's LDS twice (rowtile_bwd_too_wide: fp32 H > 608, bf16 H > 1216).  ONE
// launch and no workspace: one workgroup per (32-row tile, WIDE_COLS output columns) walks the H columns of its tile in WIDE_KCHUNK chunks:
//   gather    the chunk of G into LDS exactly as the row tile gathers it (TileGather with KCHUNK and the backward's loader: dZ derived from
//             dY, Y and the degree, or ready-made rows with DZIN; same ELL heads, same neighbour rounds, same fp32 sums).  The workgroups of
//             column block 0 also write the chunk's column tiles of the dZ fragment image (z_frag) from the tile's own rows, the image the
//             weight gradient reads;
//   MFMA      the chunk's k-steps against the packed weight image of the block's output columns, in the row tile's k order, accumulated in
//             registers (the weight fragments double-buffered as in wide_transform_kernel);
// then the row tile's backward epilogue and row stores: dh, or with relu_src the hand-over dZ = dh * 1[input > 0] * next_scale / (deg+1)
// to the layer below.  dh and the dZ image are bit-identical to the row tile's wherever both run (GCNPT_OPT_WIDE_BWD = 1 forces this form;
// tests/test_gpu_wide_bwd.py compares the two).  The gather is repeated once per column block: a pruned tree leaves ~4 rows of a tile that
// aggregate anything, every other row is one load.  It never carries the layer above's weight gradient (rowtile_wgrad_kernel).
template <typename CT, typename IT, typename OT, int VEC, bool DZIN>
__global__ __launch_bounds__(WIDE_THREADS) void wide_bwd_kernel(const RowTileParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr bool MASKED = !DZIN;                      // the loader computes dZ = dY * 1[Y>0] * scale / (deg+1) itself
    constexpr bool TWO = MASKED && sizeof(IT) == 4;     // the backward row tile's rounds: two fp32 streams per row, fewer rows in flight
    constexpr int NBU = TWO ? 2 : 4, ITEMS = TWO ? 2 : 3;
    constexpr int KSTEP = sizeof(CT) == 2 ? 32 : 16;    // K consumed per fragment
    constexpr int AW = sizeof(CT) == 2 ? 8 : 4;         // CT elements per lane per k-step (16 bytes)
    const int tile_id = (int)blockIdx.x, n_blocks = (int)gridDim.x, r0 = tile_id * ROWS;
    const int c_lo = (int)blockIdx.y * WIDE_COLS;
    const int stride = wide_s_stride((int)sizeof(CT));
    const int ostride = out_stride_dw(WIDE_COLS * (int)sizeof(OT) / 4) * 4 / (int)sizeof(OT);
    const size_t g_bytes = (size_t)ROWS * stride * sizeof(CT);
    const size_t s_bytes = std::max(g_bytes, (size_t)ROWS * ostride * sizeof(OT));
    CT* S = reinterpret_cast<CT*>(smem_raw);            // the chunk of G
    OT* O = reinterpret_cast<OT*>(smem_raw);            // the out tile takes its place after the last k-step
    CT* Z = reinterpret_cast<CT*>(smem_raw + s_bytes);  // with z_frag: the chunk of the tile's own dZ rows (the image's source)
    int* meta = reinterpret_cast<int*>(smem_raw + s_bytes + (p.frag_out ? g_bytes : 0));
    const TileMeta m = tile_meta(meta);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool emit = p.frag_out && blockIdx.y == 0;

    const TileHeads heads = load_tile_heads(p, r0, lane);
    park_tile_heads<true>(p, m, heads, r0, lane, p.out != nullptr);
    wave_lds_fence();
    // cleared accumulators for the weight gradients that follow, over the whole grid
    {
        const int bid = (int)(blockIdx.y * gridDim.x + blockIdx.x), nb = (int)(gridDim.x * gridDim.y);
#pragma unroll
        for (int z = 0; z < 4; ++z)
            if (p.zero_p[z])
                for (int i = bid * WIDE_THREADS + tid; i < p.zero_n[z]; i += nb * WIDE_THREADS) p.zero_p[z][i] = 0.0f;
    }

    // the chunk of G at column kofs into S (and of dZ into Z), its image tiles out.  Barriers on both sides: every wave is done with the
    // previous chunk, every row is in place after
    auto gather_chunk = [&](int kofs) __attribute__((always_inline)) {
        const int kw = min(WIDE_KCHUNK, p.Kpad - kofs), nck = kw / 8;       // kw: a multiple of 16, >= 16
        __syncthreads();
        const TileGather<CT, IT, MASKED, VEC, NBU, true> G{p, m, S, stride, r0, kofs, nck, 0xffffffffu / (unsigned)nck + 1u};
        const int n_g = *m.gcount * nck;                // rows that aggregate something: (list slot, 8-column chunk) items
        for (int base = 0; base < n_g; base += WIDE_THREADS) {
            GatherItem<IT, NBU> g;
            G.issue(n_g, base + tid, g);
            G.finish(n_g, base + tid, g);
        }
        const int n_items = ROWS * nck;                 // every row's own chunk: into Z, and into S unless the row aggregates
        for (int b0 = 0; b0 < n_items; b0 += ITEMS * WIDE_THREADS) {
            raw8<IT> s[ITEMS], sy[ITEMS];
#pragma unroll
            for (int u = 0; u < ITEMS; ++u) G.issue_self(b0 + u * WIDE_THREADS + tid, s[u], sy[u]);
#pragma unroll
            for (int u = 0; u < ITEMS; ++u) G.template copy_item<true>(b0 + u * WIDE_THREADS + tid, s[u], sy[u], Z);
        }
        __syncthreads();
        if (emit) {                                     // tile t of the whole image is tile t - kofs/16 of this chunk
            const int t0 = kofs / 16, nt = min(kw, round_up(p.K, 16) - kofs) / 16;
            const size_t tile_u4 = (size_t)n_blocks * (sizeof(CT) == 2 ? 1 : 2) * 64;
            emit_tile_image(static_cast<uint4*>(p.frag_out) + (size_t)t0 * tile_u4, Z, stride, wave, WIDE_WAVES, nt, lane, (size_t)n_blocks, tile_id, true);
        }
    };
    if (!p.out) {                                       // only the image is wanted (a one-block-column grid)
        for (int kofs = 0; kofs < p.Kpad; kofs += WIDE_KCHUNK) gather_chunk(kofs);
        return;
    }

    const int n_tiles = ceil_div(p.NOUT, 16), ksteps = p.Kpad / KSTEP;
    const uint4* wfrag = static_cast<const uint4*>(p.wfrag);
    int tl[WIDE_NTW];                                   // this wave's output column tiles (past the last one: duplicates, not stored)
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) tl[j] = min((int)blockIdx.y * WIDE_WAVES * WIDE_NTW + j * WIDE_WAVES + wave, n_tiles - 1);
    f32x4_t acc[2][WIDE_NTW];
#pragma unroll
    for (int j = 0; j < WIDE_NTW; ++j) { acc[0][j] = (f32x4_t){0, 0, 0, 0}; acc[1][j] = (f32x4_t){0, 0, 0, 0}; }
    const int arow = lane & 15, kgrp = lane >> 4;

    // the weight fragments of block b (WIDE_KB k-steps, clamped to the last k-step: always valid memory), and the block's k-steps on the
    // matrix cores, weights as A (as in the row tile).  Blocks never straddle a chunk; a block that starts a chunk gathers it first
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
        if (kk0 % CKS == 0) gather_chunk(kk0 * KSTEP);
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

    // the row tile's backward epilogue into the out tile (in S's place), then whole rows leave in 16-byte pieces (with relu_src: as the
    // layer below's dZ)
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
        epilogue_tile<OT, true>(p, aj, col0, col0 - c_lo, r0, den, inv, nullptr, O, ostride, 0, lane);
    }
    __syncthreads();
    store_tile_rows<OT, true, WIDE_THREADS>(p, O, ostride, m.rden, r0, c_lo, min(p.NOUT, c_lo + WIDE_COLS) - c_lo, tid);
}

template <typename CT, typename IT, typename OT, int VEC, bool DZIN>
static int wide_bwd_launch_vec(hipStream_t s, const RowTileParams& p) {
    const int stride = wide_s_stride((int)sizeof(CT));
    const int ostride = out_stride_dw(WIDE_COLS * (int)sizeof(OT) / 4) * 4 / (int)sizeof(OT);
    const size_t g_bytes = (size_t)ROWS * stride * sizeof(CT);
    const size_t lds = std::max(g_bytes, (size_t)ROWS * ostride * sizeof(OT)) + (p.frag_out ? g_bytes : 0) + (size_t)TILE_META_INTS * sizeof(int);
    const dim3 g(ceil_div(p.N, ROWS), p.out ? ceil_div(ceil_div(p.NOUT, 16), WIDE_WAVES * WIDE_NTW) : 1);
    auto kern = wide_bwd_kernel<CT, IT, OT, VEC, DZIN>;
    GCNPT_LDS_ATTR_ONCE(kern, 160 * 1024);
    hipLaunchKernelGGL(kern, g, dim3(WIDE_THREADS), lds, s, p);
    note_launch((int)(g.x * g.y), WIDE_THREADS, lds, sizeof(p));
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

template <typename CT, typename IT, typename OT>
static int wide_bwd_launch_t(hipStream_t s, const RowTileParams& p, bool dzin) {
    if (dzin) {
        if (p.vec_in == 8) return wide_bwd_launch_vec<CT, IT, OT, 8, true>(s, p);
        if (p.vec_in == 4) return wide_bwd_launch_vec<CT, IT, OT, 4, true>(s, p);
        return wide_bwd_launch_vec<CT, IT, OT, 0, true>(s, p);
    }
    if (p.vec_in == 8) return wide_bwd_launch_vec<CT, IT, OT, 8, false>(s, p);
    if (p.vec_in == 4) return wide_bwd_launch_vec<CT, IT, OT, 4, false>(s, p);
    return wide_bwd_launch_vec<CT, IT, OT, 0, false>(s, p);
}

int wide_bwd_launch(hipStream_t s, const RowTileParams& p, int in_dtype, int out_dtype, int compute, bool dzin) {
    if (compute == GCNPT_F32) {
        if (in_dtype != GCNPT_F32 || out_dtype != GCNPT_F32) return fail(GCNPT_E_UNSUPPORTED, "compute_dtype f32 needs f32 activations");
        return wide_bwd_launch_t<float, float, float>(s, p, dzin);
    }
    if (in_dtype == GCNPT_F32)
        return out_dtype == GCNPT_F32 ? wide_bwd_launch_t<bf16_t, float, float>(s, p, dzin) : wide_bwd_launch_t<bf16_t, float, bf16_t>(s, p, dzin);
    return out_dtype == GCNPT_F32 ? wide_bwd_launch_t<bf16_t, bf16_t, float>(s, p, dzin) : wide_bwd_launch_t<bf16_t, bf16_t, bf16_t>(s, p, dzin);
}

}  // namespace gcnpt
