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
// The transform's k-loop, epilogue and row stores and both kernels' LDS layout are wide_common.h's, shared with the wide backward-data.
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
    const WideLds L = wide_lds((int)sizeof(CT), 0, false, false);
    const int stride = L.stride;
    CT* S = reinterpret_cast<CT*>(smem_raw);
    const TileMeta m = tile_meta(reinterpret_cast<int*>(smem_raw + L.z + L.z_bytes));
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
    constexpr int RKS = sizeof(CT) == 2 ? 1 : 2;        // image k-steps (of rows) per row tile
    const int tile_id = (int)blockIdx.x, n_blocks = (int)gridDim.x, r0 = tile_id * ROWS;
    const int c_lo = (int)blockIdx.y * WIDE_COLS;
    const WideLds L = wide_lds((int)sizeof(CT), (int)sizeof(OT), false, true);
    const int stride = L.stride;
    CT* S = reinterpret_cast<CT*>(smem_raw);
    OT* O = reinterpret_cast<OT*>(smem_raw);            // the out tile takes the S chunk's place after the last k-step
    int* meta = reinterpret_cast<int*>(smem_raw + L.z + L.z_bytes);
    const TileMeta m = tile_meta(meta);
    float* sbias = reinterpret_cast<float*>(meta + TILE_META_INTS);       // [WIDE_COLS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint64_t seed_off = 0;
    if (p.seed_dev) seed_off = *p.seed_dev;

    const TileHeads heads = load_tile_heads(p, r0, lane);       // denominators of the epilogue
    park_tile_heads<false>(p, m, heads, r0, lane, true);
    if (tid < WIDE_COLS) sbias[tid] = p.bias[min(c_lo + tid, p.NOUT - 1)];

    const int ntk = ceil_div(p.K, 16);
    const uint4* img = static_cast<const uint4*>(p.frag_out);
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
    // (2) the weight-block MFMA loop over all k-steps, a chunk of the image brought into S where a block starts one
    const WideAcc acc = wide_mfma(p, S, stride, wave, lane, fill_chunk);
    // (3) the row tile's epilogue into the out tile (in S's place), then whole rows leave in 16-byte pieces
    wide_store<OT, false>(p, m, acc, O, L.ostride, sbias, seed_off, tid, lane, wave);
}

template <typename CT, typename IT, typename OT>
static int wide_launch(hipStream_t s, const RowTileParams& p) {
    GCNPT_REQUIRE(p.frag_out, "layer_fwd: Din=%d, H=%d takes the wide form, which stages S = (A+I)h through s_frag: pass "
                  "gcnpt_frag_bytes(rows, Din, compute_dtype) bytes (gcnpt_layer_fwd_needs_s_frag says where)", p.K, p.NOUT);
    const int n_rt = ceil_div(p.N, ROWS);
    const size_t lds_a = wide_lds((int)sizeof(CT), 0, false, false).bytes;
    const dim3 ga(n_rt, ceil_div(p.Kpad, WIDE_KCHUNK));
    if (p.vec_in == 8) hipLaunchKernelGGL((wide_aggregate_kernel<CT, IT, 8>), ga, dim3(WIDE_THREADS), lds_a, s, p);
    else if (p.vec_in == 4) hipLaunchKernelGGL((wide_aggregate_kernel<CT, IT, 4>), ga, dim3(WIDE_THREADS), lds_a, s, p);
    else hipLaunchKernelGGL((wide_aggregate_kernel<CT, IT, 0>), ga, dim3(WIDE_THREADS), lds_a, s, p);
    GCNPT_HIP_CHECK(hipGetLastError());
    const size_t lds_t = wide_lds((int)sizeof(CT), (int)sizeof(OT), false, true).bytes;
    const dim3 gt(n_rt, ceil_div(ceil_div(p.NOUT, 16), WIDE_WAVES * WIDE_NTW));
    hipLaunchKernelGGL((wide_transform_kernel<CT, OT>), gt, dim3(WIDE_THREADS), lds_t, s, p);
    note_launch((int)(gt.x * gt.y), WIDE_THREADS, lds_t, sizeof(p));
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

int wide_fwd_launch(hipStream_t s, const RowTileParams& p, int in_dtype, int out_dtype, int compute) {
    return with_combo(precision_combo(compute, in_dtype, out_dtype), [&](auto ct, auto it, auto ot) {
        return wide_launch<decltype(ct), decltype(it), decltype(ot)>(s, p);
    });
}

}  // namespace gcnpt
