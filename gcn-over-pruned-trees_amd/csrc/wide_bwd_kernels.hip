// The wide form of the GCN layer backward-data (wide_bwd_kernel below), next to the wide forward of wide_kernels.hip and built from the same
// phases of the row tile (rowtile_phases.h).  Its k-loop, epilogue, row stores and LDS layout are the forward transform's: wide_common.h.
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
    const int tile_id = (int)blockIdx.x, n_blocks = (int)gridDim.x, r0 = tile_id * ROWS;
    const WideLds L = wide_lds((int)sizeof(CT), (int)sizeof(OT), p.frag_out != nullptr, false);
    const int stride = L.stride;
    CT* S = reinterpret_cast<CT*>(smem_raw);            // the chunk of G
    OT* O = reinterpret_cast<OT*>(smem_raw);            // the out tile takes its place after the last k-step
    CT* Z = reinterpret_cast<CT*>(smem_raw + L.z);      // with z_frag: the chunk of the tile's own dZ rows (the image's source)
    const TileMeta m = tile_meta(reinterpret_cast<int*>(smem_raw + L.z + L.z_bytes));
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

    // the weight-block MFMA loop over all k-steps, the chunk of G gathered where a block starts one; then the row tile's backward
    // epilogue and row stores (with relu_src: as the layer below's dZ)
    const WideAcc acc = wide_mfma(p, S, stride, wave, lane, gather_chunk);
    wide_store<OT, true>(p, m, acc, O, L.ostride, nullptr, 0, tid, lane, wave);
}

template <typename CT, typename IT, typename OT, int VEC, bool DZIN>
static int wide_bwd_launch_vec(hipStream_t s, const RowTileParams& p) {
    const size_t lds = wide_lds((int)sizeof(CT), (int)sizeof(OT), p.frag_out != nullptr, false).bytes;
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
    return with_combo(precision_combo(compute, in_dtype, out_dtype), [&](auto ct, auto it, auto ot) {
        return wide_bwd_launch_t<decltype(ct), decltype(it), decltype(ot)>(s, p, dzin);
    });
}

}  // namespace gcnpt
