// Rewrites of a batch's tree arrays from one layout into another (gfx950); the layouts and the rules shared by the four kernels are in
// tree_layout.h.
//
//   gather_trees_kernel          cached padded -> padded [B,T]         (N4: a batch assembled from a dataset that was pruned once)
//   gather_trees_packed_kernel   cached padded -> token-packed
//   compact_trees_kernel         padded -> padded over the kept tokens (N1: "pooled-only" rows)
//   pack_trees_kernel            padded -> token-packed
//
// Token-packed: variable-length batches as [sum(len), width] rows + cu_seqlens instead of the reference's [B, T, width] padded to the
// longest sentence (data/loader.py:109-121, model/gcn.py:96-97,106).  The reference's adjacency is block diagonal (one [T,T] block per
// sentence, model/tree.py:167-204), so a batch of pruned trees is ONE sparse matrix over the packed token rows: row r = cu_seqlens[b] + i
// for token i of sentence b, columns are packed row numbers too (entries and their order unchanged); the layer kernels run on it
// unchanged with T = 0 ("columns are absolute"), on sum(len) rows instead of B*T.
#include "pack_common.h"
#include "tree_layout.h"

namespace gcnpt {

constexpr int REWRITE_THREADS = 256;

// Sentence idx[b] of the cached PrunedTrees (S sentences padded to Ts, capacity cap_s) becomes sentence b of a PrunedTrees
// for [B, T].  Columns are sentence-local, so entries and ELL heads are copied as they are; only offsets are re-based.
__global__ __launch_bounds__(REWRITE_THREADS) void gather_trees_kernel(const TreeSrc src, const int32_t* __restrict__ src_len,
                                                                      int S, int Ts, int cap_s, const int64_t* __restrict__ idx,
                                                                      int B, int T, int cap, const TreeArrays dst, const PackParams pk,
                                                                      int pk_dtype) {
    __shared__ int scratch[REWRITE_THREADS / WAVE][1];
    if ((int)blockIdx.x >= B) {    // side job of gcnpt_gather_trees_pack
        pack_side_job(pk, pk_dtype, B);
        return;
    }
    const int b = blockIdx.x, t = threadIdx.x;
    const CachedSentence c = lookup_cached_sentence(src.row_ptr, src.rowT_ptr, src.status, src_len, S, Ts, cap_s, idx, b, T, cap);
    const size_t s = c.s;
    const bool ok = c.code == 0;                         // otherwise: an empty, fully masked sentence, as the pruner leaves it
    for (int i = t; i <= T; i += REWRITE_THREADS) {
        const size_t o = s * (Ts + 1) + min(i, Ts);
        dst.row_ptr[(size_t)b * (T + 1) + i] = b * cap + (ok ? src.row_ptr[o] - (int)s * cap_s : 0);
        if (dst.rowT_ptr) dst.rowT_ptr[(size_t)b * (T + 1) + i] = b * cap + (ok ? src.rowT_ptr[o] - (int)s * cap_s : 0);
    }
    for (int k = t; k < c.nnz; k += REWRITE_THREADS) {
        dst.col_idx[(size_t)b * cap + k] = src.col_idx[s * cap_s + k];
        if (dst.label) dst.label[(size_t)b * cap + k] = src.label[s * cap_s + k];
    }
    if (dst.colT_idx)
        for (int k = t; k < c.nnzT; k += REWRITE_THREADS) dst.colT_idx[(size_t)b * cap + k] = src.colT_idx[s * cap_s + k];
    const i32x4_t z = {0, 0, 0, 0};
    for (int q = t; q < 2 * T; q += REWRITE_THREADS) {   // ELL heads, 16 bytes at a time
        const int i = q >> 1;
        const bool have = ok && i < Ts;
        const size_t o = (s * Ts + min(i, Ts - 1)) * 2 + (q & 1);
        reinterpret_cast<i32x4_t*>(dst.ell)[(size_t)b * T * 2 + q] = have ? reinterpret_cast<const i32x4_t*>(src.ell)[o] : z;
        if (dst.ellT) reinterpret_cast<i32x4_t*>(dst.ellT)[(size_t)b * T * 2 + q] = have ? reinterpret_cast<const i32x4_t*>(src.ellT)[o] : z;
    }
    if (dst.pool_mask)
        for (int i = t; i < T; i += REWRITE_THREADS)
            dst.pool_mask[(size_t)b * T + i] = (ok && i < Ts) ? src.pool_mask[s * Ts + i] : (uint8_t)1;
    if (t == 0) dst.status[b] = c.code;
    if (b == 0) {                                        // status[B] = longest sentence of the batch (gcn.py:97): no memset, no atomics
        int m[1] = {0};
        for (int j = t; j < B; j += REWRITE_THREADS)
            m[0] = max(m[0], lookup_cached_sentence(src.row_ptr, src.rowT_ptr, src.status, src_len, S, Ts, cap_s, idx, j, T, cap).raw_len);
        block_reduce<1, REWRITE_THREADS, 1u>(m, scratch);
        if (t == 0) dst.status[B] = m[0];
    }
}

// The same assembly straight into the TOKEN-PACKED layout (what gcnpt_pack_trees makes of gcnpt_gather_trees' arrays, bit for bit): a
// sentence's offsets are prefix sums over the batch sentences before it, which every workgroup takes from the CACHE itself (lengths and
// offsets of the cached sentences are all there: no inter-workgroup hand-off as in the pruner's packed form).
__global__ __launch_bounds__(REWRITE_THREADS) void gather_trees_packed_kernel(const TreeSrc src, const int32_t* __restrict__ src_len,
                                                                             int S, int Ts, int cap_s, const int64_t* __restrict__ idx,
                                                                             int B, int T, const PackedDst dst, const PackParams pk,
                                                                             int pk_dtype) {
    __shared__ int scratch[REWRITE_THREADS / WAVE][4];
    if ((int)blockIdx.x >= B) {
        pack_side_job(pk, pk_dtype, B);
        return;
    }
    const int b = blockIdx.x, t = threadIdx.x;
    int a[4] = {0, 0, 0, 0};                                        // rows, entries, transposed entries before b; longest sentence
    for (int j = t; j < B; j += REWRITE_THREADS) {
        const CachedSentence c = lookup_cached_sentence(src.row_ptr, src.rowT_ptr, src.status, src_len, S, Ts, cap_s, idx, j, T, 3 * T);
        if (j < b) { a[0] += c.len; a[1] += c.nnz; a[2] += c.nnzT; }
        a[3] = max(a[3], c.raw_len);
    }
    block_reduce<4, REWRITE_THREADS, 1u << 3>(a, scratch);
    const CachedSentence c = lookup_cached_sentence(src.row_ptr, src.rowT_ptr, src.status, src_len, S, Ts, cap_s, idx, b, T, 3 * T);
    const bool ok = c.code == 0;
    // the padded layout's share: the per-sentence codes and the mask GCN.forward returns
    if (t == 0) {
        dst.sent_status[b] = c.code;
        if (b == 0) dst.sent_status[B] = a[3];
    }
    if (dst.pool_mask_padded)
        for (int i = t; i < T; i += REWRITE_THREADS)
            dst.pool_mask_padded[(size_t)b * T + i] = (ok && i < Ts) ? src.pool_mask[c.s * Ts + i] : (uint8_t)1;
    const SentenceSrc sent{c.s * (Ts + 1), (int)c.s * cap_s, (int)c.s * cap_s, c.s * Ts, c.len, c.nnz, c.nnzT, ok};
    write_packed_sentence<REWRITE_THREADS>(src, sent, b, B, a[0], a[1], a[2], dst);
}

// "Pooled-only" rows (gcn.py:116-121 pools h over the tokens of the pruned tree only, and a tree token's row of
// every layer depends on tree tokens only -- the adjacency has no entry outside the tree).  The kept tokens of a sentence
// are renumbered 0..kept-1 in token order and the pattern is rewritten in those numbers for a [B, Tc] batch: the layer
// kernels then run on B*Tc rows instead of B*T (a pruned tree keeps ~1 token in 4-8), with identical values in every
// kept row.  One workgroup per sentence; slot numbers of the sentence's tokens live in LDS.
__global__ __launch_bounds__(REWRITE_THREADS) void compact_trees_kernel(const TreeSrc src, int B, int T, int cap, int Tc, int cap_c,
                                                                       const TreeArrays dst, int64_t* __restrict__ tok,
                                                                       int32_t* __restrict__ kept_out) {
    extern __shared__ int c_slot[];                      // [T] slot of token i, or -1
    __shared__ int s_wave[REWRITE_THREADS / WAVE];
    __shared__ int s_base;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) s_base = 0;
    __syncthreads();
    // exclusive scan of the in-tree flags, 256 tokens per round
    for (int i0 = 0; i0 < T; i0 += REWRITE_THREADS) {
        const int i = i0 + t;
        const bool in = i < T && src.pool_mask[(size_t)b * T + i] == 0;
        const unsigned long long m = __ballot(in);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = s_base;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (i < T) c_slot[i] = in ? before + __popcll(m & ((1ull << lane) - 1ull)) : -1;
        __syncthreads();
        if (t == 0) {
            int tot = s_base;
            for (int w = 0; w < REWRITE_THREADS / WAVE; ++w) tot += s_wave[w];
            s_base = tot;
        }
        __syncthreads();
    }
    const int kept = s_base;
    const int nnz = src.row_ptr[(size_t)b * (T + 1) + T] - b * cap;
    const int nnzT = src.rowT_ptr ? src.rowT_ptr[(size_t)b * (T + 1) + T] - b * cap : 0;
    int code = src.status[b];
    if (code == 0 && kept > Tc) code = GCNPT_E_LENGTH;
    if (code == 0 && (nnz > cap_c || nnzT > cap_c)) code = GCNPT_E_CAPACITY;
    const bool ok = code == 0;
    if (t == 0) {
        dst.status[b] = code;
        kept_out[b] = ok ? kept : 0;
        if (ok) atomicMax(&dst.status[B], kept);
    }
    // slots past the kept tokens (or the whole sentence when it failed): no entries, excluded from pooling
    const int first_free = ok ? kept : 0;
    for (int j = first_free + t; j <= Tc; j += REWRITE_THREADS) {
        dst.row_ptr[(size_t)b * (Tc + 1) + j] = b * cap_c + (ok ? nnz : 0);
        if (dst.rowT_ptr) dst.rowT_ptr[(size_t)b * (Tc + 1) + j] = b * cap_c + (ok ? nnzT : 0);
        if (j < Tc) {
            tok[(size_t)b * Tc + j] = -1;
            dst.pool_mask[(size_t)b * Tc + j] = 1;
            zero_ell_head((size_t)b * Tc + j, dst.ell, dst.ellT);
        }
    }
    if (!ok) return;
    auto renumber_head = [&](const int32_t* in, int32_t* out) {       // [count, 7 columns] -> the same in slot numbers
        const int n = in[0];
        out[0] = n;
#pragma unroll
        for (int k = 1; k < 8; ++k) out[k] = k <= n ? c_slot[min(max(in[k], 0), T - 1)] : 0;
    };
    for (int i = t; i < T; i += REWRITE_THREADS) {
        const int j = c_slot[i];
        if (j < 0) continue;
        tok[(size_t)b * Tc + j] = i;
        dst.pool_mask[(size_t)b * Tc + j] = 0;
        dst.row_ptr[(size_t)b * (Tc + 1) + j] = b * cap_c + src.row_ptr[(size_t)b * (T + 1) + i] - b * cap;
        renumber_head(src.ell + ((size_t)b * T + i) * 8, dst.ell + ((size_t)b * Tc + j) * 8);
        if (dst.rowT_ptr) {
            dst.rowT_ptr[(size_t)b * (Tc + 1) + j] = b * cap_c + src.rowT_ptr[(size_t)b * (T + 1) + i] - b * cap;
            renumber_head(src.ellT + ((size_t)b * T + i) * 8, dst.ellT + ((size_t)b * Tc + j) * 8);
        }
    }
    for (int k = t; k < nnz; k += REWRITE_THREADS) {
        dst.col_idx[(size_t)b * cap_c + k] = c_slot[min(max(src.col_idx[(size_t)b * cap + k], 0), T - 1)];
        if (dst.label) dst.label[(size_t)b * cap_c + k] = src.label[(size_t)b * cap + k];
    }
    if (dst.colT_idx)
        for (int k = t; k < nnzT; k += REWRITE_THREADS)
            dst.colT_idx[(size_t)b * cap_c + k] = c_slot[min(max(src.colT_idx[(size_t)b * cap + k], 0), T - 1)];
}

// What gcnpt_prune_to_csr / gcnpt_gather_trees produced for [B, T], token-packed.  One workgroup per sentence: its row offset cu[b] and
// entry offsets are prefix sums over the sentences before it (B is a few hundred at most: every workgroup sums for itself, no second
// pass).
__global__ __launch_bounds__(REWRITE_THREADS) void pack_trees_kernel(const TreeSrc src, const int32_t* __restrict__ len, int B, int T,
                                                                    const PackedDst dst) {
    __shared__ int scratch[REWRITE_THREADS / WAVE][3];
    const int b = blockIdx.x;
    auto sentence = [&](int j) {
        SentenceSrc s;
        s.row = (size_t)j * (T + 1);
        s.tok = (size_t)j * T;
        s.len = min(len[j], T);
        s.rp0 = src.row_ptr[s.row];
        s.nnz = src.row_ptr[s.row + T] - s.rp0;
        s.rpT0 = 0; s.nnzT = 0;
        if (src.rowT_ptr) {                                         // (one branch: both loads leave with the ones above)
            s.rpT0 = src.rowT_ptr[s.row];
            s.nnzT = src.rowT_ptr[s.row + T] - s.rpT0;
        }
        s.ok = true;
        return s;
    };
    int pre[3] = {0, 0, 0};                                         // rows, entries, transposed entries before b
    for (int j = threadIdx.x; j < b; j += REWRITE_THREADS) {
        const SentenceSrc s = sentence(j);
        pre[0] += s.len; pre[1] += s.nnz; pre[2] += s.nnzT;
    }
    block_reduce<3, REWRITE_THREADS>(pre, scratch);
    write_packed_sentence<REWRITE_THREADS>(src, sentence(b), b, B, pre[0], pre[1], pre[2], dst);
}

// what a rewrite of a batch's arrays (gather / pack / compact) may ask of its source: labels, the transposed pattern (all or nothing) and
// the pool mask only where the source holds them; what: the entry point, for the messages
int check_request(const char* what, const int32_t* src_label, const int32_t* src_rowT_ptr, const int32_t* src_colT_idx,
                  const int32_t* src_ellT, const uint8_t* src_pool_mask, const int32_t* label, const int32_t* rowT_ptr,
                  const int32_t* colT_idx, const int32_t* ellT, const uint8_t* pool_mask) {
    GCNPT_REQUIRE(!label || src_label, "%s: labels wanted but the source holds none", what);
    const int rc = check_transposed(what, rowT_ptr, colT_idx, ellT);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(!rowT_ptr || (src_rowT_ptr && src_colT_idx && src_ellT), "%s: transposed pattern wanted but the source holds none", what);
    GCNPT_REQUIRE(!pool_mask || src_pool_mask, "%s: pool mask wanted but the source holds none", what);
    return GCNPT_OK;
}

int side_job(SideJob& sj, bool optional, int threads, int n_layers, const float* const* W, const int* H, const int* Din, int dtype,
             void* const* w_fwd, void* const* w_bwd) {
    sj = SideJob{};
    sj.dtype = dtype;
    if (optional && n_layers <= 0) return GCNPT_OK;
    const int rc = fill_pack_params(sj.pk, n_layers, W, H, Din, dtype, w_fwd, w_bwd);
    if (rc != GCNPT_OK) return rc;
    sj.blocks = (int)std::min<long long>(192, (sj.pk.first[n_layers] + threads - 1) / threads);
    return GCNPT_OK;
}

}  // namespace gcnpt

using namespace gcnpt;

static int gather_impl(void* stream, const int32_t* src_row_ptr, const int32_t* src_col_idx, const int32_t* src_label,
                       const int32_t* src_rowT_ptr, const int32_t* src_colT_idx, const int32_t* src_ell,
                       const int32_t* src_ellT, const uint8_t* src_pool_mask, const int32_t* src_status,
                       const int32_t* src_len, int S, int Ts, int cap_s, const int64_t* idx, int B, int T, int cap,
                       int32_t* row_ptr, int32_t* col_idx, int32_t* label, int32_t* rowT_ptr, int32_t* colT_idx,
                       int32_t* ell, int32_t* ellT, uint8_t* pool_mask, int32_t* status, const SideJob& sj) {
    GCNPT_REQUIRE(src_row_ptr && src_col_idx && src_ell && src_status && src_len && idx, "gather_trees: null cache pointer");
    GCNPT_REQUIRE(row_ptr && col_idx && ell && status, "gather_trees: null output pointer");
    GCNPT_REQUIRE(S > 0 && Ts > 0 && cap_s > 0 && B > 0 && T > 0 && cap > 0, "gather_trees: sizes must be positive");
    const int rc = check_request("gather_trees", src_label, src_rowT_ptr, src_colT_idx, src_ellT, src_pool_mask, label, rowT_ptr, colT_idx, ellT,
                                 pool_mask);
    if (rc != GCNPT_OK) return rc;
    if ((long long)B * cap > 0x7fffffffLL) return fail(GCNPT_E_UNSUPPORTED, "gather_trees: B*cap overflows int32");
    const TreeSrc src{src_row_ptr, src_col_idx, src_label, rowT_ptr ? src_rowT_ptr : nullptr, src_colT_idx, src_ell, src_ellT, src_pool_mask,
                      src_status};
    const TreeArrays dst{row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, status};
    hipLaunchKernelGGL(gather_trees_kernel, dim3(B + sj.blocks), dim3(REWRITE_THREADS), 0, (hipStream_t)stream, src, src_len, S, Ts, cap_s, idx,
                       B, T, cap, dst, sj.pk, sj.dtype);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_gather_trees(void* stream, const int32_t* src_row_ptr, const int32_t* src_col_idx, const int32_t* src_label,
                                  const int32_t* src_rowT_ptr, const int32_t* src_colT_idx, const int32_t* src_ell,
                                  const int32_t* src_ellT, const uint8_t* src_pool_mask, const int32_t* src_status,
                                  const int32_t* src_len, int S, int Ts, int cap_s, const int64_t* idx, int B, int T, int cap,
                                  int32_t* row_ptr, int32_t* col_idx, int32_t* label, int32_t* rowT_ptr, int32_t* colT_idx,
                                  int32_t* ell, int32_t* ellT, uint8_t* pool_mask, int32_t* status) {
    return gather_impl(stream, src_row_ptr, src_col_idx, src_label, src_rowT_ptr, src_colT_idx, src_ell, src_ellT, src_pool_mask, src_status,
                       src_len, S, Ts, cap_s, idx, B, T, cap, row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, status,
                       SideJob{});
}

extern "C" int gcnpt_gather_trees_pack(void* stream, const int32_t* src_row_ptr, const int32_t* src_col_idx, const int32_t* src_label,
                                       const int32_t* src_rowT_ptr, const int32_t* src_colT_idx, const int32_t* src_ell,
                                       const int32_t* src_ellT, const uint8_t* src_pool_mask, const int32_t* src_status,
                                       const int32_t* src_len, int S, int Ts, int cap_s, const int64_t* idx, int B, int T, int cap,
                                       int32_t* row_ptr, int32_t* col_idx, int32_t* label, int32_t* rowT_ptr, int32_t* colT_idx,
                                       int32_t* ell, int32_t* ellT, uint8_t* pool_mask, int32_t* status, int n_layers,
                                       const float* const* W, const int* H, const int* Din, int dtype, void* const* w_fwd,
                                       void* const* w_bwd) {
    SideJob sj;
    const int rc = side_job(sj, false, REWRITE_THREADS, n_layers, W, H, Din, dtype, w_fwd, w_bwd);
    if (rc != GCNPT_OK) return rc;
    return gather_impl(stream, src_row_ptr, src_col_idx, src_label, src_rowT_ptr, src_colT_idx, src_ell, src_ellT, src_pool_mask, src_status,
                       src_len, S, Ts, cap_s, idx, B, T, cap, row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, status, sj);
}

extern "C" int gcnpt_gather_trees_packed(void* stream, const int32_t* src_row_ptr, const int32_t* src_col_idx, const int32_t* src_label,
                                        const int32_t* src_rowT_ptr, const int32_t* src_colT_idx, const int32_t* src_ell,
                                        const int32_t* src_ellT, const uint8_t* src_pool_mask, const int32_t* src_status,
                                        const int32_t* src_len, int S, int Ts, int cap_s, const int64_t* idx, int B, int T,
                                        int32_t* cu_seqlens, int32_t* row_ptr, int32_t* col_idx, int32_t* label, int32_t* rowT_ptr,
                                        int32_t* colT_idx, int32_t* ell, int32_t* ellT, uint8_t* pool_mask, int32_t* row_sent, int n_rows,
                                        int nnz_cap, int32_t* status, int32_t* sent_status, uint8_t* pool_mask_padded, int n_layers,
                                        const float* const* W, const int* H, const int* Din, int dtype, void* const* w_fwd,
                                        void* const* w_bwd) {
    GCNPT_REQUIRE(src_row_ptr && src_col_idx && src_ell && src_status && src_len && src_pool_mask && idx, "gather_trees_packed: null cache pointer");
    GCNPT_REQUIRE(cu_seqlens && row_ptr && col_idx && ell && pool_mask && row_sent && status && sent_status, "gather_trees_packed: null output pointer");
    GCNPT_REQUIRE(S > 0 && Ts > 0 && cap_s > 0 && B > 0 && T > 0 && n_rows > 0 && nnz_cap > 0, "gather_trees_packed: sizes must be positive");
    int rc = check_request("gather_trees_packed", src_label, src_rowT_ptr, src_colT_idx, src_ellT, src_pool_mask, label, rowT_ptr, colT_idx, ellT,
                           pool_mask);
    if (rc != GCNPT_OK) return rc;
    SideJob sj;
    rc = side_job(sj, true, REWRITE_THREADS, n_layers, W, H, Din, dtype, w_fwd, w_bwd);
    if (rc != GCNPT_OK) return rc;
    const TreeSrc src{src_row_ptr, src_col_idx, src_label, rowT_ptr ? src_rowT_ptr : nullptr, src_colT_idx, src_ell, src_ellT, src_pool_mask,
                      src_status};
    const PackedDst dst{cu_seqlens, row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, row_sent, status, n_rows, nnz_cap,
                        pool_mask_padded, sent_status};
    hipLaunchKernelGGL(gather_trees_packed_kernel, dim3(B + sj.blocks), dim3(REWRITE_THREADS), 0, (hipStream_t)stream, src, src_len, S, Ts, cap_s, idx,
                       B, T, dst, sj.pk, sj.dtype);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_compact_trees(void* stream, const int32_t* src_row_ptr, const int32_t* src_col_idx, const int32_t* src_label,
                                   const int32_t* src_rowT_ptr, const int32_t* src_colT_idx, const int32_t* src_ell,
                                   const int32_t* src_ellT, const uint8_t* src_pool_mask, const int32_t* src_status, int B, int T,
                                   int cap, int Tc, int cap_c, int32_t* row_ptr, int32_t* col_idx, int32_t* label,
                                   int32_t* rowT_ptr, int32_t* colT_idx, int32_t* ell, int32_t* ellT, uint8_t* pool_mask,
                                   int32_t* status, int64_t* tok, int32_t* kept) {
    GCNPT_REQUIRE(src_row_ptr && src_col_idx && src_ell && src_pool_mask && src_status, "compact_trees: null source pointer");
    GCNPT_REQUIRE(row_ptr && col_idx && ell && pool_mask && status && tok && kept, "compact_trees: null output pointer");
    GCNPT_REQUIRE(B > 0 && T > 0 && cap > 0 && Tc > 0 && cap_c > 0, "compact_trees: sizes must be positive");
    const int rc = check_request("compact_trees", src_label, src_rowT_ptr, src_colT_idx, src_ellT, src_pool_mask, label, rowT_ptr, colT_idx, ellT,
                                 pool_mask);
    if (rc != GCNPT_OK) return rc;
    if ((long long)B * cap_c > 0x7fffffffLL) return fail(GCNPT_E_UNSUPPORTED, "compact_trees: B*cap_c overflows int32");
    const size_t lds = sizeof(int) * (size_t)T;
    if (lds > 60 * 1024) return fail(GCNPT_E_UNSUPPORTED, "compact_trees: T=%d exceeds the %d tokens a sentence may have", T, 60 * 1024 / 4);
    const TreeSrc src{src_row_ptr, src_col_idx, src_label, rowT_ptr ? src_rowT_ptr : nullptr, src_colT_idx, src_ell, src_ellT, src_pool_mask,
                      src_status};
    const TreeArrays dst{row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, status};
    hipStream_t s = (hipStream_t)stream;
    GCNPT_HIP_CHECK(hipMemsetAsync(status + B, 0, sizeof(int32_t), s));         // status[B] = most kept tokens in a sentence (atomicMax)
    hipLaunchKernelGGL(compact_trees_kernel, dim3(B), dim3(REWRITE_THREADS), lds, s, src, B, T, cap, Tc, cap_c, dst, tok, kept);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

// No memset in front of the launch: the last sentence writes both status words (write_packed_sentence).
extern "C" int gcnpt_pack_trees(void* stream, const int32_t* src_row_ptr, const int32_t* src_col_idx, const int32_t* src_label,
                                const int32_t* src_rowT_ptr, const int32_t* src_colT_idx, const int32_t* src_ell, const int32_t* src_ellT,
                                const uint8_t* src_pool_mask, const int32_t* len, int B, int T, int cap, int32_t* cu_seqlens,
                                int32_t* row_ptr, int32_t* col_idx, int32_t* label, int32_t* rowT_ptr, int32_t* colT_idx, int32_t* ell,
                                int32_t* ellT, uint8_t* pool_mask, int32_t* row_sent, int n_rows, int nnz_cap, int32_t* status) {
    GCNPT_REQUIRE(src_row_ptr && src_col_idx && src_ell && src_pool_mask && len, "pack_trees: null source pointer");
    GCNPT_REQUIRE(cu_seqlens && row_ptr && col_idx && ell && pool_mask && row_sent && status, "pack_trees: null destination pointer");
    GCNPT_REQUIRE(B > 0 && T > 0 && cap > 0 && n_rows > 0 && nnz_cap > 0, "pack_trees: sizes must be positive");
    const int rc = check_request("pack_trees", src_label, src_rowT_ptr, src_colT_idx, src_ellT, src_pool_mask, label, rowT_ptr, colT_idx, ellT,
                                 pool_mask);
    if (rc != GCNPT_OK) return rc;
    const TreeSrc src{src_row_ptr, src_col_idx, src_label, src_rowT_ptr, src_colT_idx, src_ell, src_ellT, src_pool_mask, nullptr};
    const PackedDst dst{cu_seqlens, row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, row_sent, status, n_rows, nnz_cap,
                        nullptr, nullptr};
    hipLaunchKernelGGL(pack_trees_kernel, dim3(B), dim3(REWRITE_THREADS), 0, (hipStream_t)stream, src, len, B, T, dst);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}
