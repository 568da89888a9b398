// The two layouts of a batch's tree arrays (include/gcnpt.h) as the pruner (tree_kernels.hip) and the rewrite kernels of
// tree_rewrite_kernels.hip see them, and the ONE copy of each rule they share: the header of a packed sentence, how a source sentence
// becomes a sentence of the token-packed layout, how an ELL head is shifted or left empty, how a cached sentence is looked up, the
// workgroup reduction behind their offsets, and the host check that the transposed arrays come together.  Whichever producer wrote a
// layout, the arrays are the same bit for bit (tests/test_gpu_packed.py, tests/test_gpu_parity.py).
#pragma once
#include "gcnpt_common.h"

namespace gcnpt {

typedef int i32x4_t __attribute__((ext_vector_type(4)));       // (a first-class vector: a select between int4 STRUCTS went through scratch memory)

// a padded batch [B, T] that a rewrite only reads (rowT_ptr: NULL unless the transposed pattern is wanted -- the gathers and the compaction
// count a sentence's transposed entries from it; status: NULL where the entry point takes none)
struct TreeSrc {
    const int32_t *row_ptr, *col_idx, *label, *rowT_ptr, *colT_idx, *ell, *ellT;
    const uint8_t* pool_mask;
    const int32_t* status;
};
// a padded batch that a rewrite writes
struct TreeArrays {
    int32_t *row_ptr, *col_idx, *label, *rowT_ptr, *colT_idx, *ell, *ellT;
    uint8_t* pool_mask;
    int32_t* status;
};
// a token-packed batch.  The rewrites write it only through write_packed_sentence(), but for the two arrays of the PADDED layout that
// come with it when a cache or the parse is the source (NULL otherwise), which gather_trees_packed_kernel fills itself.  The pruner
// writes every member itself (tree_kernels.hip: emit_rows), the header through write_packed_header(); it is also its destination for
// the padded layout: cu == NULL, the arrays a TreeArrays' with pool_mask_padded as its mask and sent_status as its status, the members
// of the packed layout alone unused.
struct PackedDst {
    int32_t *cu, *row_ptr, *col_idx, *label, *rowT_ptr, *colT_idx, *ell, *ellT;
    uint8_t* pool_mask;
    int32_t *row_sent, *status;      // status[2]: 0 / GCNPT_E_CAPACITY, sum(len)
    int n_rows, nnz_cap;
    uint8_t* pool_mask_padded;       // NULL or [B*T]
    int32_t* sent_status;            // NULL or [B+1]
};

// where one sentence of a TreeSrc starts, and what it contributes to a packed batch
struct SentenceSrc {
    size_t row;              // its row 0 in row_ptr / rowT_ptr
    int rp0, rpT0;           // what those offsets count from: its first entry in col_idx / label, and in colT_idx
    size_t tok;              // its first token slot: pool_mask[tok], ELL heads from word tok * 8
    int len, nnz, nnzT;      // rows, entries, transposed entries
    bool ok;                 // false: an empty, fully masked sentence (len rows, no entries), as the pruner leaves a failed one
};

// Sums of N per-thread values over the workgroup (maxima where bit q of MAX_MASK is set): shuffle-reduce per wave, meet in LDS, every
// thread reads the totals.  One barrier; `scratch` must not be reused before the next one.
template <int N, int THREADS, unsigned MAX_MASK = 0>
__device__ __forceinline__ void block_reduce(int (&v)[N], int (*scratch)[N]) {
    auto join = [](int q, int x, int y) { return (MAX_MASK >> q & 1) ? max(x, y) : x + y; };
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = join(q, v[q], __shfl_xor(v[q], d));
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) scratch[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = scratch[0][q];
#pragma unroll
    for (int w = 1; w < THREADS / WAVE; ++w)
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = join(q, v[q], scratch[w][q]);
}

// rowT_ptr, colT_idx and ellT of a destination: all three or none (host; what: the entry point, for the message)
inline int check_transposed(const char* what, const void* rowT_ptr, const void* colT_idx, const void* ellT) {
    GCNPT_REQUIRE((rowT_ptr == nullptr) == (colT_idx == nullptr) && (rowT_ptr == nullptr) == (ellT == nullptr),
                  "%s: rowT_ptr, colT_idx and ellT go together", what);
    return GCNPT_OK;
}

// The ELL head of a row without entries, in both patterns (ellT: NULL or the transposed heads): count 0, zeros in the slots.
__device__ __forceinline__ void zero_ell_head(size_t row, int32_t* ell, int32_t* ellT) {
    const i32x4_t z = {0, 0, 0, 0};
    reinterpret_cast<i32x4_t*>(ell + row * 8)[0] = z; reinterpret_cast<i32x4_t*>(ell + row * 8)[1] = z;
    if (ellT) { reinterpret_cast<i32x4_t*>(ellT + row * 8)[0] = z; reinterpret_cast<i32x4_t*>(ellT + row * 8)[1] = z; }
}

// One 16-byte half of a row's ELL head ([count, c0..c2] / [c3..c6]) into the packed layout: cu added to the live slots, zeros in the
// others.  head_src / head_dst: the row's 8 words; !ok: an all-zero head, nothing is read.
__device__ __forceinline__ void shift_ell_half(const int32_t* head_src, int32_t* head_dst, int half, bool ok, int cu) {
    const int cnt = ok ? head_src[0] : 0;
    i32x4_t v = ok ? reinterpret_cast<const i32x4_t*>(head_src)[half] : i32x4_t{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int slot = half * 4 + j - 1;                       // entry number of this word (-1 = the count)
        if (slot >= 0) v[j] = slot < cnt ? v[j] + cu : 0;
    }
    reinterpret_cast<i32x4_t*>(head_dst)[half] = v;
}

// The header of sentence b of a token-packed batch (len rows from cu, nnz / nnzT entries from eo / eoT), by thread 0; every thread gets
// whether the sentence fits the n_rows rows and nnz_cap entries of the destination, of which these are the cu, row_ptr, rowT_ptr and
// status: one that does not writes nothing but cu[b].  The last sentence writes the batch's totals and closing offsets: offsets grow
// with b, so it fits iff every sentence does.  (Values and pointers, not the PackedDst: see lookup_cached_sentence.)
__device__ __forceinline__ bool write_packed_header(int b, int B, int cu, int eo, int eoT, int len, int nnz, int nnzT, int32_t* cu_out,
                                                    int32_t* row_ptr, int32_t* rowT_ptr, int32_t* status, int n_rows, int nnz_cap) {
    const bool fits = cu + len <= n_rows && eo + nnz <= nnz_cap && eoT + nnzT <= nnz_cap;
    if (threadIdx.x == 0) {
        cu_out[b] = cu;
        if (b == B - 1) {
            cu_out[B] = cu + len;
            status[0] = fits ? 0 : GCNPT_E_CAPACITY;
            status[1] = cu + len;
            if (fits) {
                row_ptr[cu + len] = eo + nnz;
                if (rowT_ptr) rowT_ptr[cu + len] = eoT + nnzT;
            }
        }
    }
    return fits;
}

// Sentence b of a token-packed batch (layout: gcnpt_pack_trees in include/gcnpt.h), by all THREADS of a workgroup: rows from cu,
// entries from eo / eoT (the sums of len, nnz, nnzT over the sentences before it); columns and live ELL slots shifted by cu.
template <int THREADS>
__device__ __forceinline__ void write_packed_sentence(const TreeSrc& src, const SentenceSrc& s, int b, int B, int cu, int eo, int eoT,
                                                      const PackedDst& dst) {
    const int t = threadIdx.x;
    if (!write_packed_header(b, B, cu, eo, eoT, s.len, s.nnz, s.nnzT, dst.cu, dst.row_ptr, dst.rowT_ptr, dst.status, dst.n_rows, dst.nnz_cap))
        return;
    for (int i = t; i < s.len; i += THREADS) {
        dst.row_ptr[cu + i] = eo + (s.ok ? src.row_ptr[s.row + i] - s.rp0 : 0);
        if (dst.rowT_ptr) dst.rowT_ptr[cu + i] = eoT + (s.ok ? src.rowT_ptr[s.row + i] - s.rpT0 : 0);
        dst.pool_mask[cu + i] = s.ok ? src.pool_mask[s.tok + i] : (uint8_t)1;
        dst.row_sent[cu + i] = b;
    }
    for (int k = t; k < s.nnz; k += THREADS) {
        dst.col_idx[eo + k] = src.col_idx[(size_t)s.rp0 + k] + cu;
        if (dst.label) dst.label[eo + k] = src.label[(size_t)s.rp0 + k];
    }
    if (dst.colT_idx)
        for (int k = t; k < s.nnzT; k += THREADS) dst.colT_idx[eoT + k] = src.colT_idx[(size_t)s.rpT0 + k] + cu;
    for (int q = t; q < 2 * s.len; q += THREADS) {                  // ELL heads, 16 bytes at a time
        const size_t from = (s.tok + (q >> 1)) * 8, to = (size_t)(cu + (q >> 1)) * 8;
        shift_ell_half(src.ell + from, dst.ell + to, q & 1, s.ok, cu);
        if (dst.ellT) shift_ell_half(src.ellT + from, dst.ellT + to, q & 1, s.ok, cu);
    }
}

// Sentence idx[j] of a cache (S sentences padded to Ts, capacity cap_s, lengths src_len; row_ptr / rowT_ptr / status of its TreeSrc) as
// sentence j of a batch padded to T whose sentences may hold cap_limit entries.  (The three pointers, not the TreeSrc: a kernel-argument
// struct whose address is taken, even by a call that is inlined, loses the scalar loads of what it points to -- DESIGN.md section 3.)  code != 0: the sentence is not there (E_INVALID), failed when the cache was built, is longer
// than T (E_LENGTH) or holds too many entries (E_CAPACITY); it then contributes its rows and no entries.
struct CachedSentence {
    size_t s;                // its number in the cache (0 when idx[j] is out of range)
    int raw_len, len;        // its length, and that clamped to T
    int nnz, nnzT, code;
};
__device__ __forceinline__ CachedSentence lookup_cached_sentence(const int32_t* row_ptr, const int32_t* rowT_ptr, const int32_t* status,
                                                                 const int32_t* __restrict__ src_len, int S, int Ts, int cap_s,
                                                                 const int64_t* __restrict__ idx, int j, int T, int cap_limit) {
    CachedSentence c;
    const int64_t s64 = idx[j];
    const bool known = s64 >= 0 && s64 < S;
    c.s = known ? (size_t)s64 : 0;
    c.raw_len = known ? src_len[c.s] : 0;
    c.len = min(c.raw_len, T);
    c.nnz = row_ptr[c.s * (Ts + 1) + Ts] - (int)c.s * cap_s;
    c.nnzT = rowT_ptr ? rowT_ptr[c.s * (Ts + 1) + Ts] - (int)c.s * cap_s : 0;
    c.code = known ? status[c.s] : GCNPT_E_INVALID;
    if (c.code == 0 && c.raw_len > T) c.code = GCNPT_E_LENGTH;
    if (c.code == 0 && (c.nnz > cap_limit || c.nnzT > cap_limit)) c.code = GCNPT_E_CAPACITY;
    if (c.code != 0) { c.nnz = 0; c.nnzT = 0; }
    return c;
}

}  // namespace gcnpt
