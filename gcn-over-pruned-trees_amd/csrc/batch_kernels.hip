// The loader's batch assembly (reference data/loader.py:81-141) for gfx950: the dataset's token arrays stay in HBM as int32 [S,Ts], and
// ONE launch writes the eight loader tensors, the labels and the lengths of a batch from them -- the other half of N4 (the trees of
// the batch come from gcnpt_gather_trees over the same sentence numbers).
//
//   id fields   field[b*T+t] = src_field[idx[b]*Ts+t] for t < len, the pad value behind it: PAD_ID (0) for words / pos / ner / deprel /
//               head (get_long_tensor, loader.py:167-174), pos_fill for subj_pos / obj_pos (150 in loader.py:120-121)
//   masks       t >= len.  The reference derives the mask as words == 0 (loader.py:110); the two agree on everything its loader
//               produces (a real token never has the id PAD_ID), and the length needs no second pass over the words
//   word dropout (loader.py:96-98, 182-186)  a real token whose id is not UNK_ID becomes UNK_ID when dropped; counter based like every
//               dropout here: one decision per BATCH SLOT, !drop_keep(drop_hash(seed + *seed_dev, b*T + t, 0), 0, thresh16), so a sentence
//               that sits in two slots is dropped independently and a replayed graph follows the device word
//
// One workgroup per sentence and chunk of 64 * VW tokens; wave w writes fields w and w + 4 of (words, pos, ner, deprel, head, subj_pos,
// obj_pos, masks), a lane VW consecutive tokens of them: 16-byte stores of int64 pairs with VW = 2 (even T, 16-byte aligned outputs), 8-byte
// stores with VW = 1.  Every output element has exactly one writer: no workspace, no memset, replayable.  idx[b], the length and the row
// bases are wave-uniform (scalar registers); no load sits behind a condition (a slot past the end re-reads the sentence's last token).
#include "layer_common.h"

namespace gcnpt {

constexpr int GB_THREADS = 256;
constexpr int UNK_ID = 1;          // utils/constant.py:10

struct BatchSrc { const int32_t *words, *pos, *ner, *deprel, *head, *subj_pos, *obj_pos; };
struct BatchDst { int64_t *words, *pos, *ner, *deprel, *head, *subj_pos, *obj_pos; };

typedef long long i64x2_t __attribute__((ext_vector_type(2)));

// VW tokens of one id field from slot t0 of batch row `out`; `in`: the cached sentence's row (n tokens, n <= Ts; in[0] is readable
// even when n == 0).  thresh16 != 0: the word field, `key` = b*T + t0
template <int VW>
__device__ __forceinline__ void gather_ids(const int32_t* __restrict__ in, int64_t* __restrict__ out, int t0, int n, long long fill,
                                           unsigned thresh16, uint64_t seed, unsigned key) {
    long long v[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) {
        const int t = t0 + j;
        const int w = in[min(t, max(n - 1, 0))];
        const bool drop = thresh16 != 0 && w != UNK_ID && !drop_keep(drop_hash(seed, key + (unsigned)j, 0u), 0u, thresh16);
        v[j] = t < n ? (long long)(drop ? UNK_ID : w) : fill;
    }
    if constexpr (VW == 2) *reinterpret_cast<i64x2_t*>(out + t0) = i64x2_t{v[0], v[1]};
    else out[t0] = v[0];
}

template <int VW>
__global__ __launch_bounds__(GB_THREADS) void gather_batch_kernel(const BatchSrc src, const int32_t* __restrict__ src_len,
                                                                  const int32_t* __restrict__ src_label, int S, int Ts,
                                                                  const int64_t* __restrict__ idx, int T, const BatchDst dst,
                                                                  uint8_t* __restrict__ masks, int64_t* __restrict__ labels,
                                                                  int32_t* __restrict__ lens, int32_t* __restrict__ status,
                                                                  long long pos_fill, unsigned thresh16, uint64_t seed,
                                                                  const uint64_t* __restrict__ seed_dev) {
    const int b = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), lane = threadIdx.x % WAVE;
    // the cached sentence: the codes gcnpt_gather_trees gives (lookup_cached_sentence of tree_layout.h), an empty row for a failing one
    const int64_t s64 = idx[b];
    const bool known = s64 >= 0 && s64 < S;
    const size_t s = known ? (size_t)s64 : 0;
    const int raw_len = src_len[s], label = src_label[s];
    const int code = !known ? GCNPT_E_INVALID : ((raw_len > T || raw_len > Ts) ? GCNPT_E_LENGTH : 0);
    const int n = code == 0 ? max(raw_len, 0) : 0;
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        labels[b] = code == 0 ? (int64_t)label : 0;
        if (lens) lens[b] = n;
        if (status) status[b] = code;
    }
    const int t0 = ((int)blockIdx.y * WAVE + lane) * VW;
    if (t0 >= T) return;                                               // (VW = 2: T is even, so t0 + 1 < T too)
    const size_t from = s * (size_t)Ts, to = (size_t)b * T;
    const uint64_t sd = seed + (seed_dev ? *seed_dev : 0ull);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int f = wave + 4 * k;                                    // wave-uniform: the selects below are scalar
        if (f == 7) {
            if constexpr (VW == 2)
                *reinterpret_cast<unsigned short*>(masks + to + t0) = (unsigned short)((t0 >= n ? 1u : 0u) | (t0 + 1 >= n ? 0x100u : 0u));
            else
                masks[to + t0] = t0 >= n ? 1 : 0;
            continue;
        }
        const int32_t* in = f == 0 ? src.words : f == 1 ? src.pos : f == 2 ? src.ner : f == 3 ? src.deprel : f == 4 ? src.head
                          : f == 5 ? src.subj_pos : src.obj_pos;
        int64_t* out = f == 0 ? dst.words : f == 1 ? dst.pos : f == 2 ? dst.ner : f == 3 ? dst.deprel : f == 4 ? dst.head
                     : f == 5 ? dst.subj_pos : dst.obj_pos;
        if (!in) continue;                                             // no NER field (SemEval)
        gather_ids<VW>(in + from, out + to, t0, n, f >= 5 ? pos_fill : 0ll, f == 0 ? thresh16 : 0u, sd, (unsigned)(to + t0));
    }
}

}  // namespace gcnpt

using namespace gcnpt;

extern "C" int gcnpt_gather_batch(void* stream, const int32_t* src_words, const int32_t* src_pos, const int32_t* src_ner,
                                  const int32_t* src_deprel, const int32_t* src_head, const int32_t* src_subj_pos,
                                  const int32_t* src_obj_pos, const int32_t* src_len, const int32_t* src_label, int S, int Ts,
                                  const int64_t* idx, int B, int T, int64_t* words, uint8_t* masks, int64_t* pos, int64_t* ner,
                                  int64_t* deprel, int64_t* head, int64_t* subj_pos, int64_t* obj_pos, int64_t* labels, int32_t* lens,
                                  int32_t* status, int64_t pos_fill, float p_word, uint64_t seed, const uint64_t* seed_dev) {
    GCNPT_REQUIRE(src_words && src_pos && src_deprel && src_head && src_subj_pos && src_obj_pos && src_len && src_label && idx,
                  "gcnpt_gather_batch: null source pointer");
    GCNPT_REQUIRE(words && masks && pos && deprel && head && subj_pos && obj_pos && labels, "gcnpt_gather_batch: null output pointer");
    GCNPT_REQUIRE((src_ner == nullptr) == (ner == nullptr), "gcnpt_gather_batch: src_ner and ner go together (both or neither)");
    GCNPT_REQUIRE(S > 0 && Ts > 0 && B > 0 && T > 0, "gcnpt_gather_batch: sizes must be positive");
    GCNPT_REQUIRE(p_word >= 0.0f && p_word < 1.0f, "gcnpt_gather_batch: the word dropout probability must be in [0, 1)");     // (NaN fails both)
    const int per_wg = WAVE * 2;
    if ((long long)B * T >= (1ll << 31) || ceil_div(T, WAVE) > 65535)
        return fail(GCNPT_E_UNSUPPORTED, "gcnpt_gather_batch: at most 2^31 token slots and %d tokens per sentence", 65535 * WAVE);
    auto aligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    const bool pairs = T % 2 == 0 && aligned(words, 16) && aligned(pos, 16) && aligned(ner, 16) && aligned(deprel, 16) && aligned(head, 16) &&
                       aligned(subj_pos, 16) && aligned(obj_pos, 16) && aligned(masks, 2);
    const BatchSrc src{src_words, src_pos, src_ner, src_deprel, src_head, src_subj_pos, src_obj_pos};
    const BatchDst dst{words, pos, ner, deprel, head, subj_pos, obj_pos};
    const unsigned thresh16 = (unsigned)((double)p_word * 65536.0);
    hipStream_t st = (hipStream_t)stream;
    if (pairs)
        hipLaunchKernelGGL(gather_batch_kernel<2>, dim3(B, ceil_div(T, per_wg)), dim3(GB_THREADS), 0, st, src, src_len, src_label, S, Ts, idx, T,
                           dst, masks, labels, lens, status, (long long)pos_fill, thresh16, seed, seed_dev);
    else
        hipLaunchKernelGGL(gather_batch_kernel<1>, dim3(B, ceil_div(T, WAVE)), dim3(GB_THREADS), 0, st, src, src_len, src_label, S, Ts, idx, T,
                           dst, masks, labels, lens, status, (long long)pos_fill, thresh16, seed, seed_dev);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}
