// The embedding front end of GCN.forward (reference model/gcn.py:235-241) for gfx950: one launch builds the layer stack's input, one
// launch takes its gradient apart.
//
// Forward: out[row] = in_drop([emb_drop(emb[words]) | pos_emb[pos] | ner_emb[ner]]) for every token -- three lookups, the cat, the
// word-type EmbeddingDropout (model/dropouts.py:23-39), nn.Dropout, the cast to bf16 and, with cu_seqlens, pack_rows, all in one pass.
// One wave per token row; a lane owns a column pair (all widths even, 8-byte aligned bases: C2's 300/30/30) or single columns (any widths).
//
// Dropout is counter based (drop_hash / drop_keep of layer_common.h), so the backward recomputes it and no mask is ever stored:
//   word type   one decision per (sentence b, word id): hash(seed_emb, b, id >> 1), half (id & 1) -- every occurrence of a word in a
//               sentence shares its fate, and no [B, V] Bernoulli matrix exists;
//   element     hash(seed_in, b*T + t, col >> 1), half (col & 1): keyed on the PADDED token number in both layouts, so the packed output
//               is pack_rows of the padded output bit for bit.
// Arithmetic: out = (v * s_emb) * s_in in fp32 (s = 1/(1-p) in float32; s_emb = 1 outside the word segment and for a dense word source),
// a dropped element is +0.0.
//
// Backward: one launch over g.  The word table's gradient is either dense -- fp32 atomic adds into [V,E0], one wave per token row and
// 64 consecutive columns (256 contiguous bytes) per wave-instruction -- or row sparse, plain stores into [B*T,E0].  No atomic is issued
// for a token whose id is the padding index, >= topn, out of range, or whose word type was dropped.  The POS / NER tables have a few
// dozen rows that thousands of tokens add into (every adder on a handful of rows: the slow shape for global atomics), so a workgroup
// sums its tokens in LDS and adds only the table rows it touched, once, at its end.
#include "layer_common.h"

namespace gcnpt {

constexpr int EM_THREADS = 256;
constexpr int EM_WAVES = EM_THREADS / WAVE;
constexpr int EM_FWD_TOK = 8;              // tokens of one sentence per forward workgroup
constexpr int EM_BWD_TOK = 32;             // ... per backward workgroup (what its LDS sums of the small tables cover)
constexpr size_t EM_LDS_MAX = 48 * 1024;   // small tables above this add straight into global memory

struct EmbArgs {
    const int64_t* words;      // [B*T] or NULL (dense word source)
    const int64_t* pos;        // [B*T] or NULL (E1 == 0)
    const int64_t* ner;        // [B*T] or NULL (E2 == 0)
    int V0, V1, V2, E0, E1, E2;
    const int32_t* cu;         // NULL = padded rows; else the packed layout's [B+1] offsets
    int B, T, n_rows;
    unsigned th_emb, th_in;    // 16-bit drop thresholds (0 = keep everything)
    float s_emb, s_in;
    uint64_t seed_emb, seed_in;
    const uint64_t* seed_dev;  // NULL or a device word added to both seeds
};

// one token of the batch as a wave sees it (everything here is wave-uniform)
struct EmbToken {
    unsigned n;        // padded token number b*T + t: the element dropout's row key
    size_t row;        // its row of the output / of g (clamped to a valid row when !present)
    bool present;      // the layout holds this token
    int id0, id1, id2;          // range-checked (0 when outside the table)
    bool live0, live1, live2;   // the segment is read / gets a gradient
    int bad;           // status bits of out-of-range ids
};

__device__ __forceinline__ EmbToken emb_token(const EmbArgs& a, int b, int t, int base, int len, uint64_t seed_emb) {
    EmbToken k;
    k.n = (unsigned)b * (unsigned)a.T + (unsigned)t;
    const long long r = a.cu ? (long long)base + t : (long long)k.n;
    k.present = t < len && r >= 0 && r < (long long)a.n_rows;
    k.row = k.present ? (size_t)r : 0;
    k.bad = 0;
    const long long w = a.words ? a.words[k.n] : 0, p = a.E1 > 0 ? a.pos[k.n] : 0, r2 = a.E2 > 0 ? a.ner[k.n] : 0;
    k.id0 = 0;
    k.live0 = true;
    if (a.words) {
        const bool ok = w >= 0 && w < a.V0;
        if (ok) k.id0 = (int)w; else k.bad |= 1;
        const unsigned id = (unsigned)k.id0;
        k.live0 = ok && drop_keep(drop_hash(seed_emb, (unsigned)b, id >> 1), id & 1u, a.th_emb);
    }
    k.live1 = a.E1 > 0 && p >= 0 && p < a.V1;
    k.id1 = k.live1 ? (int)p : 0;
    if (a.E1 > 0 && !k.live1) k.bad |= 2;
    k.live2 = a.E2 > 0 && r2 >= 0 && r2 < a.V2;
    k.id2 = k.live2 ? (int)r2 : 0;
    if (a.E2 > 0 && !k.live2) k.bad |= 4;
    return k;
}

template <typename OT> __device__ __forceinline__ void emb_store2(OT* p, float x, float y);
template <> __device__ __forceinline__ void emb_store2<float>(float* p, float x, float y) { *reinterpret_cast<float2*>(p) = make_float2(x, y); }
template <> __device__ __forceinline__ void emb_store2<bf16_t>(bf16_t* p, float x, float y) {
    *reinterpret_cast<unsigned*>(p) = (unsigned)f32_to_bf16(x) | ((unsigned)f32_to_bf16(y) << 16);
}

// VW = 2: a lane owns a column pair (E0, E1, E2 even; table, source and output bases 8-byte aligned); VW = 1: any widths
template <typename OT, int VW>
__global__ __launch_bounds__(EM_THREADS) void embed_fwd_kernel(EmbArgs a, const float* __restrict__ dense, const float* __restrict__ t0,
                                                                const float* __restrict__ t1, const float* __restrict__ t2,
                                                                OT* __restrict__ out, int32_t* status) {
    const int b = blockIdx.y, wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const uint64_t sd = a.seed_dev ? *a.seed_dev : 0ull;
    const uint64_t seed_emb = a.seed_emb + sd, seed_in = a.seed_in + sd;
    const int Din = a.E0 + a.E1 + a.E2;
    const int base = a.cu ? a.cu[b] : 0;
    const int len = a.cu ? min(a.cu[b + 1] - base, a.T) : a.T;
    for (int i = wave; i < EM_FWD_TOK; i += EM_WAVES) {
        const int t = blockIdx.x * EM_FWD_TOK + i;
        if (t >= a.T) break;
        const EmbToken k = emb_token(a, b, t, base, len, seed_emb);
        if (!k.present) continue;                                   // packed layout: slots past the sentence's end do not exist
        if (k.bad && status && lane == 0) atomicOr(status, k.bad);
        // a segment that is not live still reads row 0 of its table (valid memory) and is zeroed: no load sits behind a condition
        const float* p0 = a.words ? t0 + (size_t)k.id0 * a.E0 : dense + (size_t)k.n * a.E0;
        const float* p1 = a.E1 > 0 ? t1 + (size_t)k.id1 * a.E1 : p0;
        const float* p2 = a.E2 > 0 ? t2 + (size_t)k.id2 * a.E2 : p0;
        const float se0 = a.words ? a.s_emb : 1.0f;
        OT* o = out + k.row * (size_t)Din;
        for (int c = lane * VW; c < Din; c += WAVE * VW) {
            const bool w = c < a.E0, q = c < a.E0 + a.E1;
            const float* p = w ? p0 + c : (q ? p1 + (c - a.E0) : p2 + (c - a.E0 - a.E1));
            const bool live = w ? k.live0 : (q ? k.live1 : k.live2);
            const float se = w ? se0 : 1.0f;
            const unsigned h = drop_hash(seed_in, k.n, (unsigned)c >> 1);
            if constexpr (VW == 2) {
                const float2 v = *reinterpret_cast<const float2*>(p);
                const float x = (v.x * se) * a.s_in, y = (v.y * se) * a.s_in;
                emb_store2<OT>(o + c, live && drop_keep(h, 0u, a.th_in) ? x : 0.0f, live && drop_keep(h, 1u, a.th_in) ? y : 0.0f);
            } else {
                const float x = (*p * se) * a.s_in;
                io<OT>::store1(o + c, live && drop_keep(h, (unsigned)c, a.th_in) ? x : 0.0f);
            }
        }
    }
}

template <typename GT>
__global__ __launch_bounds__(EM_THREADS) void embed_bwd_kernel(EmbArgs a, const GT* __restrict__ g, int pad_idx, int topn,
                                                                float* d0, float* __restrict__ rows, float* __restrict__ ddense, float* d1,
                                                                float* d2, int use_lds) {
    extern __shared__ float em_lds[];        // [V1*E1] [V2*E2] sums, then int [V1] [V2] "row touched" flags
    const int b = blockIdx.y, wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int n1 = d1 ? a.V1 * a.E1 : 0, n2 = d2 ? a.V2 * a.E2 : 0;
    float* s1 = em_lds;
    float* s2 = em_lds + n1;
    int* touched = reinterpret_cast<int*>(em_lds + n1 + n2);
    if (use_lds) {
        for (int q = threadIdx.x; q < n1 + n2 + a.V1 + a.V2; q += EM_THREADS) em_lds[q] = 0.0f;     // (+0.0f is the zero bit pattern)
        __syncthreads();
    }
    const uint64_t sd = a.seed_dev ? *a.seed_dev : 0ull;
    const uint64_t seed_emb = a.seed_emb + sd, seed_in = a.seed_in + sd;
    const int Din = a.E0 + a.E1 + a.E2;
    const int base = a.cu ? a.cu[b] : 0;
    const int len = a.cu ? min(a.cu[b + 1] - base, a.T) : a.T;
    for (int i = wave; i < EM_BWD_TOK; i += EM_WAVES) {
        const int t = blockIdx.x * EM_BWD_TOK + i;
        if (t >= a.T) break;
        const EmbToken k = emb_token(a, b, t, base, len, seed_emb);
        // which tokens reach the word table: not the padding row, not the rows above topn (gcn.py:84-88), not a dropped word type
        const bool add0 = k.present && k.live0 && (!a.words || (k.id0 != pad_idx && k.id0 < topn));
        const bool add1 = k.present && k.live1 && d1, add2 = k.present && k.live2 && d2;
        const float se0 = a.words ? a.s_emb : 1.0f;
        const GT* gr = g + k.row * (size_t)Din;
        for (int c = lane; c < Din; c += WAVE) {       // 64 consecutive columns per wave-instruction: 256 contiguous bytes per atomic
            const float gv = io<GT>::load1(gr + c);
            const bool keep = drop_keep(drop_hash(seed_in, k.n, (unsigned)c >> 1), (unsigned)c, a.th_in);
            float x = keep ? gv * a.s_in : 0.0f;
            if (c < a.E0) {
                x = add0 ? x * se0 : 0.0f;
                if (d0) { if (add0) atomicAdd(d0 + (size_t)k.id0 * a.E0 + c, x); }
                else if (rows) rows[(size_t)k.n * a.E0 + c] = x;
                else if (ddense) ddense[(size_t)k.n * a.E0 + c] = x;
            } else if (c < a.E0 + a.E1) {
                const int q = k.id1 * a.E1 + (c - a.E0);
                if (add1) { if (use_lds) atomicAdd(s1 + q, x); else atomicAdd(d1 + q, x); }
            } else {
                const int q = k.id2 * a.E2 + (c - a.E0 - a.E1);
                if (add2) { if (use_lds) atomicAdd(s2 + q, x); else atomicAdd(d2 + q, x); }
            }
        }
        if (use_lds && lane == 0) {
            if (add1) touched[k.id1] = 1;
            if (add2) touched[a.V1 + k.id2] = 1;
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int q = threadIdx.x; q < n1; q += EM_THREADS)
            if (touched[q / a.E1]) atomicAdd(d1 + q, s1[q]);
        for (int q = threadIdx.x; q < n2; q += EM_THREADS)
            if (touched[a.V1 + q / a.E2]) atomicAdd(d2 + q, s2[q]);
    }
}

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// the checks both entry points share; fills `a`
static int embed_args(const char* what, EmbArgs& a, const int64_t* words, const int64_t* pos, const int64_t* ner, int V0, int V1, int V2,
                      int E0, int E1, int E2, const int32_t* cu, int B, int T, int n_rows, float p_emb, float p_in, uint64_t seed_emb,
                      uint64_t seed_in, const uint64_t* seed_dev) {
    GCNPT_REQUIRE(B > 0 && T > 0, "%s: B and T must be positive", what);
    GCNPT_REQUIRE(B <= 65535 && (long long)B * T < (1ll << 31), "%s: at most 65535 sentences and 2^31 tokens", what);
    GCNPT_REQUIRE(E0 > 0, "%s: the word segment must be at least 1 wide (E0 = %d)", what, E0);
    GCNPT_REQUIRE(E1 >= 0 && E2 >= 0 && (long long)E0 + E1 + E2 < (1 << 24), "%s: bad segment widths %d/%d/%d", what, E0, E1, E2);
    GCNPT_REQUIRE(!words || V0 > 0, "%s: the word table has no rows", what);
    GCNPT_REQUIRE(E1 == 0 || (pos && V1 > 0), "%s: null POS ids or empty table with E1 = %d", what, E1);
    GCNPT_REQUIRE(E2 == 0 || (ner && V2 > 0), "%s: null NER ids or empty table with E2 = %d", what, E2);
    GCNPT_REQUIRE((long long)V1 * E1 < (1 << 28) && (long long)V2 * E2 < (1 << 28), "%s: POS / NER tables too large", what);
    GCNPT_REQUIRE(!cu || n_rows > 0, "%s: a packed call needs n_rows > 0 (got %d)", what, n_rows);
    GCNPT_REQUIRE(p_emb >= 0.0f && p_emb < 1.0f && p_in >= 0.0f && p_in < 1.0f, "%s: dropout probabilities must be in [0, 1)", what);
    a.words = words; a.pos = E1 > 0 ? pos : nullptr; a.ner = E2 > 0 ? ner : nullptr;
    a.V0 = V0; a.V1 = V1; a.V2 = V2; a.E0 = E0; a.E1 = E1; a.E2 = E2;
    a.cu = cu; a.B = B; a.T = T;
    a.n_rows = cu ? n_rows : B * T;
    if (!words) p_emb = 0.0f;                                  // a dense word source has no word types to drop
    a.th_emb = (unsigned)((double)p_emb * 65536.0);
    a.th_in = (unsigned)((double)p_in * 65536.0);
    a.s_emb = 1.0f / (1.0f - p_emb);
    a.s_in = 1.0f / (1.0f - p_in);
    a.seed_emb = seed_emb; a.seed_in = seed_in; a.seed_dev = seed_dev;
    return GCNPT_OK;
}

}  // namespace gcnpt

using namespace gcnpt;

extern "C" int gcnpt_embed_fwd(void* stream, const int64_t* words, const float* word_dense, const int64_t* pos, const int64_t* ner,
                               const float* emb, const float* pos_emb, const float* ner_emb, int V0, int V1, int V2, int E0, int E1, int E2,
                               const int32_t* cu_seqlens, int B, int T, int n_rows, void* out, int out_dtype, float p_emb, float p_in,
                               uint64_t seed_emb, uint64_t seed_in, const uint64_t* seed_dev, int32_t* status) {
    GCNPT_REQUIRE(out, "embed_fwd: null output");
    GCNPT_REQUIRE((words != nullptr) != (word_dense != nullptr), "embed_fwd: give word ids or a dense word source, one of the two");
    GCNPT_REQUIRE(!words || emb, "embed_fwd: null word table");
    GCNPT_REQUIRE((E1 <= 0 || pos_emb) && (E2 <= 0 || ner_emb), "embed_fwd: null POS / NER table");
    GCNPT_REQUIRE(dtype_ok(out_dtype), "embed_fwd: bad dtype %d", out_dtype);
    EmbArgs a;
    const int rc = embed_args("embed_fwd", a, words, pos, ner, V0, V1, V2, E0, E1, E2, cu_seqlens, B, T, n_rows, p_emb, p_in, seed_emb,
                              seed_in, seed_dev);
    if (rc != GCNPT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (status) GCNPT_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    const bool pairs = E0 % 2 == 0 && E1 % 2 == 0 && E2 % 2 == 0 && aligned8(out) && aligned8(emb) && aligned8(word_dense) &&
                       aligned8(pos_emb) && aligned8(ner_emb);
    const dim3 grid(ceil_div(T, EM_FWD_TOK), B), block(EM_THREADS);
#define GCNPT_EMBED_FWD(OT, VW) \
    hipLaunchKernelGGL((embed_fwd_kernel<OT, VW>), grid, block, 0, s, a, word_dense, emb, pos_emb, ner_emb, static_cast<OT*>(out), status)
    if (out_dtype == GCNPT_F32) { if (pairs) GCNPT_EMBED_FWD(float, 2); else GCNPT_EMBED_FWD(float, 1); }
    else { if (pairs) GCNPT_EMBED_FWD(bf16_t, 2); else GCNPT_EMBED_FWD(bf16_t, 1); }
#undef GCNPT_EMBED_FWD
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_embed_bwd(void* stream, const void* g, int g_dtype, const int64_t* words, const int64_t* pos, const int64_t* ner,
                               int V0, int V1, int V2, int E0, int E1, int E2, const int32_t* cu_seqlens, int B, int T, int n_rows,
                               float p_emb, float p_in, uint64_t seed_emb, uint64_t seed_in, const uint64_t* seed_dev, int padding_idx,
                               int topn, float* d_emb, float* d_emb_rows, float* d_word_dense, float* d_pos_emb, float* d_ner_emb) {
    GCNPT_REQUIRE(g, "embed_bwd: null gradient");
    GCNPT_REQUIRE(dtype_ok(g_dtype), "embed_bwd: bad dtype %d", g_dtype);
    GCNPT_REQUIRE(d_emb || d_emb_rows || d_word_dense || d_pos_emb || d_ner_emb, "embed_bwd: null outputs (nothing to compute)");
    GCNPT_REQUIRE(!(d_emb && d_emb_rows), "embed_bwd: the word table's gradient is dense or row sparse, not both");
    GCNPT_REQUIRE(!(words && d_word_dense), "embed_bwd: word ids and a dense word source's gradient given, one of the two");
    GCNPT_REQUIRE(words || !(d_emb || d_emb_rows), "embed_bwd: a word table gradient needs the word ids");
    GCNPT_REQUIRE((E1 > 0 || !d_pos_emb) && (E2 > 0 || !d_ner_emb), "embed_bwd: gradient of a table whose segment is 0 wide");
    EmbArgs a;
    const int rc = embed_args("embed_bwd", a, words, pos, ner, V0, V1, V2, E0, E1, E2, cu_seqlens, B, T, n_rows, p_emb, p_in, seed_emb,
                              seed_in, seed_dev);
    if (rc != GCNPT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the accumulators start from zero (the row-sparse and dense-source forms are written completely instead)
    if (d_emb) GCNPT_HIP_CHECK(hipMemsetAsync(d_emb, 0, (size_t)V0 * E0 * sizeof(float), s));
    if (d_pos_emb) GCNPT_HIP_CHECK(hipMemsetAsync(d_pos_emb, 0, (size_t)V1 * E1 * sizeof(float), s));
    if (d_ner_emb) GCNPT_HIP_CHECK(hipMemsetAsync(d_ner_emb, 0, (size_t)V2 * E2 * sizeof(float), s));
    const size_t lds = ((d_pos_emb ? (size_t)V1 * E1 : 0) + (d_ner_emb ? (size_t)V2 * E2 : 0) + (size_t)V1 + V2) * sizeof(float);
    const int use_lds = (d_pos_emb || d_ner_emb) && lds <= EM_LDS_MAX;
    const int pad = padding_idx, top = topn > 0 && topn < V0 ? topn : V0;
    const dim3 grid(ceil_div(T, EM_BWD_TOK), B), block(EM_THREADS);
    if (g_dtype == GCNPT_F32)
        hipLaunchKernelGGL(embed_bwd_kernel<float>, grid, block, use_lds ? lds : 0, s, a, static_cast<const float*>(g), pad, top, d_emb,
                           d_emb_rows, d_word_dense, d_pos_emb, d_ner_emb, use_lds);
    else
        hipLaunchKernelGGL(embed_bwd_kernel<bf16_t>, grid, block, use_lds ? lds : 0, s, a, static_cast<const bf16_t*>(g), pad, top, d_emb,
                           d_emb_rows, d_word_dense, d_pos_emb, d_ner_emb, use_lds);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}
