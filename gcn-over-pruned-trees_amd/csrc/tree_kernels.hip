// Pruned-dependency-tree adjacency on the device (gfx950).
//
// Replaces the host round trip of reference model/gcn.py:96-110 (6 device->host copies, a Python loop
// over model/tree.py:58 head_to_tree and model/tree.py:167 tree_to_adj, one host->device copy of a
// dense [B,T,T] float tensor) with one launch: a workgroup per sentence stages the head array in LDS,
// prunes the tree there and writes the CSR pattern (3n-2 entries for an n-node tree) the layer kernels
// consume.  Integer work only; results are exact.
//
// The pruning uses the closed form of SURVEY.md 3c (fuzz-verified against the reference):
//   chain(t) = t and its ancestors;  CA = intersection of chain(t) over entity tokens;
//   lca = the member of CA with no child in CA;  P = (union of chains - CA) + {lca};
//   dist[i] = edges from i up to its first ancestor-or-self in P (infinite if none);  keep = dist <= K;
//   edges = {(head[i]-1 -> i) : keep[i], i != lca, head[i] > 0}.
#include "gcnpt_common.h"
#include "pack_common.h"
#include "tree_layout.h"

namespace gcnpt {

constexpr int PRUNE_THREADS = 1024;  // wave 0 prunes the sentence (wave-local phases); all 16 waves then emit the rows (one each, typically)
constexpr int PRUNE_SCAN_MAX = 1 << 16;   // B*T up to which workgroup 0 finds the longest sentence itself (no memset, no atomics)
constexpr int ADJ_THREADS = 256;

enum : int {
    F_SUBJ = 1, F_OBJ = 2, F_FWD_NZ = 4, F_REV_NZ = 8, F_CA = 16, F_CA_HASCHILD = 32, F_PATH = 64, F_HASEDGE = 128
};
enum : int { K_KEEP = 1, K_CHILD = 2 };
enum : int { ERR_CHAIN_BADHEAD = 1, ERR_CHAIN_CYCLE = 2, ERR_BADHEAD = 4, ERR_CYCLE = 8, ERR_ASSERT = 16 };

// the parse of a batch [B, T].  The sentences' lengths: from pad_mask, or (NULL) from the array len [B], which travels beside this
// struct as a parameter of its own: `const __restrict__` on a kernel parameter is what makes len[b] a scalar load, and a member
// cannot carry it
struct ParseSrc {
    const int64_t *head, *subj_pos, *obj_pos, *deprel;
    const uint8_t* pad_mask;
};

// Token-packed output of the pruner (gcnpt_prune_to_csr_packed; a PackedDst with cu != NULL): row cu[b] + i, columns
// shifted by cu[b], entry offsets contiguous over the batch.  A sentence's offsets are prefix sums of (len, nnz, nnzT) over the sentences
// before it, which other workgroups of the SAME launch compute: every workgroup publishes its three counts in ONE 8-byte word (valid bit |
// len << 40 | nnz << 20 | nnzT, an agent-scope atomic store: the word is its own flag, nothing to order), then sums the words of the
// sentences before it (agent-scope atomic loads, spinning on the valid bit).  Sentences are taken in TICKET order (an atomic counter), not
// in blockIdx order, so a workgroup only ever waits for workgroups that already run: no assumption about dispatch order.  The last
// workgroup to finish polling clears the words and both counters: the workspace is all-zero between launches (graph replay included).
// sync: [B + 2], zero between launches: the sentences' words, ticket counter, done counter.
constexpr unsigned long long PK_VALID = 1ull << 63;

// exclusive scan of a[0..n) in place, a[n] = total; `scratch` holds blockDim.x ints (any block size)
__device__ void block_exclusive_scan(int* a, int n, int* scratch) {
    const int t = threadIdx.x, nt = blockDim.x;
    const int seg = (n + nt - 1) / nt;
    const int lo = min(n, t * seg), hi = min(n, lo + seg);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += a[i];
    scratch[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < nt; ++k) { int v = scratch[k]; scratch[k] = run; run += v; }
        a[n] = run;
    }
    __syncthreads();
    int run = scratch[t];
    for (int i = lo; i < hi; ++i) { int v = a[i]; a[i] = run; run += v; }
    __syncthreads();
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
// exclusive scan of a[0..n), b[0..n), c[0..n) in place by ONE wave (lane l owns the contiguous segment l), the totals in ta, tb, tc:
// three independent shuffle chains share the latency of one
__device__ __forceinline__ void wave_exclusive_scan3(int* a, int* b, int* c, int n, int lane, int& ta, int& tb, int& tc) {
    const int seg = (n + WAVE - 1) / WAVE;
    const int lo = min(n, lane * seg), hi = min(n, lo + seg);
    int sa = 0, sb = 0, sc = 0;
    for (int i = lo; i < hi; ++i) { sa += a[i]; sb += b[i]; sc += c[i]; }
    int ia = sa, ib = sb, ic = sc;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int ua = __shfl_up(ia, o), ub = __shfl_up(ib, o), uc = __shfl_up(ic, o);
        if (lane >= o) { ia += ua; ib += ub; ic += uc; }
    }
    ta = __shfl(ia, WAVE - 1); tb = __shfl(ib, WAVE - 1); tc = __shfl(ic, WAVE - 1);
    int ra = ia - sa, rb = ib - sb, rc = ic - sc;
    for (int i = lo; i < hi; ++i) {
        const int va = a[i], vb = b[i], vc = c[i];
        a[i] = ra; b[i] = rb; c[i] = rc;
        ra += va; rb += vb; rc += vc;
    }
}

// One 32-bit word per token keeps its parent and its flags together, so that every step of a walk up the tree is
// ONE LDS read:  bits 0..11 = parent + 2 (0 = head points past the sentence, 1 = root / none), bits 12.. = F_* flags.
constexpr int PW_SHIFT = 12, PW_MASK = (1 << PW_SHIFT) - 1, PRUNE_MAX_T = PW_MASK - 3;
__device__ __forceinline__ int pw_par(int w) { return (w & PW_MASK) - 2; }

// One word per row that carries an edge, with everything the row emission needs of it: bits 0..11 = the token, 12..23 = parent + 2 (as
// in its pw word), 24 = it is a kept child of that parent, 25 / 26 = the entry the pair has in the forward / reverse direction is non-zero.
constexpr int ER_CHILD = 1 << 24, ER_FWD_NZ = 1 << 25, ER_REV_NZ = 1 << 26;
__device__ __forceinline__ int er_encode(int token, int pw, int keep_bits) {
    const int f = pw >> PW_SHIFT;
    return token | ((pw & PW_MASK) << PW_SHIFT) | ((keep_bits & K_CHILD) ? ER_CHILD : 0) | ((f & F_FWD_NZ) ? ER_FWD_NZ : 0) |
           ((f & F_REV_NZ) ? ER_REV_NZ : 0);
}
__device__ __forceinline__ int er_token(int w) { return w & PW_MASK; }
__device__ __forceinline__ int er_parent(int w) { return pw_par(w >> PW_SHIFT); }
__device__ __forceinline__ bool er_is_child(int w) { return w & ER_CHILD; }
__device__ __forceinline__ bool er_fwd_nz(int w) { return w & ER_FWD_NZ; }
__device__ __forceinline__ bool er_rev_nz(int w) { return w & ER_REV_NZ; }

// Sentences of up to PRUNE_WAVE0_T tokens: wave 0 runs the pruning phases alone, separated by wave_lds_fence() (gcnpt_common.h): no
// workgroup barrier.  Longer ones (ALLW): every phase is a loop over the tokens by ALL 1024 threads with a
// workgroup barrier behind it, so a 300-token sentence is one round per phase instead of five (round 2: 30 us at T = 300).
#ifndef GCNPT_PRUNE_WAVE0_T
#define GCNPT_PRUNE_WAVE0_T 64       // measured (tools/ab_libs.sh): T = 100 takes 8.4 us with wave 0 alone, 7.3 us with all waves; T = 50: 4.1 against 5.4
#endif
constexpr int PRUNE_WAVE0_T = GCNPT_PRUNE_WAVE0_T;

// status[B] = longest sentence of the batch (gcn.py:97).  false: waves of workgroup 0 that have no token to prune find it (see the
// kernel).  true -- batches too big for that, sentences that leave no idle wave --: one atomicMax per sentence, on a word that
// prune_impl clears in front of the launch.
__host__ __device__ constexpr bool longest_by_atomic(int B, int T) {
    return (long long)B * T > PRUNE_SCAN_MAX || (T > PRUNE_WAVE0_T && T + WAVE > PRUNE_THREADS);
}

// The workgroup's dynamic LDS: PER_TOKEN words per token for the pruning phases, PER_TOKEN_STAGED with the entry lists of the staged
// row emission (emit_rows), FIXED on top (deg, degT and rank hold T + 1).  Two regions change hands between the phases.
struct PruneLds {
    static constexpr int PER_TOKEN = 7, PER_TOKEN_STAGED = 14, FIXED = 4;
    // (n_long is the LAST word of bytes(T, true): entF starts behind FIXED, so there is no slack word to give away)
    static constexpr size_t bytes(int T, bool staged) { return sizeof(int) * ((size_t)(staged ? PER_TOKEN_STAGED : PER_TOKEN) * T + FIXED); }
    int* pw;        // [T]   parent + flags (see above)
    int* cnt;       // [T]   #entity chains through the token; from the distance phase on the K_KEEP / K_CHILD bits; in the staged
                    //       emission the fill counter of the forward rows
    int* deg;       // [T+1] row degree -> row offsets
    int* degT;      // [T+1] column degree -> transposed row offsets
    int* rank;      // [T+1] rank of the token among the rows that carry an edge; in the staged emission the fill counter of the transposed rows
    int* lab;       // [T]   deprel id of the token
    int* einfo;     // [T]   the edge rows, ascending (er_encode)
    // staged only
    int* entF;      // [3T]  forward entries: column (the label follows from the pair, see write_row)
    int* entT;      // [3T]  transposed entries: column
    int* longrows;  // [<= T / EMIT_SORT_MAX + 1] edge rows left to the scan form
    int* n_long;    //       their count: the last word of that region
    __device__ PruneLds(int* smem, int T)
        : pw(smem), cnt(pw + T), deg(cnt + T), degT(deg + T + 1), rank(degT + T + 1), lab(rank + T + 1), einfo(lab + T),
          entF(smem + PER_TOKEN * T + FIXED), entT(entF + 3 * T), longrows(entT + 3 * T), n_long(longrows + T - 1) {}
};

// The workgroup's static words.
struct PruneShared {
    int err;        // ERR_* bits of the phases
    int status;     // the sentence's GCNPT_E_* code (packed output that does not fit: GCNPT_E_CAPACITY)
    int nrows;      // rows that carry an edge (0 for a failed sentence)
    int red[4];     // workgroup-wide sums / minimum of the ALLW form: [0] pad slots, [1] subject tokens, [2] entity tokens, [3] lca;
                    // then the three sums of the look-back
    int out[4];     // padded: first row, first entry of the two patterns, column shift; packed: len, nnz, nnzT until the look-back
    int ticket;     // the sentence this workgroup takes
    int maxlen;     // workgroup 0: the longest sentence
};

// Phases: lengths, LCA, path, distances, kept tokens, degrees, row offsets, compacted edge rows.
// (dst by reference here and in emit_rows / emit_row_scan: measured against a copy, the packed shapes are 0.1 us faster.)
template <bool ALLW>
__device__ void prune_sentence(const ParseSrc in, const int32_t* __restrict__ len_in, int b, int B, int T, int prune_k, int cap,
                               const PruneLds L, PruneShared& sh, const PackedDst& dst, unsigned long long* sync,
                               unsigned long long* stamps) {
    int *const pw = L.pw, *const cnt = L.cnt, *const deg = L.deg, *const degT = L.degT, *const rank = L.rank;
    const int lane = threadIdx.x & 63;
    const int t0 = ALLW ? (int)threadIdx.x : lane;            // this thread's first token
    constexpr int NT = ALLW ? PRUNE_THREADS : WAVE;           // token stride
    const size_t base = (size_t)b * T;
    auto phase_sync = [&]() { if constexpr (ALLW) __syncthreads(); else wave_lds_fence(); };
    // sum over the participating threads (ALLW: through sh.red[slot], which the kernel cleared; the caller syncs before reading)
    auto team_sum = [&](int v, int slot) {
        v = wave_sum(v);
        if constexpr (ALLW) { if (lane == 0 && v) atomicAdd(&sh.red[slot], v); }
        return v;
    };

    // ---- stage the parse (tree.py:60-63, 82-83).  Wave-0 form: two tokens per lane per round, every load of the round issued before
    // the first use (clamped addresses, no load behind a condition): a sentence of up to 128 tokens costs ONE memory round trip.
    // ALLW: one token per thread, one round for up to 1024 tokens.
    int npad = 0;
    constexpr int PER = ALLW ? 1 : 2;
    for (int i0 = 0; i0 < T; i0 += PER * NT) {
        int64_t h[PER], sp[PER], op[PER], d[PER];
        bool pad[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const size_t j = base + min(i0 + u * NT + t0, T - 1);
            h[u] = in.head[j]; sp[u] = in.subj_pos[j]; op[u] = in.obj_pos[j]; d[u] = in.deprel[j];
            pad[u] = in.pad_mask ? in.pad_mask[j] != 0 : false;
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = i0 + u * NT + t0;
            if (i >= T) continue;
            npad += pad[u] ? 1 : 0;
            int f = 0;
            if (sp[u] == 0) f |= F_SUBJ;
            if (op[u] == 0) f |= F_OBJ;
            if (d[u] != 0) f |= F_FWD_NZ;                  // adj[p,c] = deprel[c]        survives `adj != 0`
            if (d[u] + FWD_BOUND != 0) f |= F_REV_NZ;      // adj[c,p] = deprel[c] + 42
            const int p = h[u] > 0 ? (int)min(h[u] - 1, (int64_t)(PW_MASK - 2)) : -1;      // range-checked against len below
            pw[i] = (p + 2) | (f << PW_SHIFT);
            L.lab[i] = (int)d[u]; cnt[i] = 0; deg[i] = 0; degT[i] = 0;
        }
    }
    // sentence length = number of non-pad slots (gcn.py:96)
    int len;
    if (in.pad_mask) {
        const int np = team_sum(npad, 0);
        if constexpr (ALLW) { __syncthreads(); len = T - sh.red[0]; } else { len = T - np; }
    } else {
        len = min(max(len_in[b], 0), T);
    }
    if (threadIdx.x == 0 && longest_by_atomic(B, T)) atomicMax(&dst.sent_status[B], len);
    int nsubj = 0, nent = 0;
    for (int i = t0; i < T; i += NT) {
        const int w = pw[i];
        int f = w >> PW_SHIFT, p = pw_par(w);
        if (i >= len) { f = 0; p = -1; }
        else if (p >= len) p = -2;
        nsubj += (f & F_SUBJ) ? 1 : 0;
        nent += ((f & F_SUBJ) ? 1 : 0) + ((f & F_OBJ) ? 1 : 0);
        pw[i] = (p + 2) | (f << PW_SHIFT);
    }
    nsubj = team_sum(nsubj, 1);
    nent = team_sum(nent, 2);
    phase_sync();
    if constexpr (ALLW) { nsubj = sh.red[1]; nent = sh.red[2]; }
    GCNPT_STAMP(stamps, 1);

    // ---- every entity token walks to the root, counting visits (tree.py:86-109)
    for (int i = t0; i < len; i += NT) {
        const int f = pw[i] >> PW_SHIFT;
        const int w = ((f & F_SUBJ) ? 1 : 0) + ((f & F_OBJ) ? 1 : 0);
        if (!w) continue;
        int a = i, steps = 0;
        while (a >= 0) {
            atomicAdd(&cnt[a], w);                     // result unused: no-return LDS add, nothing to wait for
            a = pw_par(pw[a]);
            if (++steps > len) { atomicOr(&sh.err, ERR_CHAIN_CYCLE); a = -1; }
        }
        if (a == -2) atomicOr(&sh.err, ERR_CHAIN_BADHEAD);
    }
    phase_sync();
    int err = 0;
    if (sh.err & ERR_CHAIN_BADHEAD) err = GCNPT_E_BAD_HEAD;
    else if (sh.err & ERR_CHAIN_CYCLE) err = GCNPT_E_CYCLE;
    else if (nsubj == 0) err = GCNPT_E_NO_SUBJECT;
    GCNPT_STAMP(stamps, 2);

    // ---- common ancestors and the lowest of them (tree.py:112-124)
    int lca = 0x7fffffff;
    if (!err) {                                          // (err is the same in every thread: the syncs below are uniform)
        for (int i = t0; i < len; i += NT)
            if (cnt[i] == nent) pw[i] |= F_CA << PW_SHIFT;
        phase_sync();
        for (int i = t0; i < len; i += NT) {
            const int w = pw[i], p = pw_par(w);
            if ((w & (F_CA << PW_SHIFT)) && p >= 0 && (pw[p] & (F_CA << PW_SHIFT))) atomicOr(&pw[p], F_CA_HASCHILD << PW_SHIFT);
        }
        phase_sync();
        for (int i = t0; i < len; i += NT)
            if (((pw[i] >> PW_SHIFT) & (F_CA | F_CA_HASCHILD)) == F_CA) lca = min(lca, i);
        lca = wave_min(lca);
        if constexpr (ALLW) {
            if (lane == 0 && lca != 0x7fffffff) atomicMin(&sh.red[3], lca);
            __syncthreads();
            lca = sh.red[3];
        }
        if (lca == 0x7fffffff) err = GCNPT_E_NO_LCA;
    }
    GCNPT_STAMP(stamps, 3);

    // ---- path nodes, distance to the path, kept tokens (tree.py:126-147)
    if (!err) {
        for (int i = t0; i < len; i += NT)
            if ((cnt[i] > 0 && !(pw[i] & (F_CA << PW_SHIFT))) || i == lca) pw[i] |= F_PATH << PW_SHIFT;
        phase_sync();
        for (int i = t0; i < len; i += NT) {
            int a = i, d = 0, w = pw[i];
            while (a >= 0 && !(w & (F_PATH << PW_SHIFT))) {          // one LDS read per step
                a = pw_par(w);
                if (a >= 0) w = pw[a];
                if (++d > len) { atomicOr(&sh.err, ERR_CYCLE); a = -1; }
            }
            if (a == -2) atomicOr(&sh.err, ERR_BADHEAD);
            const bool keep = a >= 0 && d <= prune_k;
            const bool child = keep && i != lca && pw_par(pw[i]) >= 0;
            cnt[i] = (keep ? K_KEEP : 0) | (child ? K_CHILD : 0);   // cnt is free from here on
        }
        phase_sync();
        if (sh.err & ERR_BADHEAD) err = GCNPT_E_BAD_HEAD;
        else if (sh.err & ERR_CYCLE) err = GCNPT_E_CYCLE;
    }
    GCNPT_STAMP(stamps, 4);

    // ---- degrees of the labelled adjacency tree_to_adj would write (tree.py:182-192)
    if (!err) {
        for (int i = t0; i < len; i += NT) {
            if (!(cnt[i] & K_CHILD)) continue;
            const int w = pw[i], p = pw_par(w), f = w >> PW_SHIFT;
            if (!(cnt[p] & K_KEEP)) atomicOr(&sh.err, ERR_ASSERT);   // tree.py:159
            if (f & F_FWD_NZ) { atomicAdd(&deg[p], 1); atomicAdd(&degT[i], 1); }
            if (f & F_REV_NZ) { atomicAdd(&deg[i], 1); atomicAdd(&degT[p], 1); }
            atomicOr(&pw[p], F_HASEDGE << PW_SHIFT);
            atomicOr(&pw[i], F_HASEDGE << PW_SHIFT);
        }
        phase_sync();
        if (sh.err & ERR_ASSERT) err = GCNPT_E_ASSERT;
    }
    int n_edge_rows = 0;
    if (!err) {
        for (int i = t0; i < T; i += NT) {
            const int he = (i < len && (pw[i] & (F_HASEDGE << PW_SHIFT))) ? 1 : 0;
            deg[i] += he; degT[i] += he;                             // the 84 on the diagonal
            rank[i] = he;
            if (dst.pool_mask_padded) dst.pool_mask_padded[base + i] = (deg[i] + degT[i]) == 0;      // gcn.py:262
        }
        phase_sync();
        if (!ALLW || threadIdx.x < WAVE) {                           // the three scans: one wave (lane l owns a contiguous segment)
            int tot, totT;
            wave_exclusive_scan3(deg, degT, rank, T, lane, tot, totT, n_edge_rows);
            if (lane == 0) { deg[T] = tot; degT[T] = totT; rank[T] = n_edge_rows; }
        }
        phase_sync();
        n_edge_rows = rank[T];
        if (deg[T] > cap || degT[T] > cap) err = GCNPT_E_CAPACITY;
    }
    GCNPT_STAMP(stamps, 5);

    // ---- where this sentence's rows and entries go.  Padded layout: slots of its own (rows b*T.., entries b*cap..), its T + 1 row
    //      offsets from b*(T+1).  Packed: behind the sentences before it (see PK_VALID): the counts are published HERE, the offsets
    //      are taken as late as possible -- in emit_rows(), after the rows have been sorted in registers --, so that waiting for a
    //      slower sentence costs nothing
    const bool packed = dst.cu != nullptr;
    if (packed) {
        const int my_nnz = err ? 0 : deg[T], my_nnzT = err ? 0 : degT[T];
        if (threadIdx.x == 0) {
            __hip_atomic_store(sync + b, PK_VALID | ((unsigned long long)len << 40) | ((unsigned long long)my_nnz << 20) | (unsigned long long)my_nnzT,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sh.out[0] = len; sh.out[1] = my_nnz; sh.out[2] = my_nnzT;
            dst.sent_status[b] = err; sh.status = err; sh.nrows = err ? 0 : n_edge_rows;
        }
        if (err) {                                                   // (its rows are written in emit_rows)
            if (dst.pool_mask_padded)
                for (int i = t0; i < T; i += NT) dst.pool_mask_padded[base + i] = 1;
            return;
        }
        for (int i = t0; i < len; i += NT) {                         // the compacted edge rows (see below); every global write waits
            const int w = pw[i];
            if (w & (F_HASEDGE << PW_SHIFT)) L.einfo[rank[i]] = er_encode(i, w, cnt[i]);
        }
        if constexpr (!ALLW) wave_lds_fence();
        GCNPT_STAMP(stamps, 6);
        return;
    }
    const int ebase = b * cap;
    const size_t rp0 = (size_t)b * (T + 1);
    if (threadIdx.x == 0) { sh.out[0] = (int)base; sh.out[1] = ebase; sh.out[2] = ebase; sh.out[3] = 0; }

    if (err) {   // the sentence contributes no edges; every row is empty and masked
        for (int i = t0; i < T + 1; i += NT) {
            dst.row_ptr[rp0 + i] = ebase;
            if (dst.rowT_ptr) dst.rowT_ptr[rp0 + i] = ebase;
        }
        for (int i = t0; i < T; i += NT) {
            if (dst.pool_mask_padded) dst.pool_mask_padded[base + i] = 1;
            zero_ell_head(base + i, dst.ell, dst.ellT);
        }
        if (threadIdx.x == 0) { dst.sent_status[b] = err; sh.status = err; }
        return;
    }

    // ---- emit both patterns, columns ascending (same order a dense -> CSR conversion gives).
    // Only rows that carry an edge have entries, and only such rows appear as columns: compact them (ascending)
    // with everything the inner loop needs in ONE word, so that loop is a stream of broadcast LDS reads.
    for (int i = t0; i < T + 1; i += NT) {
        dst.row_ptr[rp0 + i] = ebase + deg[i];
        if (dst.rowT_ptr) dst.rowT_ptr[rp0 + i] = ebase + degT[i];
    }
    for (int i = t0; i < T; i += NT) {
        const int w = i < len ? pw[i] : 0;
        if (w & (F_HASEDGE << PW_SHIFT)) L.einfo[rank[i]] = er_encode(i, w, cnt[i]);
        else zero_ell_head(base + i, dst.ell, dst.ellT);              // no entries
    }
    if constexpr (!ALLW) wave_lds_fence();                          // (ALLW: the kernel's barrier in front of emit_rows)
    GCNPT_STAMP(stamps, 6);
    if (threadIdx.x == 0) { sh.nrows = n_edge_rows; dst.sent_status[b] = 0; }
}

// One row of both patterns by ONE WAVE: one candidate column per lane (the edge rows, ascending), ballot + prefix popcount give every
// entry its slot -- no sorting, any number of entries.  me: the row's edge-row word; labr_raw, o_rel, oT_rel: its lab / deg / degT (the
// chunked caller holds them in the lanes' registers and reads row qq of the chunk with v_readlane); base, ebase, eTbase, cshift: where
// the sentence's rows and entries go (emit_rows).
__device__ __forceinline__ void emit_row_scan(const PruneLds L, int n_edge_rows, size_t base, int ebase, int eTbase, int cshift, int me,
                                              int labr_raw, int o_rel, int oT_rel, const PackedDst& dst) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int r = er_token(me), rp = er_parent(me);
    const bool rchild = er_is_child(me), rfwd = er_fwd_nz(me), rrev = er_rev_nz(me);
    const int labr = labr_raw + FWD_BOUND;
    const int o = ebase + o_rel, oT = eTbase + oT_rel;
    int32_t* hd = dst.ell + (base + r) * 8;                   // ELL head: [0] = count, [1..7] = first 7 columns
    int32_t* hdT = dst.ellT ? dst.ellT + (base + r) * 8 : nullptr;
    int n_e = 0, n_eT = 0;
    for (int k0 = 0; k0 < n_edge_rows; k0 += WAVE) {          // candidate columns: the edge rows, ascending
        const bool valid = k0 + lane < n_edge_rows;
        const int w = valid ? L.einfo[k0 + lane] : 0;
        const int j = er_token(w);
        const bool is_child = valid && er_is_child(w) && er_parent(w) == r;      // j is a kept child of r
        const bool is_self = valid && j == r;
        const bool is_par = valid && rchild && j == rp;
        const bool e = (is_child && er_fwd_nz(w)) || is_self || (is_par && rrev);      // adj[r,j] != 0
        const bool eT = (is_child && er_rev_nz(w)) || is_self || (is_par && rfwd);     // adj[j,r] != 0
        const unsigned long long m = __ballot(e), mT = __ballot(eT);
        if (e) {
            const int pos = n_e + __popcll(m & lt);
            dst.col_idx[o + pos] = j + cshift;
            if (dst.label) dst.label[o + pos] = is_self ? SELF_LOOP_ID : (is_child ? L.lab[j] : labr);
            if (pos < 7) hd[1 + pos] = j + cshift;
        }
        if (eT) {
            const int pos = n_eT + __popcll(mT & lt);
            if (dst.colT_idx) dst.colT_idx[oT + pos] = j + cshift;
            if (hdT && pos < 7) hdT[1 + pos] = j + cshift;
        }
        n_e += __popcll(m);
        n_eT += __popcll(mT);
    }
    if (lane < 8) {                                           // count, and zeros in the unused slots
        if (lane == 0) hd[0] = n_e; else if (lane > n_e) hd[lane] = 0;
        if (hdT) { if (lane == 0) hdT[0] = n_eT; else if (lane > n_eT) hdT[lane] = 0; }
    }
}

// All 16 waves: the CSR entries and ELL heads of the rows that carry an edge.
// STAGED (sentences whose entry lists fit LDS beside the pruning arrays): every edge row is a THREAD.  It appends its own entries
// (diagonal; for a kept child also the pair with its parent) to the rows' LDS segments through per-row fill counters, and after one
// barrier sorts its row's segment by column (an insertion sort: a row of a pruned tree has 2-4 entries) and writes it out with its
// ELL head.  Rows with more than EMIT_SORT_MAX entries (a star-shaped parse) go to the scan form below, one wave each.
// Otherwise: one row at a time per wave, one candidate column per lane (emit_row_scan) -- O(rows^2 / 64) wave iterations, which at
// T = 300, K = 2 was 11-25 k cycles of the sentence's 29-43 k.
// Token-packed output: the sentence's offsets are resolved INSIDE it.
constexpr int EMIT_SORT_MAX = 12;
__device__ void emit_rows(const PruneLds L, PruneShared& sh, int b, int B, int T, bool staged, const PackedDst& dst,
                          unsigned long long* sync, unsigned long long* stamps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int err = sh.status, n_edge_rows = sh.nrows;
    const bool packed = dst.cu != nullptr;
    if (err && !packed) return;
    GCNPT_STAMP(stamps, 8);
    int *const cnt = L.cnt, *const deg = L.deg, *const degT = L.degT, *const rank = L.rank;      // (cnt, rank: the fill counters)
    size_t base = (size_t)sh.out[0];                       // first row, first entries of the two patterns, column shift (prune_sentence)
    int ebase = sh.out[1], eTbase = sh.out[2], cshift = sh.out[3];
    int done = -1;                                         // (thread 0, packed) how many workgroups had resolved before this one

    // Token-packed output: the look-back (see PK_VALID).  Sums the words of the sentences before this one (spinning on their valid bits),
    // then writes everything of the sentence that is not an entry of an edge row: cu, row offsets, empty ELL heads, masks, sentence ids.
    // All threads; false = the sentence does not fit the caller's arrays (nothing of it is written: gcnpt_pack_trees' rule).
    auto resolve = [&]() -> bool {
        const int len = sh.out[0], my_nnz = sh.out[1], my_nnzT = sh.out[2];
        int a0 = 0, a1 = 0, a2 = 0;
        for (int j = threadIdx.x; j < b; j += PRUNE_THREADS) {
            unsigned long long v = __hip_atomic_load(sync + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (!(v & PK_VALID)) {
                __builtin_amdgcn_s_sleep(2);
                v = __hip_atomic_load(sync + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            a0 += (int)((v >> 40) & 0xffff); a1 += (int)((v >> 20) & 0xfffff); a2 += (int)(v & 0xfffff);
        }
        a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
        __syncthreads();                                               // (sh.out and the sums of the pruning phases are consumed)
        if (threadIdx.x == 0) { sh.red[0] = 0; sh.red[1] = 0; sh.red[2] = 0; }
        __syncthreads();
        if (lane == 0 && (a0 | a1 | a2)) { atomicAdd(&sh.red[0], a0); atomicAdd(&sh.red[1], a1); atomicAdd(&sh.red[2], a2); }
        __syncthreads();
        a0 = sh.red[0]; a1 = sh.red[1]; a2 = sh.red[2];
        // this workgroup has polled every sentence before it: the last one to get here leaves the workspace zeroed (finish(), below; the
        // counter's old value is only looked at there, so its round trip is off the sentence's critical path)
        if (threadIdx.x == 0) done = (int)atomicAdd(sync + B + 1, 1ull);
        base = (size_t)a0; ebase = a1; eTbase = a2; cshift = a0;
        if (!write_packed_header(b, B, a0, a1, a2, len, my_nnz, my_nnzT, dst.cu, dst.row_ptr, dst.rowT_ptr, dst.status, dst.n_rows, dst.nnz_cap)) {
            if (threadIdx.x == 0) sh.status = GCNPT_E_CAPACITY;
            return false;
        }
        for (int i = threadIdx.x; i < len; i += PRUNE_THREADS) {
            dst.row_sent[a0 + i] = b;
            dst.row_ptr[a0 + i] = a1 + (err ? 0 : deg[i]);
            if (dst.rowT_ptr) dst.rowT_ptr[a0 + i] = a2 + (err ? 0 : degT[i]);
            if (dst.pool_mask) dst.pool_mask[a0 + i] = err ? 1 : ((deg[i + 1] - deg[i]) + (degT[i + 1] - degT[i])) == 0;
            if (err || !(L.pw[i] & (F_HASEDGE << PW_SHIFT))) zero_ell_head(a0 + i, dst.ell, dst.ellT);
        }
        return true;
    };
    auto finish = [&]() {
        if (packed && threadIdx.x == 0 && done == B - 1)
            for (int j = 0; j < B + 2; ++j) sync[j] = 0ull;
    };
    if (err) {                                                         // (packed) an empty sentence still has its rows
        resolve();
        finish();
        return;
    }

    if (staged && (n_edge_rows > WAVE || packed)) {          // (up to 64 edge rows the scan form is as fast: 4.7 k against 5.3 k cycles at T = 100, K = 1)
        for (int i = threadIdx.x; i < T; i += PRUNE_THREADS) { cnt[i] = 0; rank[i] = 0; }
        if (threadIdx.x == 0) *L.n_long = 0;
        __syncthreads();
        for (int q = threadIdx.x; q < n_edge_rows; q += PRUNE_THREADS) {
            const int me = L.einfo[q];
            const int r = er_token(me), rp = er_parent(me);
            L.entF[deg[r] + atomicAdd(&cnt[r], 1)] = r;                                             // adj[r,r] = 84 (tree.py:186-187)
            L.entT[degT[r] + atomicAdd(&rank[r], 1)] = r;
            if (er_is_child(me)) {                                                                  // r is a kept child of rp
                if (er_fwd_nz(me)) {                                                                // adj[rp,r] = deprel[r]
                    L.entF[deg[rp] + atomicAdd(&cnt[rp], 1)] = r;
                    L.entT[degT[r] + atomicAdd(&rank[r], 1)] = rp;
                }
                if (er_rev_nz(me)) {                                                                // adj[r,rp] = deprel[r] + 42
                    L.entF[deg[r] + atomicAdd(&cnt[r], 1)] = rp;
                    L.entT[degT[rp] + atomicAdd(&rank[rp], 1)] = r;
                }
            }
        }
        __syncthreads();
        // a thread's edge row: its entries sorted by column in registers (sort_row), then written with its ELL head (write_row).  Packed
        // output, one row per thread at most: the offsets are resolved BETWEEN the two, so a sentence that has to wait for a slower one
        // before it waits with its rows sorted
        struct Row { int r, o, n, oT, nT; int v[EMIT_SORT_MAX], vT[EMIT_SORT_MAX]; };
        auto sort_row = [&](int q, Row& w) -> bool {
            w.r = er_token(L.einfo[q]);
            w.o = deg[w.r]; w.n = deg[w.r + 1] - w.o; w.oT = degT[w.r]; w.nT = degT[w.r + 1] - w.oT;
            if (w.n > EMIT_SORT_MAX || w.nT > EMIT_SORT_MAX) { L.longrows[atomicAdd(L.n_long, 1)] = q; return false; }
#pragma unroll
            for (int k = 0; k < EMIT_SORT_MAX; ++k) {
                w.v[k] = k < w.n ? L.entF[w.o + k] : 0x7fffffff;
                w.vT[k] = k < w.nT ? L.entT[w.oT + k] : 0x7fffffff;
            }
            // (a fixed odd-even transposition network keeps the arrays in registers; unused slots hold INT_MAX and stay behind)
#pragma unroll
            for (int pass = 0; pass < EMIT_SORT_MAX; ++pass)
#pragma unroll
                for (int k = pass & 1; k + 1 < EMIT_SORT_MAX; k += 2) {
                    const bool sw = w.v[k] > w.v[k + 1];
                    const int lo = sw ? w.v[k + 1] : w.v[k], hi = sw ? w.v[k] : w.v[k + 1];
                    w.v[k] = lo; w.v[k + 1] = hi;
                    const bool swT = w.vT[k] > w.vT[k + 1];
                    const int loT = swT ? w.vT[k + 1] : w.vT[k], hiT = swT ? w.vT[k] : w.vT[k + 1];
                    w.vT[k] = loT; w.vT[k + 1] = hiT;
                }
            return true;
        };
        auto write_row = [&](const Row& w) {
            const int r = w.r, o = w.o, n = w.n, oT = w.oT, nT = w.nT;
            int hd[8], hdT[8];
            hd[0] = n; hdT[0] = nT;
#pragma unroll
            for (int k = 0; k < EMIT_SORT_MAX; ++k) {
                if (k < n) {
                    const int j = w.v[k];
                    dst.col_idx[ebase + o + k] = j + cshift;
                    // the value tree_to_adj wrote there (tree.py:184-192): 84 on the diagonal, deprel[j] for a child j, deprel[r] + 42 for the parent
                    if (dst.label) dst.label[ebase + o + k] = j == r ? SELF_LOOP_ID : (pw_par(L.pw[j]) == r ? L.lab[j] : L.lab[r] + FWD_BOUND);
                }
                if (k < nT && dst.colT_idx) dst.colT_idx[eTbase + oT + k] = w.vT[k] + cshift;
                if (k < 7) { hd[1 + k] = k < n ? w.v[k] + cshift : 0; hdT[1 + k] = k < nT ? w.vT[k] + cshift : 0; }
            }
            int4* e = reinterpret_cast<int4*>(dst.ell + (base + r) * 8);
            e[0] = make_int4(hd[0], hd[1], hd[2], hd[3]); e[1] = make_int4(hd[4], hd[5], hd[6], hd[7]);
            if (dst.ellT) {
                int4* eT = reinterpret_cast<int4*>(dst.ellT + (base + r) * 8);
                eT[0] = make_int4(hdT[0], hdT[1], hdT[2], hdT[3]); eT[1] = make_int4(hdT[4], hdT[5], hdT[6], hdT[7]);
            }
        };
        if (packed && n_edge_rows <= PRUNE_THREADS) {
            Row w;
            const bool mine = (int)threadIdx.x < n_edge_rows && sort_row(threadIdx.x, w);
            if (!resolve()) { finish(); return; }
            if (mine) write_row(w);
        } else {
            if (packed && !resolve()) { finish(); return; }
            for (int q = threadIdx.x; q < n_edge_rows; q += PRUNE_THREADS) {
                Row w;
                if (sort_row(q, w)) write_row(w);
            }
        }
        __syncthreads();
        const int nl = *L.n_long;
        for (int x = wave; x < nl; x += PRUNE_THREADS / WAVE) {           // the few long rows: one wave each, scan form
            const int me = L.einfo[L.longrows[x]];
            const int r = er_token(me);
            emit_row_scan(L, n_edge_rows, base, ebase, eTbase, cshift, me, L.lab[r], deg[r], degT[r], dst);
        }
        GCNPT_STAMP(stamps, 7);
        finish();
        return;
    }
    if (packed && !resolve()) { finish(); return; }
    for (int q0 = 0; q0 < n_edge_rows; q0 += WAVE) {                  // rows, a chunk of 64 at a time (registers)
        const int rw = q0 + lane < n_edge_rows ? L.einfo[q0 + lane] : 0;
        const int rdeg = deg[er_token(rw)], rdegT = degT[er_token(rw)], rlab = L.lab[er_token(rw)];
        const int nq = min(WAVE, n_edge_rows - q0);
        for (int qq = wave; qq < nq; qq += PRUNE_THREADS / WAVE) {    // this wave's rows of the chunk
            emit_row_scan(L, n_edge_rows, base, ebase, eTbase, cshift, __builtin_amdgcn_readlane(rw, qq), __builtin_amdgcn_readlane(rlab, qq),
                          __builtin_amdgcn_readlane(rdeg, qq), __builtin_amdgcn_readlane(rdegT, qq), dst);
        }
    }
    GCNPT_STAMP(stamps, 7);
    finish();
}

// in, len: the parse; dst: the arrays in either layout (PackedDst), sync: the look-back workspace of the packed one; pk, pk_dtype: the side job
__global__ __launch_bounds__(PRUNE_THREADS) void prune_to_csr_kernel(const ParseSrc in, const int32_t* __restrict__ len,
                                                                     int B, int T, int prune_k, int cap,
                                                                     const PackedDst dst, unsigned long long* sync,
                                                                     unsigned long long* stamps, const PackParams pk, int pk_dtype, int staged) {
    extern __shared__ int smem[];
    __shared__ PruneShared sh;
    if ((int)blockIdx.x >= B) {    // side job of gcnpt_prune_to_csr_pack: the launch leaves most CUs idle, these workgroups pack the weights
        pack_side_job(pk, pk_dtype, B);
        return;
    }
    const PruneLds L(smem, T);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // packed output: sentences in ticket order (see PK_VALID), else the workgroup's own
    if (threadIdx.x == 0) sh.ticket = dst.cu ? (int)atomicAdd(sync + B, 1ull) : (int)blockIdx.x;
    if (threadIdx.x == 0) { sh.err = 0; sh.status = 0; sh.nrows = 0; sh.red[0] = sh.red[1] = sh.red[2] = 0; sh.red[3] = 0x7fffffff; }
    GCNPT_STAMP_REAL(stamps);
    GCNPT_STAMP(stamps, 0);
    if (threadIdx.x == 0) sh.maxlen = 0;
    __syncthreads();
    const int b = sh.ticket;
    const bool allw = T > PRUNE_WAVE0_T;
    // the longest sentence (longest_by_atomic): waves of workgroup 0 that have no token to prune count every sentence's non-pad slots
    // while the others prune (wave 0 alone, or the waves holding the T tokens), so the launch needs neither a memset of that word nor
    // one atomic per sentence
    const bool scan_longest = b == 0 && !longest_by_atomic(B, T);
    const int first_idle = allw ? (T + WAVE - 1) / WAVE : 1;
    if (scan_longest && wave >= first_idle) {
        const int n_idle = PRUNE_THREADS / WAVE - first_idle;
        int m = 0;
        for (int sidx = wave - first_idle; sidx < B; sidx += n_idle) {
            int n;
            if (in.pad_mask) {
                n = 0;
                for (int i0 = 0; i0 < T; i0 += WAVE) {
                    const int i = i0 + lane;
                    n += __popcll(__ballot(i < T && in.pad_mask[(size_t)sidx * T + min(i, T - 1)] == 0));
                }
            } else {
                n = min(max(len[sidx], 0), T);
            }
            m = max(m, n);
        }
        if (lane == 0) atomicMax(&sh.maxlen, m);
    }
    if (allw) prune_sentence<true>(in, len, b, B, T, prune_k, cap, L, sh, dst, sync, stamps);
    else if (wave == 0) prune_sentence<false>(in, len, b, B, T, prune_k, cap, L, sh, dst, sync, stamps);
    __syncthreads();
    if (scan_longest && threadIdx.x == 0) dst.sent_status[B] = sh.maxlen;
    emit_rows(L, sh, b, B, T, staged != 0, dst, sync, stamps);
    // (packed output that did not fit: the per-sentence code stays what the pruning found; the batch-level status says E_CAPACITY)
}

// ---- dense float adjacency -> CSR of (adj != 0) and of its transpose (gcn.py:260-262) -----------------
__global__ __launch_bounds__(ADJ_THREADS) void adj_to_csr_kernel(
    const float* __restrict__ adj, int B, int T, int cap, int32_t* __restrict__ row_ptr, int32_t* __restrict__ col_idx,
    int32_t* __restrict__ label, int32_t* __restrict__ rowT_ptr, int32_t* __restrict__ colT_idx,
    int32_t* __restrict__ ell, int32_t* __restrict__ ellT, uint8_t* __restrict__ pool_mask,
    int32_t* __restrict__ status) {
    extern __shared__ int smem[];
    int* deg = smem;              // [T+1]
    int* degT = deg + T + 1;      // [T+1]
    int* scratch = degT + T + 1;  // [ADJ_THREADS]
    const int b = blockIdx.x, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6, NW = ADJ_THREADS / WAVE;
    const float* A = adj + (size_t)b * T * T;

    for (int r = wave; r < T; r += NW) {
        int n = 0, nT = 0;
        for (int c0 = 0; c0 < T; c0 += WAVE) {
            const int c = c0 + lane;
            const bool nz = c < T && A[(size_t)r * T + c] != 0.0f;
            const bool nzT = c < T && A[(size_t)c * T + r] != 0.0f;
            n += __popcll(__ballot(nz));
            nT += __popcll(__ballot(nzT));
        }
        if (lane == 0) { deg[r] = n; degT[r] = nT; }
    }
    __syncthreads();
    if (pool_mask)
        for (int i = t; i < T; i += ADJ_THREADS) pool_mask[(size_t)b * T + i] = (deg[i] + degT[i]) == 0;
    __syncthreads();
    block_exclusive_scan(deg, T, scratch);
    block_exclusive_scan(degT, T, scratch);
    const bool over = deg[T] > cap;
    for (int i = t; i <= T; i += ADJ_THREADS) {
        row_ptr[(size_t)b * (T + 1) + i] = b * cap + (over ? 0 : deg[i]);
        if (rowT_ptr) rowT_ptr[(size_t)b * (T + 1) + i] = b * cap + (over ? 0 : degT[i]);
    }
    if (t == 0) {
        status[b] = over ? GCNPT_E_CAPACITY : 0;
        atomicMax(&status[B], T);
    }
    // ELL heads start as "count = 0"; the fill below overwrites the rows that have entries
    for (int i = t; i < T * 8; i += ADJ_THREADS) {
        ell[(size_t)b * T * 8 + i] = 0;
        if (ellT) ellT[(size_t)b * T * 8 + i] = 0;
    }
    __syncthreads();
    if (over) return;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = wave; r < T; r += NW) {
        const int o0 = b * cap + deg[r], oT0 = b * cap + degT[r];
        int o = o0, oT = oT0;
        int32_t* e = ell + ((size_t)b * T + r) * 8;
        int32_t* eT = ellT ? ellT + ((size_t)b * T + r) * 8 : nullptr;
        for (int c0 = 0; c0 < T; c0 += WAVE) {
            const int c = c0 + lane;
            const float v = c < T ? A[(size_t)r * T + c] : 0.0f;
            const float vT = c < T ? A[(size_t)c * T + r] : 0.0f;
            const bool nz = c < T && v != 0.0f, nzT = c < T && vT != 0.0f;
            const unsigned long long m = __ballot(nz), mT = __ballot(nzT);
            if (nz) {
                const int k = o + __popcll(m & lt);
                col_idx[k] = c; if (label) label[k] = (int)v;
                if (k - o0 < 7) e[1 + k - o0] = c;
            }
            if (nzT) {
                const int k = oT + __popcll(mT & lt);
                if (colT_idx) colT_idx[k] = c;
                if (eT && k - oT0 < 7) eT[1 + k - oT0] = c;
            }
            o += __popcll(m);
            oT += __popcll(mT);
        }
        if (lane == 0) { e[0] = o - o0; if (eT) eT[0] = oT - oT0; }
    }
}

__global__ void csr_to_adj_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx,
                                  const int32_t* __restrict__ label, int B, int T, float* __restrict__ adj) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * T) return;
    const int b = r / T, i = r - b * T;
    const int beg = row_ptr[(size_t)b * (T + 1) + i], end = row_ptr[(size_t)b * (T + 1) + i + 1];
    for (int e = beg; e < end; ++e)
        adj[((size_t)b * T + i) * T + col_idx[e]] = label ? (float)label[e] : 1.0f;
}

}  // namespace gcnpt

using namespace gcnpt;

// the padded layout as the pruner's destination: no cu, the mask and the status in the padded layout's two members
static PackedDst padded_dst(const TreeArrays& a) {
    PackedDst d{};
    d.row_ptr = a.row_ptr; d.col_idx = a.col_idx; d.label = a.label; d.rowT_ptr = a.rowT_ptr; d.colT_idx = a.colT_idx;
    d.ell = a.ell; d.ellT = a.ellT; d.pool_mask_padded = a.pool_mask; d.sent_status = a.status;
    return d;
}

// dst.cu == NULL: the padded layout, cap entries per sentence (sync unused)
static int prune_impl(void* stream, const ParseSrc& in, const int32_t* len, int B, int T, int prune_k, int cap, const PackedDst& dst, uint64_t* sync,
                      const SideJob& sj) {
    GCNPT_REQUIRE(in.head && in.subj_pos && in.obj_pos && in.deprel && (in.pad_mask || len), "prune_to_csr: null input pointer");
    GCNPT_REQUIRE(dst.row_ptr && dst.col_idx && dst.ell && dst.sent_status, "prune_to_csr: null output pointer");
    const int rc = check_transposed("prune_to_csr", dst.rowT_ptr, dst.colT_idx, dst.ellT);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(B > 0 && T > 0 && cap > 0, "prune_to_csr: B, T, cap must be positive (B=%d T=%d cap=%d)", B, T, cap);
    if (prune_k < 0)
        return fail(GCNPT_E_PRUNE_NEGATIVE, "prune_k=%d: the reference fork only works with prune_k >= 0 "
                    "(model/tree.py:194 reads Tree.head, which the unpruned branch never sets)", prune_k);
    if ((long long)B * cap > 0x7fffffffLL) return fail(GCNPT_E_UNSUPPORTED, "prune_to_csr: B*cap overflows int32");
    // the staged row emission when its entry lists still fit LDS (T <= ~2900)
    const int staged = PruneLds::bytes(T, true) <= 160 * 1024 - 256 ? 1 : 0;
    const size_t lds = PruneLds::bytes(T, staged);
    if (T > PRUNE_MAX_T) return fail(GCNPT_E_UNSUPPORTED, "prune_to_csr: T=%d exceeds the %d tokens a sentence may have", T, PRUNE_MAX_T);
    hipStream_t s = (hipStream_t)stream;
    // sentences beyond ~2300 tokens need more than the default 64 KB of LDS; minus the kernel's few static words
    if (lds > 64 * 1024) GCNPT_LDS_ATTR_ONCE(prune_to_csr_kernel, 160 * 1024 - 256);
    if (longest_by_atomic(B, T)) GCNPT_HIP_CHECK(hipMemsetAsync(dst.sent_status + B, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(prune_to_csr_kernel, dim3(B + sj.blocks), dim3(PRUNE_THREADS), lds, s, in, len, B, T, prune_k, cap, dst,
                       reinterpret_cast<unsigned long long*>(sync), static_cast<unsigned long long*>(g_debug_stamps), sj.pk, sj.dtype, staged);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_prune_to_csr(void* stream, const int64_t* head, const int64_t* subj_pos, const int64_t* obj_pos,
                                  const int64_t* deprel, const uint8_t* pad_mask, const int32_t* len, int B, int T,
                                  int prune_k, int cap, int32_t* row_ptr, int32_t* col_idx, int32_t* label,
                                  int32_t* rowT_ptr, int32_t* colT_idx, int32_t* ell, int32_t* ellT, uint8_t* pool_mask,
                                  int32_t* status) {
    const TreeArrays out{row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, status};
    return prune_impl(stream, ParseSrc{head, subj_pos, obj_pos, deprel, pad_mask}, len, B, T, prune_k, cap, padded_dst(out), nullptr, SideJob{});
}

extern "C" int gcnpt_prune_to_csr_pack(void* stream, const int64_t* head, const int64_t* subj_pos, const int64_t* obj_pos,
                                       const int64_t* deprel, const uint8_t* pad_mask, const int32_t* len, int B, int T,
                                       int prune_k, int cap, int32_t* row_ptr, int32_t* col_idx, int32_t* label,
                                       int32_t* rowT_ptr, int32_t* colT_idx, int32_t* ell, int32_t* ellT, uint8_t* pool_mask,
                                       int32_t* status, int n_layers, const float* const* W, const int* H, const int* Din, int dtype,
                                       void* const* w_fwd, void* const* w_bwd) {
    SideJob sj;
    const int rc = side_job(sj, false, PRUNE_THREADS, n_layers, W, H, Din, dtype, w_fwd, w_bwd);
    if (rc != GCNPT_OK) return rc;
    const TreeArrays out{row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, status};
    return prune_impl(stream, ParseSrc{head, subj_pos, obj_pos, deprel, pad_mask}, len, B, T, prune_k, cap, padded_dst(out), nullptr, sj);
}

// The pruner writing the token-packed layout itself (what gcnpt_pack_trees makes of gcnpt_prune_to_csr's arrays, bit for bit), optionally
// with the weight pack as a side job: one launch instead of two (three with the pack).
extern "C" int gcnpt_prune_to_csr_packed(void* stream, const int64_t* head, const int64_t* subj_pos, const int64_t* obj_pos,
                                         const int64_t* deprel, const uint8_t* pad_mask, const int32_t* len, int B, int T, int prune_k,
                                         int32_t* cu_seqlens, int32_t* row_ptr, int32_t* col_idx, int32_t* label, int32_t* rowT_ptr,
                                         int32_t* colT_idx, int32_t* ell, int32_t* ellT, uint8_t* pool_mask, int32_t* row_sent, int n_rows,
                                         int nnz_cap, int32_t* status, int32_t* sent_status, uint8_t* pool_mask_padded, uint64_t* sync_ws,
                                         int n_layers, const float* const* W, const int* H, const int* Din, int dtype, void* const* w_fwd,
                                         void* const* w_bwd) {
    GCNPT_REQUIRE(cu_seqlens && row_sent && status && sent_status && sync_ws && pool_mask, "prune_to_csr_packed: null pointer");
    GCNPT_REQUIRE(n_rows > 0 && nnz_cap > 0, "prune_to_csr_packed: n_rows and nnz_cap must be positive");
    GCNPT_REQUIRE(T <= 0xffff && 3 * (long long)T < (1 << 20), "prune_to_csr_packed: T=%d too long", T);
    SideJob sj;
    const int rc = side_job(sj, true, PRUNE_THREADS, n_layers, W, H, Din, dtype, w_fwd, w_bwd);
    if (rc != GCNPT_OK) return rc;
    const PackedDst dst{cu_seqlens, row_ptr, col_idx, label, rowT_ptr, colT_idx, ell, ellT, pool_mask, row_sent, status, n_rows, nnz_cap,
                        pool_mask_padded, sent_status};
    return prune_impl(stream, ParseSrc{head, subj_pos, obj_pos, deprel, pad_mask}, len, B, T, prune_k, 3 * T, dst, sync_ws, sj);
}

extern "C" int gcnpt_adj_to_csr(void* stream, const float* adj, int B, int T, int cap, int32_t* row_ptr,
                                int32_t* col_idx, int32_t* label, int32_t* rowT_ptr, int32_t* colT_idx, int32_t* ell,
                                int32_t* ellT, uint8_t* pool_mask, int32_t* status) {
    GCNPT_REQUIRE(adj && row_ptr && col_idx && ell && status, "adj_to_csr: null pointer");
    const int rc = check_transposed("adj_to_csr", rowT_ptr, colT_idx, ellT);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(B > 0 && T > 0 && cap > 0, "adj_to_csr: B, T, cap must be positive");
    if ((long long)B * cap > 0x7fffffffLL) return fail(GCNPT_E_UNSUPPORTED, "adj_to_csr: B*cap overflows int32");
    const size_t lds = sizeof(int) * ((size_t)2 * T + 2 + ADJ_THREADS);
    if (lds > 150 * 1024) return fail(GCNPT_E_UNSUPPORTED, "adj_to_csr: T=%d needs %zu B of LDS", T, lds);
    hipStream_t s = (hipStream_t)stream;
    GCNPT_HIP_CHECK(hipMemsetAsync(status + B, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(adj_to_csr_kernel, dim3(B), dim3(ADJ_THREADS), lds, s, adj, B, T, cap, row_ptr, col_idx, label,
                       rowT_ptr, colT_idx, ell, ellT, pool_mask, status);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_csr_to_adj(void* stream, const int32_t* row_ptr, const int32_t* col_idx, const int32_t* label,
                                int B, int T, float* adj) {
    GCNPT_REQUIRE(row_ptr && col_idx && adj, "csr_to_adj: null pointer");
    GCNPT_REQUIRE(B > 0 && T > 0, "csr_to_adj: B and T must be positive");
    hipStream_t s = (hipStream_t)stream;
    GCNPT_HIP_CHECK(hipMemsetAsync(adj, 0, sizeof(float) * (size_t)B * T * T, s));
    const int rows = B * T;
    hipLaunchKernelGGL(csr_to_adj_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, s, row_ptr, col_idx, label, B, T, adj);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}
