// Evaluation of a split on the device (reference model/trainer.py:112-124, train.py:245-285, utils/scorer.py:20-96) for gfx950: one launch
// per batch scores its rows where the dataset's order wants them, one finishing launch turns the accumulators into the numbers the
// reference logs.  The host reads one small result at the end, nothing in between.
//
//   eval_batch    per row m with sentence s = idx[m]:  pred[s] = argmax (lowest index on ties),  probs[s,:] = softmax (optional),
//                 row_loss[s] = -log softmax(z_m)[y_m],  seen[s] += 1,  confusion[y_m, pred] += 1   -- a wave per row, no cross-row work
//   eval_finish   by_relation [3,C] = diagonal / column sums / row sums of confusion with the no_relation class forced to 0 (the four
//                 branches of scorer.py:30-40), totals, and loss / precision / recall / F1 in double (scorer.py:84-92 literally)
//
// The accumulators take int32 INTEGER atomics only, so the counts are exact whatever the arrival order; the one floating-point sum (the
// mean loss) runs in a fixed order in the finishing launch: bit-identical run to run.  Per row the softmax statistics and the argmax are
// head_common.h's, the same code as gcnpt_head_loss_fwd: the same bits.
#include "head_common.h"

namespace gcnpt {

constexpr int EV_THREADS = 256, EV_WAVES = EV_THREADS / WAVE;        // eval_batch: a wave per row, 4 rows per workgroup
constexpr int EF_THREADS = 1024, EF_WAVES = EF_THREADS / WAVE;       // eval_finish: ONE workgroup
constexpr int EF_GROUP = 32;                                         // the loss partials are summed 32 at a time, then the 32 group sums
constexpr int EV_MAX_C = 1024;

__global__ __launch_bounds__(EV_THREADS) void eval_batch_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                               const int64_t* __restrict__ idx, const int32_t* __restrict__ slot_status,
                                                               int M, int C, int S, int64_t* __restrict__ pred, float* __restrict__ probs,
                                                               float* __restrict__ row_loss, int32_t* __restrict__ seen,
                                                               int32_t* __restrict__ confusion, int32_t* __restrict__ status) {
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int m = blockIdx.x * EV_WAVES + wave;
    if (m >= M) return;                                               // uniform over the wave; nothing below synchronises the workgroup
    const int64_t s64 = idx[m];
    const int slot = slot_status ? slot_status[m] : 0;
    if (slot != 0 || s64 < 0 || s64 >= S) return;                     // an empty slot (the padded tail of a fixed-size batch): nothing read or written
    const size_t s = (size_t)s64;
    const float* z = logits + (size_t)m * C;
    float mx, den;
    row_softmax_stats(z, C, lane, mx, den);
    if (probs) {
        const float inv = 1.0f / den;
        for (int c = lane; c < C; c += WAVE) probs[s * C + c] = expf(z[c] - mx) * inv;
    }
    const int best = row_argmax(z, C, lane, mx);
    if (lane != 0) return;
    pred[s] = best;
    const long long yl = labels[m];
    const bool ok = yl >= 0 && yl < C;
    const float zy = z[ok ? (int)yl : 0];
    row_loss[s] = ok ? (mx - zy) + logf(den) : 0.f;                 // (mx - zy first: exact, however large the logits are)
    if (ok) {
        atomicAdd(seen + s, 1);
        atomicAdd(confusion + (size_t)yl * C + best, 1);
    } else if (status) {
        atomicOr(status, 1);
    }
}

// sum of one int per thread over the workgroup (exact); every thread gets the total.  `red` holds EF_WAVES ints
__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    __syncthreads();                                                  // (the previous use of `red` is over)
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    int t = 0;
    for (int q = 0; q < EF_WAVES; ++q) t += red[q];
    return t;
}

__global__ __launch_bounds__(EF_THREADS) void eval_finish_kernel(const int32_t* __restrict__ confusion, const int32_t* __restrict__ seen,
                                                                const float* __restrict__ row_loss, int C, int S, int no_relation,
                                                                int32_t* __restrict__ by_relation, int32_t* __restrict__ totals,
                                                                double* __restrict__ metrics) {
    __shared__ int red[EF_WAVES];
    __shared__ double part[EF_THREADS], group[EF_THREADS / EF_GROUP];
    const int t = threadIdx.x, wave = t / WAVE, lane = t % WAVE;
    // row sums (gold): a wave per row, its lanes on consecutive columns
    int scored = 0, n_gold = 0;
    for (int r = wave; r < C; r += EF_WAVES) {
        int v = 0;
        for (int c = lane; c < C; c += WAVE) v += confusion[(size_t)r * C + c];
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
        const int kept = r == no_relation ? 0 : v;
        if (lane == 0) {
            by_relation[2 * C + r] = kept;
            scored += v;
            n_gold += kept;
        }
    }
    // column sums (guessed) and the diagonal (correct): a thread per column, consecutive threads on consecutive columns of each row
    int n_guessed = 0, n_correct = 0;
    for (int c = t; c < C; c += EF_THREADS) {
        int v = 0;
        for (int r = 0; r < C; ++r) v += confusion[(size_t)r * C + c];
        const bool excluded = c == no_relation;
        const int diag = excluded ? 0 : confusion[(size_t)c * C + c];
        v = excluded ? 0 : v;
        by_relation[c] = diag;
        by_relation[C + c] = v;
        n_guessed += v;
        n_correct += diag;
    }
    // sentences: how many were scored, and their losses in a fixed order -- thread t takes sentences t, t + 1024, ... in order
    int n_seen = 0;
    double acc = 0.0;
    for (int s = t; s < S; s += EF_THREADS) {
        const bool in = seen[s] > 0;
        n_seen += in;
        if (in) acc += (double)row_loss[s];
    }
    part[t] = acc;
    scored = block_sum_int(scored, red);
    n_gold = block_sum_int(n_gold, red);
    n_guessed = block_sum_int(n_guessed, red);
    n_correct = block_sum_int(n_correct, red);
    n_seen = block_sum_int(n_seen, red);                              // (its barriers also publish part[])
    if (t < EF_THREADS / EF_GROUP) {                                  // thread order: partials 32 t .. 32 t + 31, then the group sums
        double g = 0.0;
        for (int q = 0; q < EF_GROUP; ++q) g += part[t * EF_GROUP + q];
        group[t] = g;
    }
    __syncthreads();
    if (t != 0) return;
    double total = 0.0;
    for (int q = 0; q < EF_THREADS / EF_GROUP; ++q) total += group[q];
    totals[0] = scored;
    totals[1] = n_seen;
    totals[2] = n_correct;
    totals[3] = n_guessed;
    totals[4] = n_gold;
    totals[5] = S - n_seen;
    // scorer.py:84-92
    double p = 1.0, r = 0.0, f = 0.0;
    if (n_guessed > 0) p = (double)n_correct / (double)n_guessed;
    if (n_gold > 0) r = (double)n_correct / (double)n_gold;
    if (p + r > 0.0) f = 2.0 * p * r / (p + r);
    metrics[0] = n_seen > 0 ? total / (double)n_seen : 0.0;
    metrics[1] = p;
    metrics[2] = r;
    metrics[3] = f;
}

static int eval_check(const char* what, int C, int S, int no_relation) {
    GCNPT_REQUIRE(C >= 1 && S >= 1, "%s: C and S must be positive (C=%d S=%d)", what, C, S);
    GCNPT_REQUIRE(no_relation >= -1 && no_relation < C, "%s: no_relation = %d is outside [-1, C = %d)", what, no_relation, C);
    if (C > EV_MAX_C) return fail(GCNPT_E_UNSUPPORTED, "%s: at most %d classes (C=%d; the confusion matrix is C*C int32)", what, EV_MAX_C, C);
    return GCNPT_OK;
}

}  // namespace gcnpt

using namespace gcnpt;

extern "C" int gcnpt_eval_batch(void* stream, const float* logits, const int64_t* labels, const int64_t* idx, const int32_t* slot_status, int M,
                                int C, int S, int no_relation, int64_t* pred, float* probs, float* row_loss, int32_t* seen,
                                int32_t* confusion, int32_t* status) {
    GCNPT_REQUIRE(logits && labels && idx, "gcnpt_eval_batch: null input pointer (logits, labels and idx are required)");
    GCNPT_REQUIRE(pred && row_loss && seen && confusion, "gcnpt_eval_batch: null output pointer (pred, row_loss, seen and confusion are required)");
    GCNPT_REQUIRE(M >= 1, "gcnpt_eval_batch: M must be positive (M=%d)", M);
    const int rc = eval_check("gcnpt_eval_batch", C, S, no_relation);
    if (rc != GCNPT_OK) return rc;
    hipLaunchKernelGGL(eval_batch_kernel, dim3(ceil_div(M, EV_WAVES)), dim3(EV_THREADS), 0, (hipStream_t)stream, logits, labels, idx,
                       slot_status, M, C, S, pred, probs, row_loss, seen, confusion, status);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_eval_finish(void* stream, const int32_t* confusion, const int32_t* seen, const float* row_loss, int C, int S,
                                 int no_relation, int32_t* by_relation, int32_t* totals, double* metrics) {
    GCNPT_REQUIRE(confusion && seen && row_loss, "gcnpt_eval_finish: null input pointer (confusion, seen and row_loss are required)");
    GCNPT_REQUIRE(by_relation && totals && metrics, "gcnpt_eval_finish: null output pointer (by_relation, totals and metrics are required)");
    const int rc = eval_check("gcnpt_eval_finish", C, S, no_relation);
    if (rc != GCNPT_OK) return rc;
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(EF_THREADS), 0, (hipStream_t)stream, confusion, seen, row_loss, C, S, no_relation,
                       by_relation, totals, metrics);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}
