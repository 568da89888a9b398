// The recurrence of the C-GCN model's bidirectional LSTM (reference model/gcn.py encode_with_rnn / rnn_zero_state: nn.LSTM over
// pack_padded_sequence), both directions in every launch, exact fp32 on v_mfma_f32_16x16x4_f32.  Only the step-to-step part lives here;
// the time-parallel products (Gx = x W_ih^T + b, dx, dW_ih, dW_hh, db) are library GEMMs in model/rnn.py.
//
// One launch per time step s, T launches enqueued back to back by one call; nothing inside a launch depends on another workgroup of
// the same launch (no spin-waits, no grid barrier).  A workgroup owns (direction d, 16 hidden units, 16 sentences); its 8 waves split
// the contraction and meet once in LDS, summed in a fixed order (run-to-run bit-identical).  A step is a latency chain, so every wave
// issues all its operand loads at once (one round trip for H <= 256) and the element-wise operands are requested before the contraction.  Sentence b with length len:
//   forward direction  works at t = s            for s < len
//   reverse direction  works at t = len - 1 - s  for s < len   (it starts at the sentence's own end, not at T - 1)
//   s >= len           both directions write the padding row t = s: y = c = h_prev = gates = 0 forward, dG = 0 backward
// so every row of every output is written exactly once per call and no buffer needs clearing.
//
// Layouts (rows r = b*T + t): gx / gates / dgates float32 [B*T, 8H] with column d*4H + g*H + u (gate order i, f, g, o: nn.LSTM's);
// y / c / h_prev float32 [B*T, 2H] with column d*H + u; dc float32 [2, B, H] (the cell gradient carried from step to step).
#include "gcnpt_common.h"

namespace gcnpt {

constexpr int LSTM_TILE = 16, LSTM_WAVES = 8, LSTM_THREADS = LSTM_WAVES * WAVE;
constexpr int FWD_BATCH = 8, BWD_BATCH = 32;     // k-blocks of 4 whose loads a wave has in flight at once: 8 waves x 8 (x 32) blocks = H (4H) <= 256 (1024)

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ int clamp_len(const int32_t* lens, int b, int T) { return min(max(lens[b], 0), T); }

// step s: pre = Gx[t] + h_prev . W_hh^T for the 4 gate rows of 16 units; c = f c_prev + i g; h = o tanh(c).  h_prev is read from y at the
// row the previous launch wrote (t - 1 forward, t + 1 reverse).  gates / h_prev may be NULL (inference: nothing saved for backward).
__global__ __launch_bounds__(LSTM_THREADS) void lstm_fwd_step_kernel(const float* __restrict__ gx, const float* __restrict__ whh_f,
                                                                    const float* __restrict__ whh_r, const int32_t* __restrict__ lens,
                                                                    int B, int T, int H, int s, float* __restrict__ y, float* __restrict__ c,
                                                                    float* __restrict__ gates, float* __restrict__ h_prev) {
    __shared__ float part[LSTM_WAVES][4][LSTM_TILE * LSTM_TILE];
    const int d = blockIdx.x & 1, ut = blockIdx.x >> 1, bt = blockIdx.y;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int li = lane & 15, kq = lane >> 4;
    const int H2 = 2 * H, G8 = 8 * H;
    const float* __restrict__ W = d ? whh_r : whh_f;

    // the element-wise phase's own operands (thread -> sentence row = tid / 16, unit col = tid % 16; the first 4 waves), requested first
    const int row = threadIdx.x / LSTM_TILE, col = threadIdx.x % LSTM_TILE;
    const int b = bt * LSTM_TILE + row, u = ut * LSTM_TILE + col;
    const bool mine = threadIdx.x < LSTM_TILE * LSTM_TILE && b < B && u < H;
    const int len = mine ? clamp_len(lens, b, T) : 0;
    const bool live = mine && s < len;
    const int t = d ? len - 1 - s : s, tp = s > 0 ? (d ? t + 1 : t - 1) : t;     // tp: the row written one launch before (s > 0 only)
    const size_t rg = (size_t)(b * T + t) * G8 + d * 4 * H + u;
    const size_t o = (size_t)(b * T + t) * H2 + d * H + u, op = (size_t)(b * T + tp) * H2 + d * H + u;
    float gxv[4] = {0.f, 0.f, 0.f, 0.f}, cp = 0.f, hp = 0.f;
    if (live) {
#pragma unroll
        for (int g = 0; g < 4; ++g) gxv[g] = gx[rg + g * H];
        if (s > 0) {
            cp = c[op];
            hp = y[op];
        }
    }

    // 16x16x4 f32 operands: lane l holds A[l&15][k = l>>4] (h_prev of sentence bt*16 + (l&15)) and B[k][l&15] (W_hh row of unit ut*16 + (l&15))
    f32x4_t acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
        const int ba = bt * LSTM_TILE + li;
        const float* hrow = nullptr;
        if (ba < B) {
            const int lb = clamp_len(lens, ba, T);
            if (s < lb) hrow = y + (size_t)(ba * T + (d ? lb - s : s - 1)) * H2 + d * H;
        }
        const int ub = ut * LSTM_TILE + li;
        const float* wrow = ub < H ? W + (size_t)ub * H : nullptr;
        const size_t gstride = (size_t)H * H;
        for (int kb0 = wave; kb0 * 4 < H; kb0 += LSTM_WAVES * FWD_BATCH) {      // trip count is uniform over the wave
            float a[FWD_BATCH], w[FWD_BATCH][4];
#pragma unroll
            for (int j = 0; j < FWD_BATCH; ++j) {
                const int k = (kb0 + j * LSTM_WAVES) * 4 + kq;
                const bool kin = k < H;
                a[j] = (hrow && kin) ? hrow[k] : 0.f;
#pragma unroll
                for (int g = 0; g < 4; ++g) w[j][g] = (wrow && kin) ? wrow[g * gstride + k] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < FWD_BATCH; ++j) {
                if ((kb0 + j * LSTM_WAVES) * 4 >= H) break;                       // uniform: no MFMA on an all-zero block
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w[j][g], acc[g], 0, 0, 0);
            }
        }
    }
    // C/D: column (unit) = lane & 15, row (sentence) = (lane >> 4) * 4 + register
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][g][(kq * 4 + r) * LSTM_TILE + li] = acc[g][r];
    __syncthreads();

    if (!mine) return;
    if (!live) {                                      // padding row t = s of this direction
        const size_t oz = (size_t)(b * T + s) * H2 + d * H + u;
        y[oz] = 0.f;
        c[oz] = 0.f;
        if (gates) {
            const size_t rz = (size_t)(b * T + s) * G8 + d * 4 * H + u;
#pragma unroll
            for (int g = 0; g < 4; ++g) gates[rz + g * H] = 0.f;
        }
        if (h_prev) h_prev[oz] = 0.f;
        return;
    }
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < LSTM_WAVES; ++w) v += part[w][g][threadIdx.x];
        pre[g] = gxv[g] + v;
    }
    const float ig = sigmoidf(pre[0]), fg = sigmoidf(pre[1]), gg = tanhf(pre[2]), og = sigmoidf(pre[3]);
    const float cc = fg * cp + ig * gg;
    y[o] = og * tanhf(cc);
    c[o] = cc;
    if (gates) {
        gates[rg] = ig;
        gates[rg + H] = fg;
        gates[rg + 2 * H] = gg;
        gates[rg + 3 * H] = og;
    }
    if (h_prev) h_prev[o] = hp;
}

// step s, launched for s = T-1 ... 0:  dh = dY[t] + dG[t_next] . W_hh  (K = 4H: the whole gate gradient of the previous launch), then the
// cell gradient (carried in dc, per unit, in place) and this step's gate gradient dG[t] for the workgroup's own units.
__global__ __launch_bounds__(LSTM_THREADS) void lstm_bwd_step_kernel(const float* __restrict__ dy, const float* __restrict__ whh_f,
                                                                    const float* __restrict__ whh_r, const int32_t* __restrict__ lens,
                                                                    int B, int T, int H, int s, const float* __restrict__ c,
                                                                    const float* __restrict__ gates, float* __restrict__ dgates,
                                                                    float* __restrict__ dc) {
    __shared__ float part[LSTM_WAVES][LSTM_TILE * LSTM_TILE];
    const int d = blockIdx.x & 1, ut = blockIdx.x >> 1, bt = blockIdx.y;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int li = lane & 15, kq = lane >> 4;
    const int H2 = 2 * H, G8 = 8 * H;
    const float* __restrict__ W = d ? whh_r : whh_f;

    // the element-wise phase's own operands (first 4 waves), requested before the contraction
    const int row = threadIdx.x / LSTM_TILE, col = threadIdx.x % LSTM_TILE;
    const int b = bt * LSTM_TILE + row, u = ut * LSTM_TILE + col;
    const bool mine = threadIdx.x < LSTM_TILE * LSTM_TILE && b < B && u < H;
    const int len = mine ? clamp_len(lens, b, T) : 0;
    const bool live = mine && s < len;
    const int t = d ? len - 1 - s : s, tp = s > 0 ? (d ? t + 1 : t - 1) : t;     // tp: the row of the step before (s > 0 only)
    const size_t o = (size_t)(b * T + t) * H2 + d * H + u;
    const size_t rg = (size_t)(b * T + t) * G8 + d * 4 * H + u;
    float* dcp = dc + (size_t)(d * B + b) * H + u;
    float dyv = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cv = 0.f, cp = 0.f, carry = 0.f;
    if (live) {
        dyv = dy[o];
        ig = gates[rg]; fg = gates[rg + H]; gg = gates[rg + 2 * H]; og = gates[rg + 3 * H];
        cv = c[o];
        if (s > 0) cp = c[(size_t)(b * T + tp) * H2 + d * H + u];
        if (s + 1 < T) carry = *dcp;                  // written by the launch of step s + 1 (0 there if s + 1 >= len)
    }

    // lane l holds A[l&15][k] = dG[t_next] of sentence bt*16 + (l&15), gate column k; B[k][l&15] = W_hh[k][unit ut*16 + (l&15)]
    f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (s + 1 < T) {
        const int ba = bt * LSTM_TILE + li;
        const float* grow = nullptr;
        if (ba < B) {
            const int lb = clamp_len(lens, ba, T);
            if (s + 1 < lb) grow = dgates + (size_t)(ba * T + (d ? lb - 2 - s : s + 1)) * G8 + d * 4 * H;
        }
        const int ub = ut * LSTM_TILE + li;
        const float* wcol = ub < H ? W + ub : nullptr;
        for (int kb0 = wave; kb0 < H; kb0 += LSTM_WAVES * BWD_BATCH) {        // 4H gate columns = H blocks of 4
            float a[BWD_BATCH], w[BWD_BATCH];
#pragma unroll
            for (int j = 0; j < BWD_BATCH; ++j) {
                const int kb = kb0 + j * LSTM_WAVES;
                const int k = min(kb, H - 1) * 4 + kq;                            // blocks past the end load block H-1 and are not used
                a[j] = grow ? grow[k] : 0.f;
                w[j] = wcol ? wcol[(size_t)k * H] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < BWD_BATCH; ++j) {
                if (kb0 + j * LSTM_WAVES >= H) break;                             // uniform
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w[j], acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][(kq * 4 + r) * LSTM_TILE + li] = acc[r];
    __syncthreads();

    if (!mine) return;
    if (!live) {                                      // padding row t = s: no gradient, and the carry into step len-1 starts at 0
        const size_t rz = (size_t)(b * T + s) * G8 + d * 4 * H + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) dgates[rz + g * H] = 0.f;
        *dcp = 0.f;
        return;
    }
    float dh = 0.f;
#pragma unroll
    for (int w = 0; w < LSTM_WAVES; ++w) dh += part[w][threadIdx.x];
    dh += dyv;
    const float tc = tanhf(cv);
    const float dcc = carry + dh * og * (1.f - tc * tc);
    dgates[rg] = dcc * gg * ig * (1.f - ig);
    dgates[rg + H] = dcc * cp * fg * (1.f - fg);
    dgates[rg + 2 * H] = dcc * ig * (1.f - gg * gg);
    dgates[rg + 3 * H] = dh * tc * og * (1.f - og);
    *dcp = dcc * fg;
}

static int lstm_check(const char* what, const void* w_hh_f, const void* w_hh_r, const void* lens, int B, int T, int H, int gx_cols) {
    GCNPT_REQUIRE(w_hh_f && w_hh_r && lens, "%s: null pointer", what);
    GCNPT_REQUIRE(B >= 1 && T >= 1, "%s: B and T must be positive (B=%d T=%d)", what, B, T);
    GCNPT_REQUIRE(H >= 1, "%s: hidden size must be >= 1 (H=%d)", what, H);
    GCNPT_REQUIRE(gx_cols == 8 * (long long)H, "%s: gate rows have %d columns, the two directions' 4 gates of H=%d need %lld", what, gx_cols,
                  H, 8 * (long long)H);
    // 32-bit row indices inside the kernels; H*H weight offsets are size_t
    if ((long long)B * T * 8 * H > 0x7fffffffLL || (long long)B * T > 0x7fffffffLL)
        return fail(GCNPT_E_UNSUPPORTED, "%s: B*T*8H = %lld elements is beyond the kernels' 32-bit row indexing", what, (long long)B * T * 8 * H);
    return GCNPT_OK;
}

}  // namespace gcnpt

using namespace gcnpt;

extern "C" int gcnpt_lstm_fwd(void* stream, const float* gx, int gx_cols, const float* w_hh_f, const float* w_hh_r, const int32_t* lens,
                              int B, int T, int H, float* y, float* c, float* gates, float* h_prev) {
    int rc = lstm_check("lstm_fwd", w_hh_f, w_hh_r, lens, B, T, H, gx_cols);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(gx && y && c, "lstm_fwd: null pointer (gx, y and c are required)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(2 * ceil_div(H, LSTM_TILE), ceil_div(B, LSTM_TILE));
    for (int s = 0; s < T; ++s) {
        hipLaunchKernelGGL(lstm_fwd_step_kernel, grid, dim3(LSTM_THREADS), 0, st, gx, w_hh_f, w_hh_r, lens, B, T, H, s, y, c, gates, h_prev);
        GCNPT_HIP_CHECK(hipGetLastError());
    }
    return GCNPT_OK;
}

extern "C" int gcnpt_lstm_bwd(void* stream, const float* dy, const float* w_hh_f, const float* w_hh_r, const int32_t* lens, int B, int T,
                              int H, const float* c, const float* gates, int gates_cols, float* dgates, float* dc) {
    int rc = lstm_check("lstm_bwd", w_hh_f, w_hh_r, lens, B, T, H, gates_cols);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(dy && c && gates && dgates && dc, "lstm_bwd: null pointer (dy, c, gates, dgates and dc are required)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(2 * ceil_div(H, LSTM_TILE), ceil_div(B, LSTM_TILE));
    for (int s = T - 1; s >= 0; --s) {
        hipLaunchKernelGGL(lstm_bwd_step_kernel, grid, dim3(LSTM_THREADS), 0, st, dy, w_hh_f, w_hh_r, lens, B, T, H, s, c, gates, dgates, dc);
        GCNPT_HIP_CHECK(hipGetLastError());
    }
    return GCNPT_OK;
}
