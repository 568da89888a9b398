// The output head of GCNClassifier (reference model/gcn.py:31-36, 66-72, 122-125 and model/trainer.py:94-100, 119-120) for gfx950, everything
// float32: the out_mlp / classifier Linear (+ ReLU) layers and the trainer's loss, one launch each way, exact fp32 on v_mfma_f32_16x16x4_f32.
//
//   head_linear_fwd   Y[M,N] = act(X[M,K] . W^T + b)          W = nn.Linear.weight [N,K] as torch stores it (no pack launch)
//   head_linear_bwd   dZ = dY * 1[Y > 0] (ReLU) or dY;  dX = dZ . W,  dW = dZ^T . X,  db = sum_rows dZ     -- ONE launch: the dX tiles and the
//                     dW / db tiles are different workgroups of the same grid (side jobs, not side streams)
//   head_loss_fwd     loss = mean_m(-log softmax(z_m)[y_m]) + l2 * mean_m sum_j pooled[m,j]^2,  probs, argmax, status
//   head_loss_bwd     dlogits = dloss * (softmax - onehot) / M,  dpooled = dloss * 2 l2 / M * pooled   (the softmax is recomputed from the logits)
//
// Nothing inside a launch waits on another workgroup of the same launch, no float atomics, no workspace, no clears: every output element
// has ONE owning workgroup that walks its whole contraction (K forward, N for dX, M for dW / db) in a fixed order, so results are
// bit-identical run to run.
//
// Loads: every operand block is read the way it lies in memory -- consecutive lanes on consecutive columns of a row, 16 bytes per lane
// where base and row stride allow -- into LDS, zero-filled outside the matrix, and the 16x16x4 operand layout (lane l: A[l & 15][k = l >> 4],
// B[k = l >> 4][l & 15]) is read from there; the LDS row strides put the 64 lanes of such a read on 64 different banks.  Addresses are
// clamped and values selected, so no load sits behind a bounds branch; only stores are guarded.
#include "head_common.h"

namespace gcnpt {

constexpr int HD_TILE = 16, HD_WAVES = 8, HD_THREADS = HD_WAVES * WAVE;
// forward: a (16 rows x 16 outputs) tile, the 8 waves split each 256-wide chunk of K and meet once in LDS
constexpr int HF_KC = 256, HF_STRIDE = HF_KC + 4;
// dX: a (16 rows x 32 inputs) tile, the 8 waves split each 128-wide chunk of N
constexpr int HX_NC = 128, HX_COLS = 32, HX_ZSTRIDE = HX_NC + 4, HX_WSTRIDE = HX_COLS + 16;
// dW / db: a (16 outputs x 128 inputs) tile, wave w owns input columns 16w .. 16w+15 and walks the whole of M in chunks of 64 rows
constexpr int HW_MC = 64, HW_COLS = HD_WAVES * HD_TILE, HW_ZSTRIDE = HD_TILE, HW_XSTRIDE = HW_COLS + 16;
constexpr int HD_PART = HD_TILE * HD_TILE;
constexpr int HD_LDS_FWD = 2 * HD_TILE * HF_STRIDE;
constexpr int HD_LDS_DX = HD_TILE * HX_ZSTRIDE + HX_NC * HX_WSTRIDE;
constexpr int HD_LDS_DW = HW_MC * HW_ZSTRIDE + HW_MC * HW_XSTRIDE;
constexpr int HD_LDS_BWD = HD_LDS_DX > HD_LDS_DW ? HD_LDS_DX : HD_LDS_DW;

// dst[r * stride + c] = src[r0 + r][c0 + c] (* 1[mask[r0 + r][c0 + c] > 0]) for r < R, c < C; 0 outside the [rows, cols] matrix.  src and
// mask have row stride ld; c0, C and stride are multiples of 4.  Consecutive threads take consecutive 4-column groups of a row.
template <int R, int C>
__device__ __forceinline__ void stage_block(float* __restrict__ dst, int stride, const float* __restrict__ src, const float* __restrict__ mask,
                                            size_t ld, int rows, int cols, int r0, int c0) {
    const bool vec = (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(mask)) & 15) == 0) && (ld & 3) == 0;
    constexpr int G = C / 4;
    for (int q = threadIdx.x; q < R * G; q += HD_THREADS) {
        const int r = q / G, c = (q % G) * 4;
        const int gr = r0 + r, gc = c0 + c;
        const bool rin = gr < rows;
        const size_t base = (size_t)min(gr, rows - 1) * ld;
        float v[4], m[4] = {1.f, 1.f, 1.f, 1.f};
        if (vec && gc + 3 < cols) {
            const float4 t = *reinterpret_cast<const float4*>(src + base + gc);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            if (mask) {
                const float4 u = *reinterpret_cast<const float4*>(mask + base + gc);
                m[0] = u.x; m[1] = u.y; m[2] = u.z; m[3] = u.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const size_t o = base + min(gc + e, cols - 1);
                const float t = src[o];
                v[e] = gc + e < cols ? t : 0.f;
                if (mask) m[e] = mask[o];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (rin && m[e] > 0.f) ? v[e] : 0.f;
        *reinterpret_cast<float4*>(dst + r * stride + c) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

__device__ __forceinline__ f32x4_t mfma4(float a, float b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(HD_THREADS) void head_linear_fwd_kernel(const float* __restrict__ x, size_t ldx, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, float* __restrict__ y, int M, int K, int N,
                                                                    int relu) {
    __shared__ __attribute__((aligned(16))) float lds[HD_LDS_FWD];
    float* xs = lds;
    float* ws = lds + HD_TILE * HF_STRIDE;
    const int nt = blockIdx.x, mt = blockIdx.y;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE, li = lane & 15, kq = lane >> 4;
    f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
    for (int k0 = 0; k0 < K; k0 += HF_KC) {
        stage_block<HD_TILE, HF_KC>(xs, HF_STRIDE, x, nullptr, ldx, M, K, mt * HD_TILE, k0);
        stage_block<HD_TILE, HF_KC>(ws, HF_STRIDE, w, nullptr, (size_t)K, N, K, nt * HD_TILE, k0);
        __syncthreads();
        const int kw = wave * (HF_KC / HD_WAVES);                  // this wave's 32 columns of the chunk
#pragma unroll
        for (int j = 0; j < HF_KC / HD_WAVES / 4; ++j) {
            if (k0 + kw + 4 * j >= K) break;                        // uniform: no MFMA on an all-zero block
            const int kk = li * HF_STRIDE + kw + 4 * j + kq;
            acc[j & 1] = mfma4(xs[kk], ws[kk], acc[j & 1]);
        }
        __syncthreads();
    }
    // C/D: column (output n) = lane & 15, row (m) = (lane >> 4) * 4 + register; the 8 partial tiles are summed in wave order
    float* part = lds;
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave * HD_PART + (kq * 4 + r) * HD_TILE + li] = acc[0][r] + acc[1][r];
    __syncthreads();
    if (threadIdx.x >= HD_PART) return;
    const int m = mt * HD_TILE + threadIdx.x / HD_TILE, n = nt * HD_TILE + threadIdx.x % HD_TILE;
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < HD_WAVES; ++q) v += part[q * HD_PART + threadIdx.x];
    v += bias[min(n, N - 1)];
    if (relu) v = fmaxf(v, 0.f);
    if (m < M && n < N) y[(size_t)m * N + n] = v;
}

// blocks [0, n_dx): dX tile (mt, kt) = (b / kx_tiles, b % kx_tiles); blocks [n_dx, ..): dW tile (nt, kt) with db from the kt = 0 tiles
__global__ __launch_bounds__(HD_THREADS) void head_linear_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                    const float* __restrict__ x, size_t ldx, const float* __restrict__ w,
                                                                    float* __restrict__ dx, size_t ld_dx, float* __restrict__ dw,
                                                                    float* __restrict__ db, int M, int K, int N, int n_dx, int kx_tiles,
                                                                    int kw_tiles) {
    __shared__ __attribute__((aligned(16))) float lds[HD_LDS_BWD];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE, li = lane & 15, kq = lane >> 4;
    if ((int)blockIdx.x < n_dx) {
        // dX[m, k] = sum_n dZ[m, n] W[n, k]: A = dZ rows (contiguous in n), B = W rows n x 32 columns k
        const int mt = blockIdx.x / kx_tiles, kt = blockIdx.x % kx_tiles;
        float* zs = lds;
        float* wt = lds + HD_TILE * HX_ZSTRIDE;
        f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
        for (int n0 = 0; n0 < N; n0 += HX_NC) {
            stage_block<HD_TILE, HX_NC>(zs, HX_ZSTRIDE, dy, y, (size_t)N, M, N, mt * HD_TILE, n0);
            stage_block<HX_NC, HX_COLS>(wt, HX_WSTRIDE, w, nullptr, (size_t)K, N, K, n0, kt * HX_COLS);
            __syncthreads();
            const int nw = wave * (HX_NC / HD_WAVES);              // this wave's 16 rows of the chunk
#pragma unroll
            for (int j = 0; j < HX_NC / HD_WAVES / 4; ++j) {
                if (n0 + nw + 4 * j >= N) break;                    // uniform
                const int nn = nw + 4 * j + kq;
                const float a = zs[li * HX_ZSTRIDE + nn];
                acc[0] = mfma4(a, wt[nn * HX_WSTRIDE + li], acc[0]);
                acc[1] = mfma4(a, wt[nn * HX_WSTRIDE + HD_TILE + li], acc[1]);
            }
            __syncthreads();
        }
        float* part = lds;                                           // [wave][column tile][16 x 16]
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(wave * 2 + t) * HD_PART + (kq * 4 + r) * HD_TILE + li] = acc[t][r];
        __syncthreads();
        if (threadIdx.x >= 2 * HD_PART) return;
        const int row = threadIdx.x / HX_COLS, col = threadIdx.x % HX_COLS;      // 32 consecutive columns of a row per half wave
        const int m = mt * HD_TILE + row, k = kt * HX_COLS + col;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < HD_WAVES; ++q) v += part[(q * 2 + col / HD_TILE) * HD_PART + row * HD_TILE + col % HD_TILE];
        if (m < M && k < K) dx[(size_t)m * ld_dx + k] = v;
        return;
    }
    // dW[n, k] = sum_m dZ[m, n] X[m, k]: A[n][m] = dZ^T, B = X rows m x 128 columns k; wave w owns columns 16w .. 16w + 15
    const int b = blockIdx.x - n_dx;
    const int nt = b / kw_tiles, kt = b % kw_tiles;
    float* zt = lds;
    float* xs = lds + HW_MC * HW_ZSTRIDE;
    f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
    float bsum = 0.f;
    const bool has_cols = kt * HW_COLS + wave * HD_TILE < K;         // uniform over the wave
    for (int m0 = 0; m0 < M; m0 += HW_MC) {
        stage_block<HW_MC, HD_TILE>(zt, HW_ZSTRIDE, dy, y, (size_t)N, M, N, m0, nt * HD_TILE);
        stage_block<HW_MC, HW_COLS>(xs, HW_XSTRIDE, x, nullptr, ldx, M, K, m0, kt * HW_COLS);
        __syncthreads();
        if (has_cols) {
#pragma unroll
            for (int j = 0; j < HW_MC / 4; ++j) {
                if (m0 + 4 * j >= M) break;                             // uniform
                const int mm = 4 * j + kq;
                acc[j & 1] = mfma4(zt[mm * HW_ZSTRIDE + li], xs[mm * HW_XSTRIDE + wave * HD_TILE + li], acc[j & 1]);
            }
        }
        if (kt == 0 && threadIdx.x < HD_TILE)                        // db: rows in order (rows past M are zero in LDS)
            for (int mm = 0; mm < HW_MC; ++mm) bsum += zt[mm * HW_ZSTRIDE + threadIdx.x];
        __syncthreads();
    }
    // C/D: column (input k) = lane & 15, row (output n) = (lane >> 4) * 4 + register
    const int k = kt * HW_COLS + wave * HD_TILE + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = nt * HD_TILE + kq * 4 + r;
        if (n < N && k < K) dw[(size_t)n * K + k] = acc[0][r] + acc[1][r];
    }
    if (kt == 0 && threadIdx.x < HD_TILE && nt * HD_TILE + (int)threadIdx.x < N) db[nt * HD_TILE + threadIdx.x] = bsum;
}

// ---- the loss ------------------------------------------------------------------------------------------------------------------------
constexpr int HL_THREADS = 1024, HL_WAVES = HL_THREADS / WAVE;      // forward: ONE workgroup, a wave per row, rows w, w + 16, ...
constexpr int HLB_THREADS = 256, HLB_WAVES = HLB_THREADS / WAVE;     // backward: a wave per row, 4 rows per workgroup

// (wave_max, wave_sum, row_softmax_stats and row_argmax: head_common.h, shared with eval_kernels.hip)

__global__ __launch_bounds__(HL_THREADS) void head_loss_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                  const float* __restrict__ pooled, size_t ldp, int H, float l2, int M, int C,
                                                                  float* __restrict__ loss, float* __restrict__ probs,
                                                                  int64_t* __restrict__ pred, int32_t* __restrict__ status) {
    __shared__ float s_ce[HL_WAVES], s_l2[HL_WAVES];
    __shared__ int s_bad[HL_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    float ce = 0.f, sq = 0.f;                                        // this wave's rows, in row order
    int bad = 0;
    for (int m = wave; m < M; m += HL_WAVES) {
        const float* z = logits + (size_t)m * C;
        float mx, den;
        row_softmax_stats(z, C, lane, mx, den);
        if (probs) {
            const float inv = 1.0f / den;
            for (int c = lane; c < C; c += WAVE) probs[(size_t)m * C + c] = expf(z[c] - mx) * inv;
        }
        if (pred) {                                                   // the lowest index that holds the maximum
            const int best = row_argmax(z, C, lane, mx);
            if (lane == 0) pred[m] = best;
        }
        if (labels) {
            const long long yl = labels[m];
            const bool ok = yl >= 0 && yl < C;
            const float zy = z[ok ? (int)yl : 0];
            ce += ok ? (mx - zy) + logf(den) : 0.f;                 // (mx - zy first: exact, however large the logits are)
            bad |= !ok;
        }
        if (pooled && l2 > 0.f) {
            float s = 0.f;
            for (int j = lane; j < H; j += WAVE) {
                const float p = pooled[(size_t)m * ldp + j];
                s += p * p;
            }
            sq += wave_sum(s);
        }
    }
    if (lane == 0) {
        s_ce[wave] = ce;
        s_l2[wave] = sq;
        s_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tc = 0.f, tl = 0.f;
        int tb = 0;
        for (int q = 0; q < HL_WAVES; ++q) {                         // wave order
            tc += s_ce[q];
            tl += s_l2[q];
            tb |= s_bad[q];
        }
        if (loss) *loss = tc / (float)M + l2 * (tl / (float)M);
        if (status) *status = tb;
    }
}

__global__ __launch_bounds__(HLB_THREADS) void head_loss_bwd_kernel(const float* __restrict__ dloss, const float* __restrict__ logits,
                                                                   const int64_t* __restrict__ labels, const float* __restrict__ pooled,
                                                                   size_t ldp, int H, float l2, int M, int C, float* __restrict__ dlogits,
                                                                   float* __restrict__ dpooled) {
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int m = blockIdx.x * HLB_WAVES + wave;
    if (m >= M) return;                                               // uniform over the wave; nothing below synchronises the workgroup
    const float g = *dloss / (float)M;
    if (dlogits) {
        const float* z = logits + (size_t)m * C;
        float mx, den;
        row_softmax_stats(z, C, lane, mx, den);
        const long long yl = labels[m];
        const bool ok = yl >= 0 && yl < C;                            // a label outside [0, C) contributed nothing: a zero row
        const float inv = 1.0f / den;
        for (int c = lane; c < C; c += WAVE) {
            const float p = expf(z[c] - mx) * inv;
            dlogits[(size_t)m * C + c] = ok ? g * (p - (c == (int)yl ? 1.f : 0.f)) : 0.f;
        }
    }
    if (dpooled) {
        const float s = g * (2.0f * l2);
        for (int j = lane; j < H; j += WAVE) dpooled[(size_t)m * H + j] = s * pooled[(size_t)m * ldp + j];
    }
}

static int linear_check(const char* what, const void* x, long long ldx, const void* w, int M, int K, int N, int relu) {
    GCNPT_REQUIRE(M >= 1 && K >= 1 && N >= 1, "%s: M, K and N must be positive (M=%d K=%d N=%d)", what, M, K, N);
    GCNPT_REQUIRE(x && w, "%s: null pointer (x and w are required)", what);
    GCNPT_REQUIRE(ldx >= K, "%s: row stride ldx = %lld is below K = %d", what, ldx, K);
    GCNPT_REQUIRE(relu == 0 || relu == 1, "%s: relu is 0 or 1 (got %d)", what, relu);
    // tile counts are 32-bit and the grid's x dimension holds the bwd launch's tiles
    GCNPT_REQUIRE((long long)ceil_div(M, HD_TILE) * ceil_div(K, HX_COLS) + (long long)ceil_div(N, HD_TILE) * ceil_div(K, HW_COLS) < (1ll << 31) &&
                      ceil_div(M, HD_TILE) <= 65535,
                  "%s: M=%d K=%d N=%d is beyond the kernels' tile indexing", what, M, K, N);
    return GCNPT_OK;
}

}  // namespace gcnpt

using namespace gcnpt;

extern "C" int gcnpt_head_linear_fwd(void* stream, const float* x, long long ldx, const float* w, const float* b, float* y, int M, int K, int N,
                                     int relu) {
    const int rc = linear_check("head_linear_fwd", x, ldx, w, M, K, N, relu);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(b && y, "head_linear_fwd: null pointer (b and y are required)");
    const dim3 grid(ceil_div(N, HD_TILE), ceil_div(M, HD_TILE));
    hipLaunchKernelGGL(head_linear_fwd_kernel, grid, dim3(HD_THREADS), 0, (hipStream_t)stream, x, (size_t)ldx, w, b, y, M, K, N, relu);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_head_linear_bwd(void* stream, const float* dy, const float* y, const float* x, long long ldx, const float* w, float* dx,
                                     long long ld_dx, float* dw, float* db, int M, int K, int N, int relu) {
    const int rc = linear_check("head_linear_bwd", x, ldx, w, M, K, N, relu);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(dy && dw && db, "head_linear_bwd: null pointer (dy, dw and db are required)");
    GCNPT_REQUIRE(!relu || y, "head_linear_bwd: the ReLU mask needs y");
    GCNPT_REQUIRE(!dx || ld_dx >= K, "head_linear_bwd: row stride ld_dx = %lld is below K = %d", ld_dx, K);
    const int kx_tiles = ceil_div(K, HX_COLS), kw_tiles = ceil_div(K, HW_COLS);
    const int n_dx = dx ? ceil_div(M, HD_TILE) * kx_tiles : 0, n_dw = ceil_div(N, HD_TILE) * kw_tiles;
    hipLaunchKernelGGL(head_linear_bwd_kernel, dim3(n_dx + n_dw), dim3(HD_THREADS), 0, (hipStream_t)stream, dy, relu ? y : nullptr, x,
                       (size_t)ldx, w, dx, (size_t)ld_dx, dw, db, M, K, N, n_dx, kx_tiles, kw_tiles);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

static int loss_check(const char* what, const void* logits, const void* pooled, long long ldp, int H, float l2, int M, int C) {
    GCNPT_REQUIRE(M >= 1 && C >= 1, "%s: M and C must be positive (M=%d C=%d)", what, M, C);
    GCNPT_REQUIRE(logits, "%s: null logits", what);
    GCNPT_REQUIRE(l2 >= 0.0f, "%s: l2 must be >= 0 (got %g)", what, (double)l2);      // (a NaN fails this too)
    GCNPT_REQUIRE(!pooled || (H >= 1 && ldp >= H), "%s: pooled needs H >= 1 and a row stride ldp >= H (H=%d ldp=%lld)", what, H, ldp);
    return GCNPT_OK;
}

extern "C" int gcnpt_head_loss_fwd(void* stream, const float* logits, const int64_t* labels, const float* pooled, long long ldp, int H, float l2,
                                   int M, int C, float* loss, float* probs, int64_t* pred, int32_t* status) {
    const int rc = loss_check("head_loss_fwd", logits, pooled, ldp, H, l2, M, C);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(loss || probs || pred || status, "head_loss_fwd: null outputs (nothing to compute)");
    GCNPT_REQUIRE(!loss || labels, "head_loss_fwd: the loss needs labels");
    hipLaunchKernelGGL(head_loss_fwd_kernel, dim3(1), dim3(HL_THREADS), 0, (hipStream_t)stream, logits, labels, pooled, (size_t)ldp, H, l2, M,
                       C, loss, probs, pred, status);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_head_loss_bwd(void* stream, const float* dloss, const float* logits, const int64_t* labels, const float* pooled,
                                   long long ldp, int H, float l2, int M, int C, float* dlogits, float* dpooled) {
    const int rc = loss_check("head_loss_bwd", logits, pooled, ldp, H, l2, M, C);
    if (rc != GCNPT_OK) return rc;
    GCNPT_REQUIRE(dloss, "head_loss_bwd: null dloss");
    GCNPT_REQUIRE(dlogits || dpooled, "head_loss_bwd: null outputs (nothing to compute)");
    GCNPT_REQUIRE(!dlogits || labels, "head_loss_bwd: dlogits needs labels");
    GCNPT_REQUIRE(!dpooled || pooled, "head_loss_bwd: dpooled needs pooled");
    hipLaunchKernelGGL(head_loss_bwd_kernel, dim3(ceil_div(M, HLB_WAVES)), dim3(HLB_THREADS), 0, (hipStream_t)stream, dloss, logits, labels,
                       pooled, (size_t)ldp, H, l2, M, C, dlogits, dpooled);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}
