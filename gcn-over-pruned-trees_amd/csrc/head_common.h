// One wave's view of one row of logits: the softmax statistics and the argmax that the output head (head_kernels.hip) and the evaluation
// launch (eval_kernels.hip) both derive, so that the two give the same bits for the same row.
#pragma once
#include "gcnpt_common.h"

namespace gcnpt {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {                 // butterfly: a fixed order, the same total in every lane
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// max and sum_c exp(z_c - max) of one row, by one wave
__device__ __forceinline__ void row_softmax_stats(const float* __restrict__ z, int C, int lane, float& mx, float& den) {
    float m = -INFINITY;
    for (int c = lane; c < C; c += WAVE) m = fmaxf(m, z[c]);
    mx = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += WAVE) s += expf(z[c] - mx);
    den = wave_sum(s);
}

// the lowest index that holds the row's maximum mx, in every lane (an all-NaN row has no maximum: 0, as np.argmax gives)
__device__ __forceinline__ int row_argmax(const float* __restrict__ z, int C, int lane, float mx) {
    int best = 0x7fffffff;
    for (int c = lane; c < C; c += WAVE)
        if (z[c] == mx) best = min(best, c);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, WAVE));
    return best < C ? best : 0;
}

}  // namespace gcnpt
