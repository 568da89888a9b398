// The constants the two wide forms of the layer kernel share (wide_kernels.hip: forward; wide_bwd_kernels.hip: backward-data).  Two
// translation units, so that neither form's instantiations change the code the compiler emits for the other's.
#pragma once
#include "rowtile_body.h"

namespace gcnpt {

constexpr int WIDE_THREADS = 256;                       // 4 waves
constexpr int WIDE_WAVES = WIDE_THREADS / WAVE;
constexpr int WIDE_KCHUNK = 256;                        // columns of S per chunk, a multiple of both k-steps: 33 KB of fp32 tile in LDS
constexpr int WIDE_NTW = 2;                             // transform / backward: output column tiles per wave
constexpr int WIDE_COLS = WIDE_WAVES * WIDE_NTW * 16;   // transform / backward: output columns per workgroup
constexpr int WIDE_KB = 8;                              // transform / backward: k-steps of weight fragments per register block (two in flight)

// S chunk row stride in CT elements (the row tile's bank-spreading rule)
__host__ __device__ inline int wide_s_stride(int ct_size) { return lds_stride_dw(WIDE_KCHUNK * ct_size / 4) * 4 / ct_size; }

}  // namespace gcnpt
