// The relation-conditioned traversal of adj_type == 'full_deprel' (SURVEY.md 8f row N3): reference model/gcn.py:400-415
//   y[m,:] = sum_d e[m,d] * (x[m,:] @ W3[d])           W3 = Linear.weight.reshape(D, Tin, H)   (gcn.py:301)
// for the M tokens that sit in a pruned tree (compacted by the caller).  The reference materialises the outer product
// e (x) x as [B,T,D,Tin] and contracts it with two einsums.  Here the per-relation products P_d = x @ W3[d] run on the
// matrix cores and are folded into the result with one fp32 FMA per accumulator register:
//   * the MFMAs run with swapped operands (weights as A), so a lane holds ONE token row and 4 consecutive output columns:
//     the scale e[m,d] is a single scalar per lane and tile;
//   * a workgroup owns ROWS tokens x 48 output columns and one slice of the relations; each wave keeps the x fragments of its
//     16 MT tokens in registers for the whole kernel; the weight fragments of a relation come through LDS once per workgroup;
//     every relation slice writes its own plane of the result, the caller sums the planes (and adds e @ b3).
// Both precisions (bf16 operands with fp32 accumulation; exact fp32, the module's default and the mode the reference-recorded
// gradient goldens are checked in) share ONE core, parametrised by a precision trait (Bf16 / Fp32 below): the pack kernels, the
// parameters and the plan, the traversal kernels' block decode, x fragments, e tile, gy tile, de dot and plane stores, and the
// whole dW kernel but its MFMA step.  Two things stay per precision: how a relation's weight fragments reach the MFMAs (bf16: a
// 4-deep LDS ring filled by direct-to-LDS loads; fp32, MFMA-bound by a wide margin at 1/16 of the bf16 rate: a two-stage LDS
// buffer filled through registers) and the MFMA inner loops.
// Fragment = 16 bytes per lane = VPL values X[k = KSTEP kstep + VPL (lane >> 4) + j][n = 16 tile + (lane & 15)], j = 0..VPL-1 (the
// layer kernels' image orders, include/gcnpt.h).  Weights are packed once per step: image[n_tile][d * TS + ts][lane],
// TS = ceil(Tin / KSTEP), every relation padded to TS k-steps.
#include <type_traits>

#include "layer_common.h"

namespace gcnpt {

constexpr int BL_THREADS = 256, BL_WAVES = BL_THREADS / WAVE;
constexpr int BL_NT = 3;                     // 16-column output tiles per workgroup

// What the two precisions differ in.  TSMAX: k-steps per relation the registers are sized for (Tin <= 256); MT: 16-row token tiles
// per wave; ROWS: token rows per workgroup; ECAP: relations per slice whose e tile fits LDS beside the weight buffers (WLDS bytes);
// DW_MT: tile rows of a dW block (bf16: a scaled gy fragment feeds 8 MFMAs -- 4 x 3 x 4 was VALU-bound)
struct Bf16 {
    typedef bf16_t op_t;
    static constexpr int KSTEP = 32, VPL = 8, TSMAX = 8, MT = 4, ROWS = 16 * MT * BL_WAVES, ECAP = 48, DW_MT = 8;
    static constexpr int RING = 4;                                           // relations in the LDS ring
    static constexpr int GL = (BL_NT * TSMAX + BL_WAVES - 1) / BL_WAVES;     // direct-to-LDS loads per wave and relation: always 6
    static constexpr int FRAGS = GL * BL_WAVES;                              // fragment slots per ring entry (24 KiB), TS < 8 leaves some unused
    static constexpr size_t WLDS = ((size_t)RING * FRAGS + BL_WAVES) * 64 * sizeof(uint4);       // ring | one dummy fragment per wave
    static __device__ __forceinline__ uint4 make_fragment(const float (&v)[VPL]) { return pack_bf16x8(v); }
};
struct Fp32 {
    typedef float op_t;
    static constexpr int KSTEP = 16, VPL = 4, TSMAX = 16, MT = 2, ROWS = 16 * MT * BL_WAVES, ECAP = 64, DW_MT = 4;
    static constexpr int STAGE = BL_NT * TSMAX * 64;                         // uint4 per stage (all slots: the stores are unconditional)
    static constexpr size_t WLDS = (size_t)2 * STAGE * sizeof(uint4);
    static __device__ __forceinline__ uint4 make_fragment(const float (&v)[VPL]) {
        return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    }
};

// transposed = 0: contraction over Tin, output columns H (forward);  1: contraction over H, output columns Tin (the same kernel
// then computes dx = sum_d e_d (gy @ W3[d]^T))
template <class P>
__global__ void bilinear_pack_kernel(const float* __restrict__ W, int D, int Tin, int H, int TS, long long n_frag_lanes,
                                     uint4* __restrict__ img, int transposed) {
    for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < n_frag_lanes; gid += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(gid & 63);
        const long long f = gid >> 6;
        const int ks = (int)(f % ((long long)D * TS)), tl = (int)(f / ((long long)D * TS));
        const int d = ks / TS, ts = ks - d * TS;
        const int n = tl * 16 + (lane & 15), k0 = ts * P::KSTEP + P::VPL * (lane >> 4);
        const int Kd = transposed ? H : Tin, Nd = transposed ? Tin : H;
        float v[P::VPL];
#pragma unroll
        for (int j = 0; j < P::VPL; ++j) {                  // unconditional clamped loads, dropped with a select
            const int kc = min(k0 + j, Kd - 1), nc = min(n, Nd - 1);
            const float x = transposed ? W[((size_t)d * Tin + nc) * H + kc] : W[((size_t)d * Tin + kc) * H + nc];
            v[j] = (k0 + j < Kd && n < Nd) ? x : 0.0f;
        }
        img[gid] = P::make_fragment(v);
    }
}

// rows -> "row-contraction" fragment image (lane = column, VPL consecutive TOKENS per lane, as the saved operands of the layer
// kernels): img[w_tile][m_step][lane] = VPL values src[KSTEP ms + VPL (lane >> 4) + j][16 wt + (lane & 15)]
template <class P>
__global__ void rows_pack_kernel(const float* __restrict__ src, int M, int W, int m_steps, long long n_lanes, uint4* __restrict__ img) {
    for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < n_lanes; gid += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(gid & 63);
        const long long f = gid >> 6;
        const int ms = (int)(f % m_steps), wt = (int)(f / m_steps);
        const int c = wt * 16 + (lane & 15), m0 = ms * P::KSTEP + P::VPL * (lane >> 4);
        float v[P::VPL];
#pragma unroll
        for (int j = 0; j < P::VPL; ++j) {
            const float x = src[(size_t)min(m0 + j, M - 1) * W + min(c, W - 1)];
            v[j] = (m0 + j < M && c < W) ? x : 0.0f;
        }
        img[gid] = P::make_fragment(v);
    }
}

struct BilinearParams {
    const void* x;          // [M, TSA * KSTEP] operands (bf16 or fp32), zero padded
    const float* e;         // MODE 0: [M, D]
    const uint4* img;       // packed W3
    float* y;               // MODE 0: [chunks][slices][M, H], one plane per relation slice; MODE 1: [chunks][nb][M, D], one per column block
    const float* gy;        // MODE 1: [M, H] upstream gradient
    int M, D, H, TS, n_tiles, mb, nb, slices, d_per_slice;
    int TSA, chunks;        // k-steps per relation in all (x rows and the image are that wide); the contraction is cut into `chunks` runs
                            // of <= TS k-steps (Tin > 256: what the registers hold), each with planes of its own
};

__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p;
}

// ---- what the two traversal kernels share (pointers and scalars in, everything inlined) ---------------------------------------
// blockIdx -> this workgroup's run of the contraction (chunk: k-steps ts0 .. ts0 + TS), relation slice (d_lo .. d_lo + nd), row block
// bm and block bn of BL_NT output tiles
struct BlBlock { int chunk, ts0, TS, slice, bm, bn, d_lo, nd; };
__device__ __forceinline__ BlBlock bl_decode(int bid, int mb, int nb, int slices, int d_per_slice, int D, int TSp, int TSA) {
    BlBlock b;
    const int per_chunk = mb * nb * slices;
    b.chunk = bid / per_chunk; b.ts0 = b.chunk * TSp;
    b.TS = min(TSp, TSA - b.ts0);
    const int id = bid - b.chunk * per_chunk;
    b.slice = id % slices;
    const int rest = id / slices;
    b.bm = rest % mb; b.bn = rest / mb;
    b.d_lo = b.slice * d_per_slice;
    b.nd = min(D, b.d_lo + d_per_slice) - b.d_lo;
    return b;
}

// a wave's x fragments: lane (l & 15) = token row, VPL consecutive k per lane -- registers for the whole kernel
template <class P>
__device__ __forceinline__ void load_x_fragments(const typename P::op_t* x, int M, int TSA, int m0, int ts0, int TS, int lane, uint4 (&xf)[P::MT][P::TSMAX]) {
#pragma unroll
    for (int mt = 0; mt < P::MT; ++mt) {
        const size_t row = (size_t)min(m0 + 16 * mt + (lane & 15), M - 1);
#pragma unroll
        for (int ts = 0; ts < P::TSMAX; ++ts)
            xf[mt][ts] = *reinterpret_cast<const uint4*>(x + row * (TSA * P::KSTEP) + (ts0 + min(ts, TS - 1)) * P::KSTEP + P::VPL * (lane >> 4));
    }
}

// e of the workgroup's rows -> LDS, relation-major: es[nd][ROWS + 1]
template <int ROWS>
__device__ __forceinline__ void stage_e_tile(const float* e, float* es, int M, int D, int rows0, int d_lo, int nd, int tid) {
    constexpr int EU = 8;                                    // loads in flight per thread and round (a load per round would be ~20 round trips)
    for (int q0 = tid; q0 < nd * ROWS; q0 += BL_THREADS * EU) {
        float v[EU];
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const int q = min(q0 + u * BL_THREADS, nd * ROWS - 1);
            const int row = q / nd, dl = q - row * nd;
            v[u] = e[(size_t)min(rows0 + row, M - 1) * D + d_lo + dl];
        }
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const int q = q0 + u * BL_THREADS;
            const int row = q / nd, dl = q - row * nd;
            if (q < nd * ROWS) es[dl * (ROWS + 1) + row] = v[u];
        }
    }
}

// MODE 1: the upstream gradient's values at the positions of a wave's result tiles
template <int MT>
__device__ __forceinline__ void load_gy_tile(const float* gy, int M, int H, int n_tiles, int m0, int nt0, int lane, f32x4_t (&acc)[MT][BL_NT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < BL_NT; ++j) {
            const size_t row = (size_t)min(m0 + 16 * mt + (lane & 15), M - 1);
            const int n = (nt0 + j) * 16 + 4 * (lane >> 4);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float v = gy[row * H + min(n + g, H - 1)];
                acc[mt][j][g] = (n + g < H && nt0 + j < n_tiles) ? v : 0.0f;
            }
        }
}

// MODE 1: de[m, d] = P_d[m, :] . gy[m, :] over this block's 48 columns, into the block's plane
template <int MT>
__device__ __forceinline__ void de_dot_store(const f32x4_t (&prod)[MT][BL_NT], const f32x4_t (&gyt)[MT][BL_NT], float* plane, int M, int D, int m0, int d, int lane) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        float sdot = 0.0f;
#pragma unroll
        for (int j = 0; j < BL_NT; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) sdot += prod[mt][j][g] * gyt[mt][j][g];
        sdot += __shfl_xor(sdot, 16);
        sdot += __shfl_xor(sdot, 32);
        const int m = m0 + 16 * mt + (lane & 15);
        if (lane < 16 && m < M) plane[(size_t)m * D + d] = sdot;
    }
}

// MODE 0: every wave owns its rows: plain 16-byte stores into this relation slice's own plane of y (the caller sums the planes: ten
// float atomics per element cost more than the whole contraction -- ~50 G atomics/s device-wide -- a plane costs one store)
template <int MT>
__device__ __forceinline__ void store_plane(const f32x4_t (&acc)[MT][BL_NT], float* plane, int M, int H, int n_tiles, int m0, int nt0, int lane) {
    const bool vec = (H & 3) == 0;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m0 + 16 * mt + (lane & 15);
#pragma unroll
        for (int j = 0; j < BL_NT; ++j) {
            const int n = (nt0 + j) * 16 + 4 * (lane >> 4);
            if (m < M && nt0 + j < n_tiles) {
                float* dst = plane + (size_t)m * H + n;
                if (vec && n + 4 <= H) {
                    *reinterpret_cast<float4*>(dst) = make_float4(acc[mt][j][0], acc[mt][j][1], acc[mt][j][2], acc[mt][j][3]);
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (n + g < H) dst[g] = acc[mt][j][g];
                }
            }
        }
    }
}

template <int MT>
__device__ __forceinline__ void zero_tiles(f32x4_t (&t)[MT][BL_NT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < BL_NT; ++j) t[mt][j] = (f32x4_t){0, 0, 0, 0};
}

// MODE 0: y planes = sum_d e_d P_d.   MODE 1: de[m,d] = P_d[m,:] . gy[m,:] (the gradient of the relation vectors: the same per-relation
// products, dotted with the upstream gradient instead of scaled and summed), one plane per block of 48 columns.
// bf16: a workgroup owns 256 tokens (its 4 waves take 64 each).  All waves walk the SAME relations: the 3 x TS weight fragments of a
// relation come from L2 ONCE per workgroup, straight into LDS (global_load_lds, one 1-KiB fragment per wave-instruction, lane-linear on
// both sides), and feed 16 MFMAs each.  The LDS ring holds 4 relations; three are in flight while one is multiplied: the wait at the top
// of a round is a COUNTED s_waitcnt (two relations' loads of this wave may stay outstanding) and the barrier a raw s_barrier --
// __syncthreads() would drain the direct-to-LDS loads (they count as pending LDS writes) and with it the pipeline.
template <int MODE>
__global__ __launch_bounds__(BL_THREADS, 1) void bilinear_fwd_kernel(const BilinearParams p) {
    constexpr int MT = Bf16::MT, ROWS = Bf16::ROWS, TSMAX = Bf16::TSMAX, RING = Bf16::RING, GL = Bf16::GL, FRAGS = Bf16::FRAGS;
    extern __shared__ __attribute__((aligned(16))) unsigned char bl_smem[];              // ONE LDS object: ring | dummy | e tile
    const BlBlock b = bl_decode((int)blockIdx.x, p.mb, p.nb, p.slices, p.d_per_slice, p.D, p.TS, p.TSA);
    const int TS = b.TS, ts0 = b.ts0, d_lo = b.d_lo, nd = b.nd;
    const int n_frag = BL_NT * TS;
    uint4* wl = reinterpret_cast<uint4*>(bl_smem);                                       // [RING][FRAGS][64]
    uint4* dummy = wl + (size_t)RING * FRAGS * 64;                                       // [BL_WAVES][64]: where unused slots' loads land
    float* es = reinterpret_cast<float*>(dummy + BL_WAVES * 64);                         // [d_per_slice][ROWS + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = b.bm * ROWS + wave * 16 * MT, nt0 = b.bn * BL_NT;
    const size_t d_stride = (size_t)p.D * p.TSA;         // fragments per output tile in the image

    uint4 xf[MT][TSMAX];
    load_x_fragments<Bf16>(static_cast<const bf16_t*>(p.x), p.M, p.TSA, m0, ts0, TS, lane, xf);
    // relation dd -> ring entry: exactly GL loads per wave (fragments wave, wave + 4, ...; slots past 3 TS go to the dummy)
    auto fetch_w = [&](int dd) {
        const int d = d_lo + min(dd, nd - 1);
        uint4* ring = wl + (size_t)(dd & (RING - 1)) * FRAGS * 64;
#pragma unroll
        for (int u = 0; u < GL; ++u) {
            const int f = wave + u * BL_WAVES;
            const int fc = min(f, n_frag - 1);
            const int j = fc / TS, ts = fc - j * TS;
            const uint4* src = p.img + ((size_t)min(nt0 + j, p.n_tiles - 1) * d_stride + (size_t)d * p.TSA + ts0 + ts) * 64 + lane;
            uint4* dst = f < n_frag ? ring + (size_t)f * 64 : dummy + wave * 64;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        }
    };
    fetch_w(0);
    fetch_w(1);
    fetch_w(2);
    if constexpr (MODE == 0) stage_e_tile<ROWS>(p.e, es, p.M, p.D, b.bm * ROWS, d_lo, nd, tid);
    __syncthreads();                                         // (one full drain before the loop: e tile and the first three relations)

    f32x4_t acc[MT][BL_NT];                // MODE 0: the result tile; MODE 1: the upstream gradient's values at the tile's positions
    zero_tiles(acc);
    if constexpr (MODE == 1) {
        load_gy_tile(p.gy, p.M, p.H, p.n_tiles, m0, nt0, lane, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // those loads are not part of the loop's counted queue
    }

    for (int dd = 0; dd < nd; ++dd) {
        // relation dd has landed when at most the loads of dd+1 and dd+2 (2 x GL = 12 of this wave) are outstanding
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        __builtin_amdgcn_s_barrier();                        // ... in every wave; and every wave is done reading relation dd-1
        fetch_w(dd + 3);                                     // into the ring entry relation dd-1 has just left
        // Every LDS read of the loop is inline asm: hipcc cannot tell a ds_read from the ring apart from the direct-to-LDS loads in
        // flight and would put an s_waitcnt vmcnt(0) in front of each (seen in the ISA), which is the drain the counted wait avoids.
        const unsigned ring = lds_addr(wl) + (unsigned)((dd & (RING - 1)) * FRAGS * 1024) + (unsigned)lane * 16u;
        const unsigned eaddr = lds_addr(es) + (unsigned)((dd * (ROWS + 1) + wave * 16 * MT + (lane & 15)) * 4);
        float ev[MT] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (MODE == 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) asm volatile("ds_read_b32 %0, %1" : "=v"(ev[mt]) : "v"(eaddr + (unsigned)(mt * 64)));
        }
        uint4 wc[2][BL_NT];
        auto read_w = [&](int ts, uint4 (&w)[BL_NT]) {
#pragma unroll
            for (int j = 0; j < BL_NT; ++j) asm volatile("ds_read_b128 %0, %1" : "=v"(w[j]) : "v"(ring + (unsigned)((j * TS + ts) * 1024)));
        };
        read_w(0, wc[0]);
        f32x4_t prod[MT][BL_NT];
        zero_tiles(prod);
#pragma unroll
        for (int ts = 0; ts < TSMAX; ++ts) {
            if (ts < TS) {                                   // workgroup-uniform
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // this k-step's fragments (requested one k-step ago)
                if (ts + 1 < TS) read_w(ts + 1, wc[(ts + 1) & 1]);                  // the next one's, behind this k-step's MFMAs
#pragma unroll
                for (int j = 0; j < BL_NT; ++j)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        prod[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wc[ts & 1][j]),
                                                                              __builtin_bit_cast(bf16x8_t, xf[mt][ts]), prod[mt][j], 0, 0, 0);
            }
        }
        if constexpr (MODE == 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int j = 0; j < BL_NT; ++j) acc[mt][j] += ev[mt] * prod[mt][j];
        } else {
            de_dot_store(prod, acc, p.y + (size_t)(b.chunk * p.nb + b.bn) * p.M * p.D, p.M, p.D, m0, d_lo + dd, lane);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the clamped re-fetches past the slice's end
    if constexpr (MODE == 0) store_plane(acc, p.y + (size_t)(b.chunk * p.slices + b.slice) * p.M * p.H, p.M, p.H, p.n_tiles, m0, nt0, lane);
}

// fp32 (v_mfma_f32_16x16x4_f32; MFMA s of a k-step multiplies the s-th values of the fragments): 32 cycles per 16x16x4 MFMA, so the
// kernel needs none of the ring's machinery: a relation's weight fragments are prefetched through registers one relation ahead into a
// two-stage LDS buffer (a relation's MFMAs take ~10 k cycles per wave).  One workgroup per CU: ~250 registers.
template <int MODE>
__global__ __launch_bounds__(BL_THREADS, 1) void bilinear_f32_kernel(const BilinearParams p) {
    constexpr int MT = Fp32::MT, ROWS = Fp32::ROWS, TSMAX = Fp32::TSMAX, STAGE = Fp32::STAGE;
    extern __shared__ __attribute__((aligned(16))) unsigned char bf_smem[];              // [2][STAGE] uint4 | e tile
    const BlBlock b = bl_decode((int)blockIdx.x, p.mb, p.nb, p.slices, p.d_per_slice, p.D, p.TS, p.TSA);
    const int TS = b.TS, ts0 = b.ts0, d_lo = b.d_lo, nd = b.nd;
    const int n_frag = BL_NT * TS;
    uint4* wl = reinterpret_cast<uint4*>(bf_smem);
    float* es = reinterpret_cast<float*>(wl + (size_t)2 * STAGE);                        // [d_per_slice][ROWS + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = b.bm * ROWS + wave * 16 * MT, nt0 = b.bn * BL_NT;
    const size_t d_stride = (size_t)p.D * p.TSA;

    uint4 xf[MT][TSMAX];
    load_x_fragments<Fp32>(static_cast<const float*>(p.x), p.M, p.TSA, m0, ts0, TS, lane, xf);
    // a relation's fragments: thread t fetches fragment-lanes t, t + 256, ... (<= BL_NT * TSMAX * 64 / 256 = 12 per thread)
    constexpr int WPT = STAGE / BL_THREADS;
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));      // a first-class vector: hipcc kept an array of uint4 STRUCTS in scratch memory
    u32x4_t wr[WPT];
    auto fetch_w = [&](int dd) {
        const int d = d_lo + min(dd, nd - 1);
#pragma unroll
        for (int u = 0; u < WPT; ++u) {
            const int q = min(tid + u * BL_THREADS, n_frag * 64 - 1);
            const int f = q >> 6, l = q & 63;
            const int j = f / TS, ts = f - j * TS;
            wr[u] = *reinterpret_cast<const u32x4_t*>(p.img + ((size_t)min(nt0 + j, p.n_tiles - 1) * d_stride + (size_t)d * p.TSA + ts0 + ts) * 64 + l);
        }
    };
    // (unconditional stores into a stage sized for TSMAX k-steps: a prefetched register whose only use is a CONDITIONAL store gets
    // parked in scratch memory by hipcc right behind its load, i.e. the prefetch becomes a blocking load -- seen in the ISA)
    auto store_w = [&](int dd) {
        uint4* dst = wl + (size_t)(dd & 1) * STAGE;
#pragma unroll
        for (int u = 0; u < WPT; ++u) *reinterpret_cast<u32x4_t*>(dst + tid + u * BL_THREADS) = wr[u];
    };
    fetch_w(0);
    if constexpr (MODE == 0) stage_e_tile<ROWS>(p.e, es, p.M, p.D, b.bm * ROWS, d_lo, nd, tid);
    store_w(0);
    __syncthreads();

    f32x4_t acc[MT][BL_NT];                // MODE 0: the result tile; MODE 1: the upstream gradient's values at the tile's positions
    zero_tiles(acc);
    if constexpr (MODE == 1) load_gy_tile(p.gy, p.M, p.H, p.n_tiles, m0, nt0, lane, acc);

    for (int dd = 0; dd < nd; ++dd) {
        fetch_w(dd + 1);                                     // the next relation's fragments, in flight during this one's MFMAs
        const uint4* ring = wl + (size_t)(dd & 1) * STAGE;
        float ev[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) ev[mt] = MODE == 0 ? es[dd * (ROWS + 1) + wave * 16 * MT + 16 * mt + (lane & 15)] : 0.0f;
        f32x4_t prod[MT][BL_NT];
        zero_tiles(prod);
#pragma unroll
        for (int ts = 0; ts < TSMAX; ++ts) {
            if (ts < TS) {                                   // workgroup-uniform, no global load inside
                // the 4 MFMAs of a k-step that share an accumulator are kept BL_NT * MT instructions apart (a dependent MFMA right
                // behind its producer waits for the 8 passes to drain)
                f32x4_t wq[BL_NT];
#pragma unroll
                for (int j = 0; j < BL_NT; ++j) wq[j] = __builtin_bit_cast(f32x4_t, ring[(size_t)(j * TS + ts) * 64 + lane]);
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                    for (int j = 0; j < BL_NT; ++j)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            const f32x4_t xq = __builtin_bit_cast(f32x4_t, xf[mt][ts]);
                            prod[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[j][s4], xq[s4], prod[mt][j], 0, 0, 0);
                        }
            }
        }
        if constexpr (MODE == 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int j = 0; j < BL_NT; ++j) acc[mt][j] += ev[mt] * prod[mt][j];
        } else {
            de_dot_store(prod, acc, p.y + (size_t)(b.chunk * p.nb + b.bn) * p.M * p.D, p.M, p.D, m0, d_lo + dd, lane);
        }
        store_w(dd + 1);                                     // into the stage relation dd-1 left (everybody passed the barrier since)
        __syncthreads();
    }
    if constexpr (MODE == 0) store_plane(acc, p.y + (size_t)(b.chunk * p.slices + b.slice) * p.M * p.H, p.M, p.H, p.n_tiles, m0, nt0, lane);
}

// ---------------------------------------------------------------------------------------------------------------------------
// dW3[d][t][h] = sum_m e[m,d] * x[m,t] * gy[m,h]      (the weight gradient of the traversal: the outer product e (x) x contracted
// with the upstream gradient over the M tokens; the reference's autograd materialises [M, D*Tin] for it)
// Both token-side operands come as row-contraction fragment images (rows_pack_kernel): xI[t_tile][m_step][lane], gI[h_tile][m_step][lane].
// A workgroup owns a (DW_MT x 3)-tile block of dW3 for DW_ND relations; per m-step it loads the DW_MT + 3 fragments once and, for each of
// its relations, scales the three gy fragments by e[m, d] along the tokens and issues the MFMAs (`consume`, the per-precision part).  Its 4 waves
// take every 4th m-step and meet in LDS, DW_RH tile rows of one relation at a time (12 tiles x 4 waves = 48 KiB: half of a bf16
// relation's tiles, all of an fp32 one's); every element of dW3 is written once (no atomics).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int DW_NT = 3, DW_ND = 2, DW_RH = 4;

struct BilinearDwParams {
    const uint4* xI;        // [t_tiles][m_steps][64]
    const uint4* gI;        // [h_tiles][m_steps][64]
    const float* eT;        // [D][m_steps * KSTEP]: e transposed, zero padded along the tokens
    float* dW;              // [D][Tin][H] == the Linear weight's [D*H, Tin] memory
    int D, Tin, H, t_tiles, h_tiles, m_steps, tb, hb, dgroups;
};

template <class P>
struct DwOperands { uint4 xa[P::DW_MT], gb[DW_NT]; float4 ea[DW_ND][P::VPL / 4]; };

template <class P>
__global__ __launch_bounds__(BL_THREADS, 1) void bilinear_dw_kernel(const BilinearDwParams p) {
    constexpr int MT = P::DW_MT;
    static_assert(MT % DW_RH == 0, "the reduction walks the tile rows in whole rounds of DW_RH");
    __shared__ f32x4_t red[BL_WAVES][DW_RH * DW_NT][WAVE];                  // 48 KiB
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    const int bt = id % p.tb, rest = id / p.tb;
    const int bh = rest % p.hb, dg = rest / p.hb;
    const int t0 = bt * MT, h0 = bh * DW_NT, d0 = dg * DW_ND;
    f32x4_t acc[DW_ND][MT][DW_NT];
#pragma unroll
    for (int q = 0; q < DW_ND; ++q) zero_tiles(acc[q]);
    const size_t Mpad = (size_t)p.m_steps * P::KSTEP;
    auto fetch = [&](int ms_raw, DwOperands<P>& o) {         // clamped: the step past the end re-reads the last one and is not used
        const int ms = min(ms_raw, p.m_steps - 1);
#pragma unroll
        for (int i = 0; i < MT; ++i) o.xa[i] = p.xI[((size_t)min(t0 + i, p.t_tiles - 1) * p.m_steps + ms) * 64 + lane];
#pragma unroll
        for (int j = 0; j < DW_NT; ++j) o.gb[j] = p.gI[((size_t)min(h0 + j, p.h_tiles - 1) * p.m_steps + ms) * 64 + lane];
#pragma unroll
        for (int q = 0; q < DW_ND; ++q) {
            const float* ep = p.eT + (size_t)min(d0 + q, p.D - 1) * Mpad + (size_t)ms * P::KSTEP + P::VPL * (lane >> 4);
#pragma unroll
            for (int c = 0; c < P::VPL / 4; ++c) o.ea[q][c] = *reinterpret_cast<const float4*>(ep + 4 * c);
        }
    };
    // the per-precision part.  Swapped operands: rows = h (scaled gy), columns = t (x): a lane ends with 4 consecutive h of one t
    auto consume = [&](const DwOperands<P>& o) {
#pragma unroll
        for (int q = 0; q < DW_ND; ++q) {
            if constexpr (std::is_same<P, Bf16>::value) {
#pragma unroll
                for (int j = 0; j < DW_NT; ++j) {
                    // gy fragment scaled along the tokens by e[., d]: 8 bf16 -> fp32, multiply, back to bf16
                    const uint4 g = o.gb[j];
                    uint4 sg;
                    sg.x = (unsigned)f32_to_bf16(__uint_as_float(g.x << 16) * o.ea[q][0].x) | ((unsigned)f32_to_bf16(__uint_as_float(g.x & 0xffff0000u) * o.ea[q][0].y) << 16);
                    sg.y = (unsigned)f32_to_bf16(__uint_as_float(g.y << 16) * o.ea[q][0].z) | ((unsigned)f32_to_bf16(__uint_as_float(g.y & 0xffff0000u) * o.ea[q][0].w) << 16);
                    sg.z = (unsigned)f32_to_bf16(__uint_as_float(g.z << 16) * o.ea[q][1].x) | ((unsigned)f32_to_bf16(__uint_as_float(g.z & 0xffff0000u) * o.ea[q][1].y) << 16);
                    sg.w = (unsigned)f32_to_bf16(__uint_as_float(g.w << 16) * o.ea[q][1].z) | ((unsigned)f32_to_bf16(__uint_as_float(g.w & 0xffff0000u) * o.ea[q][1].w) << 16);
#pragma unroll
                    for (int i = 0; i < MT; ++i)
                        acc[q][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, sg), __builtin_bit_cast(bf16x8_t, o.xa[i]),
                                                                              acc[q][i][j], 0, 0, 0);
                }
            } else {
                // exact fp32: one multiply per value; MFMAs that share an accumulator are 12 instructions apart
                const float ev[4] = {o.ea[q][0].x, o.ea[q][0].y, o.ea[q][0].z, o.ea[q][0].w};
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                    for (int j = 0; j < DW_NT; ++j) {
                        const float sg = __builtin_bit_cast(f32x4_t, o.gb[j])[s4] * ev[s4];
#pragma unroll
                        for (int i = 0; i < MT; ++i)
                            acc[q][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(sg, __builtin_bit_cast(f32x4_t, o.xa[i])[s4], acc[q][i][j], 0, 0, 0);
                    }
            }
        }
    };
    // two m-steps per round: the operands of the next one are in flight while the current one is multiplied
    DwOperands<P> oa, ob;
    fetch(wave, oa);
    for (int ms = wave; ms < p.m_steps; ms += 2 * BL_WAVES) {
        fetch(ms + BL_WAVES, ob);
        consume(oa);
        fetch(ms + 2 * BL_WAVES, oa);
        if (ms + BL_WAVES < p.m_steps) consume(ob);          // wave-uniform, no load inside
    }
    // waves meet in LDS, DW_RH tile rows of one relation at a time
    for (int q = 0; q < DW_ND; ++q) {
        for (int ih = 0; ih < MT; ih += DW_RH) {
            __syncthreads();
#pragma unroll
            for (int q2 = 0; q2 < DW_ND; ++q2)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < DW_NT; ++j)
                        if (q2 == q && i >= ih && i < ih + DW_RH) red[wave][(i - ih) * DW_NT + j][lane] = acc[q2][i][j];      // static register indices
            __syncthreads();
            const int d = d0 + q;
            for (int tt = wave; tt < DW_RH * DW_NT; tt += BL_WAVES) {
                const int i = ih + tt / DW_NT, j = tt % DW_NT;
                f32x4_t v = red[0][tt][lane];
#pragma unroll
                for (int w = 1; w < BL_WAVES; ++w) v += red[w][tt][lane];
                const int t = (t0 + i) * 16 + (lane & 15);
                const int h = (h0 + j) * 16 + 4 * (lane >> 4);
                if (d < p.D && t < p.Tin && t0 + i < p.t_tiles && h0 + j < p.h_tiles) {
                    float* dst = p.dW + ((size_t)d * p.Tin + t) * p.H + h;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (h + g < p.H) dst[g] = v[g];
                }
            }
        }
    }
}

}  // namespace gcnpt

using namespace gcnpt;

// k-step width of the traversal's fragments: 32 values per lane group of bf16, 16 of fp32
static int bl_kstep(int dtype) { return dtype == GCNPT_BF16 ? Bf16::KSTEP : Fp32::KSTEP; }

// One workgroup per (row block, block of 48 output columns, relation slice, run of k-steps).  Tin beyond what a wave's registers hold
// (256) is cut into `chunks` runs of <= TS k-steps, each run with planes of its own.
template <class P>
static BilinearParams bilinear_plan(int M, int D, int Tin, int H) {
    BilinearParams p{};
    p.M = M; p.D = D; p.H = H; p.TSA = ceil_div(Tin, P::KSTEP); p.n_tiles = ceil_div(H, 16);
    p.chunks = ceil_div(p.TSA, P::TSMAX); p.TS = ceil_div(p.TSA, p.chunks);
    p.mb = ceil_div(M, P::ROWS); p.nb = ceil_div(p.n_tiles, BL_NT);
    // relation slices: about one workgroup per CU (each holds most of the LDS and all registers), at least 4 relations each
    int slices = std::max(1, std::min(256 / std::max(1, p.mb * p.nb * p.chunks), D / 4));
    slices = std::max(slices, ceil_div(D, P::ECAP));            // the e tile of a slice must fit LDS beside the weight buffers
    p.d_per_slice = ceil_div(D, slices);
    p.slices = ceil_div(D, p.d_per_slice);
    return p;
}
static BilinearParams bilinear_plan(int M, int D, int Tin, int H, int dtype) {
    return dtype == GCNPT_BF16 ? bilinear_plan<Bf16>(M, D, Tin, H) : bilinear_plan<Fp32>(M, D, Tin, H);
}

template <class P, int MODE>
static int bilinear_launch(hipStream_t s, const BilinearParams& p) {
    const size_t lds = P::WLDS + sizeof(float) * (P::ROWS + 1) * (size_t)p.d_per_slice;
    if (lds > 160 * 1024) return fail(GCNPT_E_UNSUPPORTED, "bilinear%s: %zu B of LDS", std::is_same<P, Bf16>::value ? "" : " (fp32)", lds);
    void (*kern)(const BilinearParams);
    if constexpr (std::is_same<P, Bf16>::value) kern = bilinear_fwd_kernel<MODE>;
    else kern = bilinear_f32_kernel<MODE>;
    GCNPT_LDS_ATTR_ONCE(kern, 160 * 1024);
    hipLaunchKernelGGL(kern, dim3(p.mb * p.nb * p.slices * p.chunks), dim3(BL_THREADS), lds, s, p);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

// gcnpt_bilinear_fwd (MODE 0: side = e, planes = y) and gcnpt_bilinear_bwd_e (MODE 1: side = gy, planes = de; stored by scalars)
template <int MODE>
static int bilinear_run(const char* who, void* stream, const void* x, const float* side, const void* w_img, int M, int D, int Tin, int H,
                        float* planes, int dtype) {
    GCNPT_REQUIRE(x && side && w_img && planes, "%s: null pointer", who);
    GCNPT_REQUIRE(M > 0 && D > 0 && Tin > 0 && H > 0, "%s: sizes must be positive", who);
    GCNPT_REQUIRE(aligned16(x) && aligned16(w_img) && (MODE == 1 || aligned16(planes)), "%s: %s must be 16-byte aligned", who,
                  MODE == 0 ? "x, w_img and y_planes" : "x and w_img");
    if (!gcnpt_bilinear_supported(D, Tin, H, dtype))
        return fail(GCNPT_E_UNSUPPORTED, "%s: Tin=%d is beyond what the traversal kernels are planned for", who, Tin);
    BilinearParams p = bilinear_plan(M, D, Tin, H, dtype);
    p.x = x; p.img = static_cast<const uint4*>(w_img); p.y = planes;
    (MODE == 0 ? p.e : p.gy) = side;
    return dtype == GCNPT_BF16 ? bilinear_launch<Bf16, MODE>((hipStream_t)stream, p) : bilinear_launch<Fp32, MODE>((hipStream_t)stream, p);
}

extern "C" size_t gcnpt_bilinear_packed_bytes(int D, int Tin, int H, int dtype) {
    if (D <= 0 || Tin <= 0 || H <= 0 || !dtype_ok(dtype)) return 0;
    return (size_t)ceil_div(H, 16) * D * ceil_div(Tin, bl_kstep(dtype)) * 64 * 16;
}

// (the bound only keeps the plane count sane: see bilinear_plan)
extern "C" int gcnpt_bilinear_supported(int D, int Tin, int H, int dtype) {
    if (!dtype_ok(dtype)) return 0;
    return D > 0 && H > 0 && Tin > 0 && ceil_div(Tin, bl_kstep(dtype)) <= 8 * (dtype == GCNPT_BF16 ? Bf16::TSMAX : Fp32::TSMAX);
}

extern "C" int gcnpt_bilinear_pack(void* stream, const float* W, int D, int Tin, int H, void* w_img, int transposed, int dtype) {
    GCNPT_REQUIRE(W && w_img, "bilinear_pack: null pointer");
    GCNPT_REQUIRE(D > 0 && Tin > 0 && H > 0 && dtype_ok(dtype), "bilinear_pack: sizes must be positive, dtype f32 or bf16");
    const int TS = ceil_div(transposed ? H : Tin, bl_kstep(dtype));
    const long long n = (long long)ceil_div(transposed ? Tin : H, 16) * D * TS * 64;
    const int grid = (int)std::min<long long>((n + 255) / 256, 1 << 16);
    auto kern = dtype == GCNPT_BF16 ? bilinear_pack_kernel<Bf16> : bilinear_pack_kernel<Fp32>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, W, D, Tin, H, TS, n, static_cast<uint4*>(w_img), transposed);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_bilinear_planes(int M, int D, int Tin, int H, int dtype) {
    if (M <= 0 || !gcnpt_bilinear_supported(D, Tin, H, dtype)) return 0;
    const BilinearParams p = bilinear_plan(M, D, Tin, H, dtype);
    return p.slices * p.chunks;
}

extern "C" int gcnpt_bilinear_de_planes(int M, int D, int Tin, int H, int dtype) {
    if (M <= 0 || !gcnpt_bilinear_supported(D, Tin, H, dtype)) return 0;
    const BilinearParams p = bilinear_plan(M, D, Tin, H, dtype);
    return p.nb * p.chunks;
}

extern "C" int gcnpt_bilinear_fwd(void* stream, const void* x, const float* e, const void* w_img, int M, int D, int Tin, int H,
                                  float* y_planes, int dtype) {
    return bilinear_run<0>("bilinear_fwd", stream, x, e, w_img, M, D, Tin, H, y_planes, dtype);
}

extern "C" int gcnpt_bilinear_bwd_e(void* stream, const void* x, const float* gy, const void* w_img, int M, int D, int Tin, int H,
                                    float* de_planes, int dtype) {
    return bilinear_run<1>("bilinear_bwd_e", stream, x, gy, w_img, M, D, Tin, H, de_planes, dtype);
}

extern "C" size_t gcnpt_rows_image_bytes(int M, int W, int dtype) {
    if (M <= 0 || W <= 0 || !dtype_ok(dtype)) return 0;
    return (size_t)ceil_div(W, 16) * ceil_div(M, bl_kstep(dtype)) * 64 * 16;
}

extern "C" int gcnpt_rows_pack(void* stream, const float* src, int M, int W, void* img, int dtype) {
    GCNPT_REQUIRE(src && img, "rows_pack: null pointer");
    GCNPT_REQUIRE(M > 0 && W > 0 && dtype_ok(dtype), "rows_pack: sizes must be positive, dtype f32 or bf16");
    const int m_steps = ceil_div(M, bl_kstep(dtype));
    const long long n = (long long)ceil_div(W, 16) * m_steps * 64;
    const int grid = (int)std::min<long long>((n + 255) / 256, 1 << 16);
    auto kern = dtype == GCNPT_BF16 ? rows_pack_kernel<Bf16> : rows_pack_kernel<Fp32>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, M, W, m_steps, n, static_cast<uint4*>(img));
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_bilinear_bwd_w(void* stream, const void* x_img, const void* gy_img, const float* eT, int M, int D, int Tin, int H,
                                    float* dW, int dtype) {
    GCNPT_REQUIRE(x_img && gy_img && eT && dW, "bilinear_bwd_w: null pointer");
    GCNPT_REQUIRE(M > 0 && D > 0 && Tin > 0 && H > 0 && dtype_ok(dtype), "bilinear_bwd_w: sizes must be positive, dtype f32 or bf16");
    GCNPT_REQUIRE(aligned16(x_img) && aligned16(gy_img) && aligned16(eT), "bilinear_bwd_w: images and eT must be 16-byte aligned");
    BilinearDwParams p{};
    p.xI = static_cast<const uint4*>(x_img); p.gI = static_cast<const uint4*>(gy_img); p.eT = eT; p.dW = dW;
    p.D = D; p.Tin = Tin; p.H = H; p.t_tiles = ceil_div(Tin, 16); p.h_tiles = ceil_div(H, 16); p.m_steps = ceil_div(M, bl_kstep(dtype));
    p.tb = ceil_div(p.t_tiles, dtype == GCNPT_BF16 ? Bf16::DW_MT : Fp32::DW_MT); p.hb = ceil_div(p.h_tiles, DW_NT); p.dgroups = ceil_div(D, DW_ND);
    const long long blocks = (long long)p.tb * p.hb * p.dgroups;
    if (blocks > 0x7fffffffLL) return fail(GCNPT_E_UNSUPPORTED, "bilinear_bwd_w: too many blocks");
    auto kern = dtype == GCNPT_BF16 ? bilinear_dw_kernel<Bf16> : bilinear_dw_kernel<Fp32>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(BL_THREADS), 0, (hipStream_t)stream, p);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}
