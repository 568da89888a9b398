// The last three lines of a single-process training step as the reference runs it (train.py:225-227: clip_grad_norm_(parameters,
// max_grad_norm); optimizer.step(); optimizer.zero_grad()) for torch.optim.SGD and MyAdagrad (utils/torch_utils.py:10-90), on the parameters
// where they live: a list of dense tensors plus a list of ROW-SPARSE tables whose gradient is the uncoalesced (token ids, rows) pair the
// embedding backward leaves.  No sort, no host sync, no [V,E] pass: four launches for a model that fits one argument block.
//   1. sumsq + elect   dense workgroups write the sum of squares of their 1024-element chunks to their own partial slot (plain stores,
//                      nothing to zero); table workgroups elect ONE owner token per id: atomicMin(owner[id], token position) on the
//                      all-ones (-1) workspace, unsigned
//   2. merge           scratch[t] = owner[ids[t]] (-1 for an id outside the table); every other token's row is added into its owner's
//                      row of `rows`: float atomics, one wave per token row and 64 consecutive columns (256 contiguous bytes) per
//                      wave-instruction, zero elements (rows >= topn, the padding row) skipped -- or, GCNPT_OPT_DETERMINISTIC, the owner's
//                      wave adds the other rows itself in ascending token position
//   3. table sumsq     owner rows only (scratch[t] == t), one slot per workgroup
//   4. update          every workgroup adds ALL slots in the same fixed order (so all agree on coef bit for bit), then updates its
//                      chunks / owner rows, stores zeros over the dense g it consumed and resets owner[id] = -1 for every token's id
// Sums of squares in double.  The descriptors travel as kernel arguments (no device-side descriptor table, nothing copied from the host):
// 64 tensors and 8 tables per launch; a model with more takes more launches per phase.
#include "gcnpt_common.h"

#include <math.h>

namespace gcnpt {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = 1024;              // dense elements per work item: one float4 per thread
constexpr int OPT_TOK = 16;                  // tokens per table work item: 4 per wave
constexpr int OPT_DENSE_BLOCKS = 512;        // most workgroups (= partial slots) of one launch's dense share
constexpr int OPT_TABLE_SLOTS = 128;         // most workgroups (= partial slots) of one table-sumsq launch
constexpr int OPT_TABLE_BLOCKS = 4096;       // most table workgroups of the other launches (they loop over the items)
constexpr int ND = GCNPT_OPTIM_TENSORS_PER_LAUNCH, NT = GCNPT_OPTIM_TABLES_PER_LAUNCH;

// first[i] = first work item of descriptor i, first[n] = their number
struct DenseArgs { gcnpt_optim_tensor_t t[ND]; int first[ND + 1]; int n; };
struct TableArgs { gcnpt_optim_table_t t[NT]; int first[NT + 1]; int n; };

template <int N>
__device__ __forceinline__ int find_item(const int (&first)[N], int n, int item) {       // (wave-uniform: scalar loads of the argument block)
    int k = 0;
    while (k + 1 < n && first[k + 1] <= item) ++k;
    return k;
}

__device__ __forceinline__ bool aligned16(const gcnpt_optim_tensor_t& t) {
    return ((((uintptr_t)t.w) | ((uintptr_t)t.g) | ((uintptr_t)t.state)) & 15) == 0;
}

// sum over the workgroup, valid in thread 0
__device__ __forceinline__ double block_sum(double s) {
    __shared__ double red[OPT_THREADS / WAVE];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < OPT_THREADS / WAVE; ++w) t += red[w];
    return t;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sumsq_elect_kernel(const DenseArgs d, const TableArgs tb, int dense_blocks,
                                                                        float* __restrict__ slots) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < dense_blocks) {
        double s = 0.0;
        const int total = d.first[d.n];
        for (int item = blockIdx.x; item < total; item += dense_blocks) {
            const int k = find_item(d.first, d.n, item);
            const float* __restrict__ g = d.t[k].g;
            const long long n = d.t[k].n, base = (long long)(item - d.first[k]) * OPT_CHUNK;
            if (aligned16(d.t[k])) {
                const long long i = base + 4 * tid;
                if (i + 3 < n) {
                    const float4 v = *reinterpret_cast<const float4*>(g + i);
                    s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
                } else {
                    for (long long j = i; j < n && j < i + 4; ++j) s += (double)g[j] * g[j];
                }
            } else {
                const long long end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
                for (long long i = base + tid; i < end; i += OPT_THREADS) s += (double)g[i] * g[i];
            }
        }
        s = block_sum(s);
        if (tid == 0) slots[blockIdx.x] = (float)s;
        return;
    }
    const int total = tb.first[tb.n], nb = gridDim.x - dense_blocks;
    for (int item = blockIdx.x - dense_blocks; item < total; item += nb) {
        const int k = find_item(tb.first, tb.n, item);
        const int t = (item - tb.first[k]) * OPT_TOK + tid;
        if (tid < OPT_TOK && t < tb.t[k].n_rows) {
            const long long id = tb.t[k].ids[t];
            if (id >= 0 && id < tb.t[k].V) atomicMin(reinterpret_cast<unsigned*>(tb.t[k].owner) + id, (unsigned)t);
        }
    }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_merge_kernel(const TableArgs tb, int deterministic) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = tb.first[tb.n];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = find_item(tb.first, tb.n, item);
        const int n_rows = tb.t[k].n_rows, E = tb.t[k].E, V = tb.t[k].V;
        const int64_t* __restrict__ ids = tb.t[k].ids;
        float* rows = tb.t[k].rows;
        for (int j = 0; j < OPT_TOK / 4; ++j) {
            const int t = (item - tb.first[k]) * OPT_TOK + wave * (OPT_TOK / 4) + j;
            if (t >= n_rows) break;
            const long long id = ids[t];
            int o = (id >= 0 && id < V) ? tb.t[k].owner[id] : -1;
            if (o >= n_rows) o = -1;             // (a workspace that was not all -1 on entry: such a token is dropped, nothing is addressed through it)
            if (lane == 0) tb.t[k].scratch[t] = o;
            if (o < 0) continue;
            if (!deterministic) {
                if (o == t) continue;
                const float* src = rows + (size_t)t * E;
                float* dst = rows + (size_t)o * E;
                for (int e = lane; e < E; e += WAVE) {              // 64 consecutive columns per wave-instruction: 256 contiguous bytes per atomic
                    const float x = src[e];
                    if (x != 0.0f) atomicAdd(dst + e, x);
                }
            } else if (o == t) {                                    // the owner is the id's first token: the others lie behind it
                float* dst = rows + (size_t)t * E;
                for (int base = t + 1; base < n_rows; base += WAVE) {
                    const int tt = base + lane;
                    unsigned long long m = __ballot(tt < n_rows && ids[tt] == id);
                    while (m) {
                        const int b = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float* src = rows + (size_t)(base + b) * E;
                        for (int e = lane; e < E; e += WAVE) dst[e] += src[e];
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_table_sumsq_kernel(const TableArgs tb, float* __restrict__ slots) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = tb.first[tb.n];
    double s = 0.0;
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = find_item(tb.first, tb.n, item);
        const int n_rows = tb.t[k].n_rows, E = tb.t[k].E;
        for (int j = 0; j < OPT_TOK / 4; ++j) {
            const int t = (item - tb.first[k]) * OPT_TOK + wave * (OPT_TOK / 4) + j;
            if (t >= n_rows) break;
            if (tb.t[k].scratch[t] != t) continue;
            const float* __restrict__ row = tb.t[k].rows + (size_t)t * E;
            for (int e = lane; e < E; e += WAVE) s += (double)row[e] * row[e];
        }
    }
    s = block_sum(s);
    if (threadIdx.x == 0) slots[blockIdx.x] = (float)s;
}

template <int KIND>
__device__ __forceinline__ void update_one(float& w, float& st, float g, float coef, float lr) {
    const float gh = coef * g;
    if (KIND == GCNPT_OPTIM_ADAGRAD) {
        st += gh * gh;
        w -= lr * gh / (sqrtf(st) + 1e-10f);
    } else {
        w -= lr * gh;
    }
}

template <int KIND>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const DenseArgs d, const TableArgs tb, int dense_blocks, float max_norm,
                                                                   float lr, const float* __restrict__ lr_dev, int clear_grads,
                                                                   float* __restrict__ partials, int n_slots, int write_result) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float s_coef;
    {   // the same sum in the same order in every workgroup of every update launch
        double s = 0.0;
        for (int i = tid; i < n_slots; i += OPT_THREADS) s += (double)partials[2 + i];
        s = block_sum(s);
        if (tid == 0) {
            const float norm = (float)sqrt(s);
            const float coef = max_norm > 0.0f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f;
            s_coef = coef;
            if (write_result && blockIdx.x == 0) { partials[GCNPT_OPTIM_NORM] = norm; partials[GCNPT_OPTIM_COEF] = coef; }
        }
        __syncthreads();
    }
    const float coef = s_coef;
    if (lr_dev) lr = *lr_dev;
    constexpr bool ADA = KIND == GCNPT_OPTIM_ADAGRAD;
    if ((int)blockIdx.x < dense_blocks) {
        const int total = d.first[d.n];
        for (int item = blockIdx.x; item < total; item += dense_blocks) {
            const int k = find_item(d.first, d.n, item);
            float* __restrict__ w = d.t[k].w;
            float* __restrict__ g = d.t[k].g;
            float* __restrict__ st = d.t[k].state;
            const long long n = d.t[k].n, base = (long long)(item - d.first[k]) * OPT_CHUNK;
            const long long i4 = base + 4 * tid;
            if (aligned16(d.t[k]) && i4 + 3 < n) {
                float4 p = *reinterpret_cast<float4*>(w + i4);
                const float4 v = *reinterpret_cast<const float4*>(g + i4);
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ADA) a = *reinterpret_cast<float4*>(st + i4);
                update_one<KIND>(p.x, a.x, v.x, coef, lr);
                update_one<KIND>(p.y, a.y, v.y, coef, lr);
                update_one<KIND>(p.z, a.z, v.z, coef, lr);
                update_one<KIND>(p.w, a.w, v.w, coef, lr);
                *reinterpret_cast<float4*>(w + i4) = p;
                if (ADA) *reinterpret_cast<float4*>(st + i4) = a;
                if (clear_grads) *reinterpret_cast<float4*>(g + i4) = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                // the scalar path: a tensor that is not 16-byte aligned (thread-strided), or the last elements of an aligned one
                const bool vec = aligned16(d.t[k]);
                const long long end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
                const long long lo = vec ? i4 : base + tid, hi = vec ? (i4 + 4 < end ? i4 + 4 : end) : end, step = vec ? 1 : OPT_THREADS;
                for (long long i = lo; i < hi; i += step) {
                    float p = w[i], a = ADA ? st[i] : 0.0f;
                    update_one<KIND>(p, a, g[i], coef, lr);
                    w[i] = p;
                    if (ADA) st[i] = a;
                    if (clear_grads) g[i] = 0.0f;
                }
            }
        }
        return;
    }
    const int total = tb.first[tb.n], nb = gridDim.x - dense_blocks;
    for (int item = blockIdx.x - dense_blocks; item < total; item += nb) {
        const int k = find_item(tb.first, tb.n, item);
        const int n_rows = tb.t[k].n_rows, E = tb.t[k].E;
        for (int j = 0; j < OPT_TOK / 4; ++j) {
            const int t = (item - tb.first[k]) * OPT_TOK + wave * (OPT_TOK / 4) + j;
            if (t >= n_rows) break;
            const int o = tb.t[k].scratch[t];
            if (o < 0) continue;                                   // an id outside the table
            const long long id = tb.t[k].ids[t];
            if (lane == 0) tb.t[k].owner[id] = -1;                 // the workspace convention: all -1 again, only the touched entries
            if (o != t) continue;
            const float* __restrict__ row = tb.t[k].rows + (size_t)t * E;
            float* __restrict__ w = tb.t[k].w + (size_t)id * E;
            float* __restrict__ st = ADA ? tb.t[k].state + (size_t)id * E : nullptr;
            for (int e = lane; e < E; e += WAVE) {
                float p = w[e], a = ADA ? st[e] : 0.0f;
                update_one<KIND>(p, a, row[e], coef, lr);
                w[e] = p;
                if (ADA) st[e] = a;
            }
        }
    }
}

static int dense_items(long long n) { return (int)((n + OPT_CHUNK - 1) / OPT_CHUNK); }
static int table_items(int n_rows) { return (n_rows + OPT_TOK - 1) / OPT_TOK; }

static void fill(DenseArgs& d, const gcnpt_optim_tensor_t* tensors, int n_tensors, int launch) {
    const int lo = launch * ND;
    d.n = lo < n_tensors ? std::min(ND, n_tensors - lo) : 0;
    d.first[0] = 0;
    for (int i = 0; i < d.n; ++i) { d.t[i] = tensors[lo + i]; d.first[i + 1] = d.first[i] + dense_items(tensors[lo + i].n); }
}

static void fill(TableArgs& tb, const gcnpt_optim_table_t* tables, int n_tables, int launch) {
    const int lo = launch * NT;
    tb.n = lo < n_tables ? std::min(NT, n_tables - lo) : 0;
    tb.first[0] = 0;
    for (int i = 0; i < tb.n; ++i) { tb.t[i] = tables[lo + i]; tb.first[i + 1] = tb.first[i] + table_items(tables[lo + i].n_rows); }
}

}  // namespace gcnpt

using namespace gcnpt;

extern "C" size_t gcnpt_optim_partials_floats(int n_tensors, int n_tables) {
    const int nd = n_tensors > 0 ? ceil_div(n_tensors, ND) : 0, nt = n_tables > 0 ? ceil_div(n_tables, NT) : 0;
    return 2 + (size_t)nd * OPT_DENSE_BLOCKS + (size_t)nt * OPT_TABLE_SLOTS;
}

extern "C" int gcnpt_optim_step(void* stream, int kind, const gcnpt_optim_tensor_t* tensors, int n_tensors, const gcnpt_optim_table_t* tables,
                                int n_tables, float max_norm, float lr, const float* lr_dev, int clear_grads, float* partials) {
    GCNPT_REQUIRE(kind == GCNPT_OPTIM_SGD || kind == GCNPT_OPTIM_ADAGRAD, "gcnpt_optim_step: unknown kind %d", kind);
    GCNPT_REQUIRE(n_tensors >= 0 && n_tables >= 0, "gcnpt_optim_step: negative count (n_tensors %d, n_tables %d)", n_tensors, n_tables);
    GCNPT_REQUIRE((n_tensors == 0 || tensors) && (n_tables == 0 || tables), "gcnpt_optim_step: null descriptor array");
    GCNPT_REQUIRE(partials && ((uintptr_t)partials & 3) == 0, "gcnpt_optim_step: partials is null or misaligned");
    GCNPT_REQUIRE(lr >= 0.0f, "gcnpt_optim_step: lr must be a number >= 0");
    GCNPT_REQUIRE(max_norm >= 0.0f, "gcnpt_optim_step: max_norm must be a number >= 0 (0 = no clipping)");
    GCNPT_REQUIRE(((uintptr_t)lr_dev & 3) == 0, "gcnpt_optim_step: lr_dev is misaligned");
    long long items = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const gcnpt_optim_tensor_t& t = tensors[i];
        GCNPT_REQUIRE(t.w && t.g, "gcnpt_optim_step: tensor %d: null w or g", i);
        GCNPT_REQUIRE(t.n > 0, "gcnpt_optim_step: tensor %d: n must be positive", i);
        GCNPT_REQUIRE(kind != GCNPT_OPTIM_ADAGRAD || t.state, "gcnpt_optim_step: tensor %d: Adagrad needs state", i);
        GCNPT_REQUIRE(((((uintptr_t)t.w) | ((uintptr_t)t.g) | ((uintptr_t)t.state)) & 3) == 0, "gcnpt_optim_step: tensor %d: pointers must be 4-byte aligned", i);
        items += (t.n + OPT_CHUNK - 1) / OPT_CHUNK;
    }
    for (int i = 0; i < n_tables; ++i) {
        const gcnpt_optim_table_t& t = tables[i];
        GCNPT_REQUIRE(t.V > 0 && t.E > 0, "gcnpt_optim_step: table %d: V and E must be positive", i);
        GCNPT_REQUIRE(t.n_rows >= 0, "gcnpt_optim_step: table %d: negative n_rows", i);
        GCNPT_REQUIRE(t.w && t.ids && t.rows && t.owner && t.scratch, "gcnpt_optim_step: table %d: null w, ids, rows, owner or scratch", i);
        GCNPT_REQUIRE(kind != GCNPT_OPTIM_ADAGRAD || t.state, "gcnpt_optim_step: table %d: Adagrad needs state", i);
        GCNPT_REQUIRE(((((uintptr_t)t.w) | ((uintptr_t)t.state) | ((uintptr_t)t.rows) | ((uintptr_t)t.owner) | ((uintptr_t)t.scratch)) & 3) == 0 &&
                          ((uintptr_t)t.ids & 7) == 0,
                      "gcnpt_optim_step: table %d: misaligned pointer", i);
        items += table_items(t.n_rows);
    }
    if (items >= (1LL << 31)) return fail(GCNPT_E_UNSUPPORTED, "gcnpt_optim_step: more than 2^31 work items");

    hipStream_t s = (hipStream_t)stream;
    const int deterministic = option(GCNPT_OPT_DETERMINISTIC) == 1;
    const int launches = std::max(1, std::max(ceil_div(n_tensors, ND), ceil_div(n_tables, NT)));
    DenseArgs d;
    TableArgs tb;
    int n_slots = 0;
    for (int l = 0; l < launches; ++l) {                                    // 1. dense sums of squares + owner election
        fill(d, tensors, n_tensors, l);
        fill(tb, tables, n_tables, l);
        const int db = std::min(d.first[d.n], OPT_DENSE_BLOCKS), eb = std::min(tb.first[tb.n], OPT_TABLE_BLOCKS);
        if (db + eb == 0) continue;
        hipLaunchKernelGGL(optim_sumsq_elect_kernel, dim3(db + eb), dim3(OPT_THREADS), 0, s, d, tb, db, partials + 2 + n_slots);
        GCNPT_HIP_CHECK(hipGetLastError());
        n_slots += db;
    }
    for (int l = 0; l * NT < n_tables; ++l) {                               // 2. merge duplicate ids into their owner's row
        fill(tb, tables, n_tables, l);
        if (tb.first[tb.n] == 0) continue;
        hipLaunchKernelGGL(optim_merge_kernel, dim3(std::min(tb.first[tb.n], OPT_TABLE_BLOCKS)), dim3(OPT_THREADS), 0, s, tb, deterministic);
        GCNPT_HIP_CHECK(hipGetLastError());
    }
    for (int l = 0; l * NT < n_tables; ++l) {                               // 3. the tables' share of the norm
        fill(tb, tables, n_tables, l);
        const int nb = std::min(tb.first[tb.n], OPT_TABLE_SLOTS);
        if (nb == 0) continue;
        hipLaunchKernelGGL(optim_table_sumsq_kernel, dim3(nb), dim3(OPT_THREADS), 0, s, tb, partials + 2 + n_slots);
        GCNPT_HIP_CHECK(hipGetLastError());
        n_slots += nb;
    }
    for (int l = 0; l < launches; ++l) {                                    // 4. coef, update, clear, workspace reset
        fill(d, tensors, n_tensors, l);
        fill(tb, tables, n_tables, l);
        const int db = std::min(d.first[d.n], OPT_DENSE_BLOCKS), ub = std::min(tb.first[tb.n], OPT_TABLE_BLOCKS);
        if (db + ub == 0 && l > 0) continue;
        const dim3 grid(std::max(1, db + ub));
        if (kind == GCNPT_OPTIM_ADAGRAD)
            hipLaunchKernelGGL(optim_update_kernel<GCNPT_OPTIM_ADAGRAD>, grid, dim3(OPT_THREADS), 0, s, d, tb, db, max_norm, lr, lr_dev, clear_grads,
                               partials, n_slots, l == 0);
        else
            hipLaunchKernelGGL(optim_update_kernel<GCNPT_OPTIM_SGD>, grid, dim3(OPT_THREADS), 0, s, d, tb, db, max_norm, lr, lr_dev, clear_grads,
                               partials, n_slots, l == 0);
        GCNPT_HIP_CHECK(hipGetLastError());
    }
    return GCNPT_OK;
}
