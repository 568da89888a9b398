// Activations between the padded and the token-packed layout (gfx950): gcnpt_pack_rows / gcnpt_unpack_rows move [B, T, W] rows to and
// from the [sum(len), W] rows the layer kernels run on with a PackedTrees (layout and tree arrays: tree_rewrite_kernels.hip), at the
// module boundary, so GCN.forward still returns [B, T, H] (model/gcn.py:395).  gcnpt_pack_ids is the integer counterpart of gcnpt_pack_rows
// for the loader's int64 [B, T] id tensors (deprel: the relation-aware layers index their embedding table with the packed array).
#include "layer_common.h"

namespace gcnpt {

constexpr int PK_THREADS = 256;

// rows of a [B, T, W] tensor <-> packed [N, W]; VB = bytes per copy piece (16 or the element size); one workgroup per 8 token slots.
// FILL (gcnpt_pack_ids; pack direction, 8-byte pieces): the packed side has n_rows rows, no row outside [0, n_rows) is written, and one
// more row of workgroups (blockIdx.y = B) writes `fill` to the rows from cu[B] on, which belong to no sentence.
template <int VB, bool UNPACK, bool FILL = false>
__global__ __launch_bounds__(PK_THREADS) void move_rows_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                             const int32_t* __restrict__ cu, int B, int T, size_t row_bytes, int n_rows,
                                                             unsigned long long fill) {
    const int b = blockIdx.y, i0 = blockIdx.x * 8;
    const size_t pieces = row_bytes / VB;
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));  // (first-class vector: a select between uint4 structs went through scratch memory)
    typedef typename std::conditional<VB == 16, u32x4_t, typename std::conditional<VB == 8, unsigned long long,
            typename std::conditional<VB == 4, unsigned, unsigned short>::type>::type>::type V;
    if constexpr (FILL) {
        if (b == B) {
            for (long long r = (long long)min(max(cu[B], 0), n_rows) + blockIdx.x; r < n_rows; r += gridDim.x)
                for (size_t q = threadIdx.x; q < pieces; q += PK_THREADS) *reinterpret_cast<V*>(dst + (size_t)r * row_bytes + q * VB) = (V)fill;
            return;
        }
    }
    const int base = cu[b], len = cu[b + 1] - base;
    for (int i = i0; i < min(i0 + 8, T); ++i) {
        const size_t padded = ((size_t)b * T + i) * row_bytes, packed = ((size_t)base + i) * row_bytes;
        if (UNPACK) {
            V z{};
            for (size_t q = threadIdx.x; q < pieces; q += PK_THREADS)
                *reinterpret_cast<V*>(dst + padded + q * VB) = i < len ? *reinterpret_cast<const V*>(src + packed + q * VB) : z;
        } else if (i < len && (!FILL || (base + i >= 0 && base + i < n_rows))) {
            for (size_t q = threadIdx.x; q < pieces; q += PK_THREADS)
                *reinterpret_cast<V*>(dst + packed + q * VB) = *reinterpret_cast<const V*>(src + padded + q * VB);
        }
    }
}

}  // namespace gcnpt

using namespace gcnpt;

template <bool UNPACK>
static int move_rows(void* stream, const void* src, int dtype, const int32_t* cu, int B, int T, int W, void* dst, const char* what) {
    GCNPT_REQUIRE(src && dst && cu, "%s: null pointer", what);
    GCNPT_REQUIRE(B > 0 && T > 0 && W > 0, "%s: sizes must be positive", what);
    GCNPT_REQUIRE(dtype_ok(dtype), "%s: bad dtype", what);
    const size_t rb = (size_t)W * esize(dtype);
    const unsigned char* a = static_cast<const unsigned char*>(src);
    unsigned char* d = static_cast<unsigned char*>(dst);
    const dim3 grid(ceil_div(T, 8), B);
    hipStream_t s = (hipStream_t)stream;
    if (rb % 16 == 0 && aligned16(src) && aligned16(dst)) hipLaunchKernelGGL((move_rows_kernel<16, UNPACK>), grid, dim3(PK_THREADS), 0, s, a, d, cu, B, T, rb, 0, 0ull);
    else if (dtype == GCNPT_F32) hipLaunchKernelGGL((move_rows_kernel<4, UNPACK>), grid, dim3(PK_THREADS), 0, s, a, d, cu, B, T, rb, 0, 0ull);
    else hipLaunchKernelGGL((move_rows_kernel<2, UNPACK>), grid, dim3(PK_THREADS), 0, s, a, d, cu, B, T, rb, 0, 0ull);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}

extern "C" int gcnpt_pack_rows(void* stream, const void* src, int dtype, const int32_t* cu_seqlens, int B, int T, int W, void* dst) {
    return move_rows<false>(stream, src, dtype, cu_seqlens, B, T, W, dst, "pack_rows");
}
extern "C" int gcnpt_unpack_rows(void* stream, const void* src, int dtype, const int32_t* cu_seqlens, int B, int T, int W, void* dst) {
    return move_rows<true>(stream, src, dtype, cu_seqlens, B, T, W, dst, "unpack_rows");
}

extern "C" int gcnpt_pack_ids(void* stream, const int64_t* src, const int32_t* cu_seqlens, int B, int T, int64_t* dst, int n_rows, int64_t fill) {
    GCNPT_REQUIRE(src && dst && cu_seqlens, "pack_ids: null pointer");
    GCNPT_REQUIRE(B > 0 && T > 0 && n_rows > 0, "pack_ids: sizes must be positive");
    hipLaunchKernelGGL((move_rows_kernel<8, false, true>), dim3(ceil_div(T, 8), B + 1), dim3(PK_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned char*>(src), reinterpret_cast<unsigned char*>(dst), cu_seqlens, B, T, sizeof(int64_t), n_rows,
                       (unsigned long long)fill);
    GCNPT_HIP_CHECK(hipGetLastError());
    return GCNPT_OK;
}
