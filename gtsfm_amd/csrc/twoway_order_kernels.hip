// Device-resident glue between the two-way matcher and the batched verifier for the classical front ends (SIFT / D2-Net +
// TwoWayMatcher + Ransac). See include/gtsfm_amd.h.
//
//   tw_order_kernel : gtsfm_twoway_match's matches0 / dist0 blocks -> per pair the kept rows (i, matches0[i]) in the
//                     TwoWayMatcher contract's order: by float32 distance ascending, ties by i ascending. Kept rows have
//                     a distance >= 0 that is never NaN, so the float's bit pattern orders as an unsigned integer and
//                     key(i) = bits(dist0[i]) << 32 | i is a total order without ties. A row's output slot is its RANK:
//                     the number of kept keys below its own. A workgroup owns 256 rows of a pair (one per thread) and
//                     streams ALL of the pair's keys through LDS tiles, every lane reading the same LDS word (a broadcast,
//                     no bank conflict) and adding one integer compare per key. There is no floating-point arithmetic, no
//                     atomic on the output and no workspace; the slots are a permutation of 0 .. K-1 by construction, so
//                     the result does not depend on the grid or on timing. Rows that are not kept carry the all-ones key,
//                     which is below nothing.
//   pack_rows_u8_kernel: float32 rows holding the integers 0 .. 255 (SIFT descriptors as OpenCV emits them) -> uint8 rows;
//                     any other value writes 0 and raises a flag, nothing is clamped.

#include "../../include/gtsfm_amd.h"
#include "common.h"

#define TWO_ROWS 256      // rows of a pair per workgroup, one per thread
#define TWO_TILE 2048     // keys per LDS tile (16 KiB)
#define TWO_BLOCKS_Y 32   // workgroups per pair; a pair with more than 32 * 256 rows loops
#define TWO_NOT_KEPT 0xffffffffffffffffull

namespace {

__device__ __forceinline__ unsigned long long tw_order_key(const int* __restrict__ m0, const float* __restrict__ d0, long long row, long long n) {
    if (row >= n || m0[row] < 0) return TWO_NOT_KEPT;
    const float d = d0[row] + 0.0f;  // -0.0f -> +0.0f: they compare equal as floats and must as integers
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(unsigned int)row;
}

__global__ __launch_bounds__(TWO_ROWS) void tw_order_kernel(const int* __restrict__ matches0, const float* __restrict__ dist0,
                                                            const long long* __restrict__ blk_off, int* __restrict__ match_idx,
                                                            int* __restrict__ match_count) {
    __shared__ unsigned long long tile[TWO_TILE];
    __shared__ int kept_total;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const long long first = blk_off[pair];
    const long long n = blk_off[pair + 1] - first;
    const int* m0 = matches0 + first;
    const float* d0 = dist0 + first;
    int* dst = match_idx + 2 * first;
    if (blockIdx.y == 0) {  // K_p: an integer count of the kept rows, by the pair's first workgroup
        if (tid == 0) kept_total = 0;
        __syncthreads();
        int mine = 0;
        for (long long r = tid; r < n; r += TWO_ROWS) mine += m0[r] >= 0;
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);  // integers: the order of the sum does not matter
        if ((tid & 63) == 0) atomicAdd(&kept_total, mine);
        __syncthreads();
        if (tid == 0) match_count[pair] = kept_total;
    }
    for (long long base = (long long)blockIdx.y * TWO_ROWS; base < n; base += (long long)gridDim.y * TWO_ROWS) {
        const long long row = base + tid;
        const unsigned long long key = tw_order_key(m0, d0, row, n);
        // a chunk without a kept row has nothing to place (uniform over the workgroup, so the barriers below stay matched)
        if (!__syncthreads_or(key != TWO_NOT_KEPT)) continue;
        int rank = 0;
        for (long long t0 = 0; t0 < n; t0 += TWO_TILE) {
            __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
            for (int k = 0; k < TWO_TILE / TWO_ROWS; ++k) tile[k * TWO_ROWS + tid] = tw_order_key(m0, d0, t0 + k * TWO_ROWS + tid, n);
            __syncthreads();
            const ulonglong2* t2 = (const ulonglong2*)tile;
#pragma unroll 8
            for (int j = 0; j < TWO_TILE / 2; ++j) {  // keys past the pair's end are all-ones: below nothing
                const ulonglong2 v = t2[j];
                rank += (v.x < key) + (v.y < key);
            }
        }
        if (key != TWO_NOT_KEPT) {
            dst[2 * (long long)rank] = (int)row;
            dst[2 * (long long)rank + 1] = m0[row];
        }
    }
}

__global__ __launch_bounds__(256) void pack_rows_u8_kernel(const float* __restrict__ src, long long rows, int dim, int src_stride,
                                                        uint8_t* __restrict__ dst, int dst_stride, int* __restrict__ flag) {
    const long long total = rows * dim;
    bool bad = false;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / dim;
        const int c = (int)(e - r * dim);
        const float v = src[r * src_stride + c];
        const bool ok = v >= 0.f && v <= 255.f && v == truncf(v);  // false for NaN
        dst[r * dst_stride + c] = ok ? (uint8_t)(int)v : (uint8_t)0;
        bad |= !ok;
    }
    if (bad) atomicOr(flag, 1);
}

}  // namespace

extern "C" int gtsfm_twoway_order_matches(const int32_t* matches0_dev, const float* dist0_dev, const long long* blk_off_dev, int num_pairs,
                                          int32_t* match_idx_dev, int32_t* match_count_dev, void* stream) {
    GTSFM_CHECK_ARG(num_pairs >= 0 && num_pairs <= 65535, "twoway_order_matches: pair count %d outside 0 .. 65535", num_pairs);
    GTSFM_CHECK_ARG(matches0_dev && dist0_dev && blk_off_dev && match_idx_dev && match_count_dev, "twoway_order_matches: null pointer");
    if (num_pairs == 0) return GTSFM_OK;
    hipLaunchKernelGGL(tw_order_kernel, dim3(num_pairs, TWO_BLOCKS_Y), dim3(TWO_ROWS), 0, (hipStream_t)stream, matches0_dev, dist0_dev, blk_off_dev,
                       match_idx_dev, match_count_dev);
    GTSFM_CHECK_LAUNCH("tw_order_kernel");
    return GTSFM_OK;
}

extern "C" int gtsfm_pack_rows_f32_to_u8(const float* src_dev, long long rows, int dim, int src_stride, uint8_t* dst_dev, int dst_stride,
                                         int32_t* flag_dev, void* stream) {
    GTSFM_CHECK_ARG(rows >= 0 && dim >= 1, "pack_rows_f32_to_u8: bad sizes (%lld rows of %d)", rows, dim);
    GTSFM_CHECK_ARG(src_stride >= dim && dst_stride >= dim, "pack_rows_f32_to_u8: a row stride (%d, %d) is below the row length %d", src_stride,
                    dst_stride, dim);
    GTSFM_CHECK_ARG(src_dev && dst_dev && flag_dev, "pack_rows_f32_to_u8: null pointer");
    if (rows == 0) return GTSFM_OK;
    const long long blocks = (rows * dim + 255) / 256;
    hipLaunchKernelGGL(pack_rows_u8_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, src_dev, rows, dim,
                       src_stride, dst_dev, dst_stride, flag_dev);
    GTSFM_CHECK_LAUNCH("pack_rows_u8_kernel");
    return GTSFM_OK;
}
