// y = normalise(W x + bias) for a few long vectors against a weight matrix far larger than the caches (NetVLAD's whitening
// 32768 -> 4096, MegaLoc's output projection 16640 -> 8448): memory-bound. The matrix is streamed once per group of IMG images, i.e.
// ceil(B / IMG) times per launch: once for NetVLAD's batches of 4 (IMG = 4); MegaLoc (IMG = 8) streams its 562 MB twice at batch 16 and
// eight times at batch 64 (the later passes partly out of the last-level cache; DESIGN.md section 4 has the figures).
// Split-K: slice s covers depths [s * 256 * F4, (s + 1) * 256 * F4); a workgroup holds its slice of IMG images in registers, a wave
// walks 16 output columns and reads each weight row piece as float4 (1 KB per wave instruction); sk_finish_kernel sums the
// slices in order, adds the bias and divides by max(||y||, 1e-12). Every image's values follow one operation order whatever the batch.
#pragma once

#include "common.h"

#define SK_IMG 4  // images per workgroup (default)

// part[s][b][n] = sum over slice s of w[n][k] x[b][k]. grid (N / 64, K / (256 * F4), ceil(B / IMG)), 256 threads; N % 64 == 0, K % (256 * F4) == 0.
template <int F4, int IMG = SK_IMG>
__global__ __launch_bounds__(256) void sk_linear_kernel(const float* __restrict__ x, const float* __restrict__ w, int K, int N, int B, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.y, b0 = blockIdx.z * IMG;
    const size_t k0 = (size_t)s * (256 * F4) + 4 * lane;
    f32x4 xr[IMG][F4];
#pragma unroll
    for (int bi = 0; bi < IMG; ++bi)
#pragma unroll
        for (int i = 0; i < F4; ++i)
            xr[bi][i] = (b0 + bi < B) ? *reinterpret_cast<const f32x4*>(x + (size_t)(b0 + bi) * K + k0 + 256 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int col = 0; col < 16; ++col) {
        const int n = blockIdx.x * 64 + wave * 16 + col;
        const float* wr = w + (size_t)n * K + k0;
        f32x4 wv[F4];
#pragma unroll
        for (int i = 0; i < F4; ++i) wv[i] = *reinterpret_cast<const f32x4*>(wr + 256 * i);
#pragma unroll
        for (int bi = 0; bi < IMG; ++bi) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < F4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = fmaf(wv[i][e], xr[bi][i][e], acc);
            acc = wave_sum(acc);
            if (lane == 0 && b0 + bi < B) part[((size_t)s * B + b0 + bi) * N + n] = acc;
        }
    }
}

// out[b] = y / max(||y||, 1e-12), y[n] = (sum of the NS slices in order) + bias[n] (one workgroup of NT threads per image; thread t owns
// n = t, t + NT, ...; the slice loop is unrolled so that its NS loads are in flight together).
template <int NS, int NT>
__global__ __launch_bounds__(NT) void sk_finish_kernel(const float* __restrict__ part, const float* __restrict__ bias, int N, int B, float* __restrict__ out) {
    __shared__ float red[NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    float g = 0.f;
    for (int n = tid; n < N; n += NT) {
        float v[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) v[s] = part[((size_t)s * B + b) * N + n];
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) acc += v[s];
        const float y = acc + bias[n];
        out[(size_t)b * N + n] = y;  // (read back below by the thread that wrote it)
        g = fmaf(y, y, g);
    }
    g = wave_sum(g);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = g;
    __syncthreads();
    float sum = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) sum += red[i];
    const float gn = fmaxf(sqrtf(sum), 1e-12f);
    for (int n = tid; n < N; n += NT) out[(size_t)b * N + n] = out[(size_t)b * N + n] / gn;
}
