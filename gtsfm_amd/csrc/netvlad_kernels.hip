// NetVLAD global descriptors (thirdparty/hloc/netvlad.py) and similarity retrieval (gtsfm/retriever/similarity_retriever.py):
// the device side of gtsfm_amd.frontend.global_descriptor.NetVLADGlobalDescriptor and gtsfm_amd.retriever.SimilarityRetriever.
// See include/gtsfm_amd.h.
//
// Forward (all exact fp32):
//   1. vgg_conv1_kernel<NvLoad> (vgg_trunk.h, shared with D2-Net): conv1_1 (3 -> 64) + ReLU on the VALU, with the reference's
//                           preprocessing applied while the input tile is staged: clamp(x * 255, 0, 255) - mean[c] (netvlad.py:178-182; std = 1). Reads the plugin's
//                           [B][3][H][W] float image or a [B][H][W][3] uint8 one (float(u8) is what (u8 / 255) * 255 gives back).
//                           Sets *range_flag when a float input lies outside [-1e-6, 1 + 1e-6] or is NaN (netvlad.py:177).
//   2. conv1_2 .. conv5_3 : launch_conv3x3 (dense_kernels.hip), max-pool fused after conv1_2 / 2_2 / 3_3 / 4_3, no ReLU after conv5_3.
//   3. nv_rownorm_kernel  : per-pixel L2 normalisation over the 512 channels (F.normalize, netvlad.py:191).
//   4. scores             : launch_gemm (LDS-DMA, exact fp32) of the normalised pixels and score_proj (netvlad.py:65).
//   5. nv_softmax64_kernel: softmax over the 64 clusters.
//   6. nv_vlad_kernel     : V[d][k] = sum_n a[k][n] (x[d][n] - c[d][k]) in the residual form (netvlad.py:67-68) without the
//                           (B, 512, 64, HW) difference tensor: 64-pixel chunks summed in order, chunk sums added in order.
//   7. nv_vlad_norm_kernel: intra-normalisation per cluster, flatten at d * 64 + k, global normalisation (netvlad.py:69-72).
//   8. sk_linear_kernel   : whitening 32768 -> 4096 as a split-K product (splitk_linear.h, shared with MegaLoc's output projection: 16
//                           slices of 2048, four images per workgroup, a wave per output column); sk_finish_kernel sums the slices in
//                           order, adds the bias and normalises.
// Every image's values follow the same operation order whatever the batch, so a batch equals its images one at a time, bit for bit.
//
// Retrieval: S = D D^T through ONE batched launch of the LDS-DMA GEMM over row strips of 1024 (each strip from its diagonal block
// on: about half the matrix), then rt_topk_kernel, one wave per row, keeps the min(k, N) best columns j > i with S[i][j] >=
// min_score in descending order, equal scores by the lower column (a register-resident list of 64 per pass; k > 64 takes
// several passes, each below the previous pass's last entry).

#include <limits.h>
#include <math.h>

#include "../../include/gtsfm_amd.h"
#include "common.h"
#include "conv_kernels.h"
#include "gemm_batch.h"
#include "gemm_kernels.h"
#include "splitk_linear.h"
#include "vgg_trunk.h"

#define NV_LAYERS VGG_LAYERS  // the whole trunk: conv1_1 .. conv5_3
#define NV_D 512
#define NV_K 64
#define NV_VLAD (NV_D * NV_K)  // 32768
#define NV_WHITE 4096
#define NV_WSLICE 2048                 // depth of one whitening slice
#define NV_WSPLIT (NV_VLAD / NV_WSLICE)  // 16
#define RT_STRIP 1024                  // rows per retrieval GEMM problem

namespace {

const int kPool[NV_LAYERS] = {0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0};

// Offsets (floats) of the packed blob: the 13 convolutions (vgg_conv_layout), score_proj [64][512], centres [512][64], mean [4], then
// (with whitening) W [4096][32768] row-major and its bias.
struct NvLayout {
    size_t w[NV_LAYERS], b[NV_LAYERS], score, centers, mean, ww, wb, total_plain, total_white;
};

NvLayout nv_layout() {
    NvLayout L;
    size_t o = vgg_conv_layout(NV_LAYERS, L.w, L.b);
    L.score = o, o += a64((size_t)NV_K * NV_D);
    L.centers = o, o += a64((size_t)NV_D * NV_K);
    L.mean = o, o += 64;
    L.total_plain = o;
    L.ww = o, o += (size_t)NV_WHITE * NV_VLAD;
    L.wb = o, o += a64(NV_WHITE);
    L.total_white = o;
    return L;
}

// Workspace (bytes, 256-aligned pieces): flag | act A [B][H][W][64] | act B [B][H/2][W/2][64] | scores | vlad | whitening slices.
struct NvWs {
    size_t actA, actB, scores, vlad, part, total;
};

NvWs nv_ws(int B, int H, int W) {
    NvWs s;
    const size_t hw = (size_t)H * W, hw5 = (size_t)(H / 16) * (W / 16);
    WorkspaceCarver c = {};
    c.offset(4);  // the range flag of a call that passes none
    s.actA = c.offset((size_t)B * hw * 64 * 4);
    s.actB = c.offset((size_t)B * (hw / 4 + 1) * 64 * 4);
    s.scores = c.offset((size_t)B * hw5 * NV_K * 4);
    s.vlad = c.offset((size_t)B * NV_VLAD * 4);
    s.part = c.offset((size_t)NV_WSPLIT * B * NV_WHITE * 4);
    s.total = c.used;
    return s;
}

// conv1_1's pixel fetch (vgg_conv1_kernel) with the reference's preprocessing: clamp(x * 255, 0, 255) - mean[c] of a float image
// [B][3][H][W], raising *range_flag when x lies outside [-1e-6, 1 + 1e-6] or is NaN; float(u8) - mean[c] of a uint8 image [B][H][W][3].
struct NvLoad {
    const void* img;
    int u8;
    const float* mean;
    int* range_flag;
    __device__ float operator()(size_t b, int c, int gy, int gx, int H, int W) const {
        if (u8) return (float)reinterpret_cast<const uint8_t*>(img)[((b * H + gy) * W + gx) * 3 + c] - mean[c];
        const float lo = (float)(-1e-6), hi = (float)(1.0 + 1e-6);
        const float x = reinterpret_cast<const float*>(img)[((b * 3 + c) * H + gy) * (size_t)W + gx];
        if (!(x >= lo && x <= hi)) atomicOr(range_flag, 1);
        return fminf(fmaxf(x * 255.0f, 0.0f), 255.0f) - mean[c];
    }
};

// x / max(||x||, 1e-12) over rows of 512 (one wave per row, in place).
__global__ __launch_bounds__(256) void nv_rownorm_kernel(float* __restrict__ x, long long rows) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    f32x4* r = reinterpret_cast<f32x4*>(x + row * NV_D);
    f32x4 v0 = r[lane], v1 = r[lane + 64];
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) ss = fmaf(v0[e], v0[e], ss);
#pragma unroll
    for (int e = 0; e < 4; ++e) ss = fmaf(v1[e], v1[e], ss);
    const float n = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v0[e] = v0[e] / n, v1[e] = v1[e] / n;
    r[lane] = v0;
    r[lane + 64] = v1;
}

// softmax over the 64 cluster scores of a pixel (one wave per pixel, lane = cluster, in place).
__global__ __launch_bounds__(256) void nv_softmax64_kernel(float* __restrict__ s, long long rows) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float v = s[row * NV_K + lane];
    const float e = expf(v - wave_max(v));
    s[row * NV_K + lane] = e / wave_sum(e);
}

// V[b][d][k] = sum_n a[b][n][k] (x[b][n][d] - c[d][k]). Workgroup = 16 d x 64 k of one image; thread = one k, four d.
__global__ __launch_bounds__(256) void nv_vlad_kernel(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ centers,
                                                    int hw, float* __restrict__ v) {
    __shared__ float as[64 * NV_K];
    __shared__ float xs[64 * 16];
    const int tid = threadIdx.x, k = tid & 63, dg = tid >> 6;
    const int d0 = blockIdx.x * 16;
    const size_t b = blockIdx.y;
    const float* xb = x + b * hw * NV_D;
    const float* ab = a + b * hw * NV_K;
    float c[4], total[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = centers[(d0 + dg * 4 + i) * NV_K + k];
    for (int n0 = 0; n0 < hw; n0 += 64) {
        const int nmax = min(64, hw - n0);
        __syncthreads();
        for (int idx = tid; idx < 64 * NV_K; idx += 256) as[idx] = (idx >> 6) < nmax ? ab[(size_t)(n0 + (idx >> 6)) * NV_K + (idx & 63)] : 0.f;
        for (int idx = tid; idx < 64 * 16; idx += 256) xs[idx] = (idx >> 4) < nmax ? xb[(size_t)(n0 + (idx >> 4)) * NV_D + d0 + (idx & 15)] : 0.f;
        __syncthreads();
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        for (int n = 0; n < nmax; ++n) {
            const float av = as[n * NV_K + k];
#pragma unroll
            for (int i = 0; i < 4; ++i) part[i] = fmaf(av, xs[n * 16 + dg * 4 + i] - c[i], part[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) total[i] += part[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[(b * NV_D + d0 + dg * 4 + i) * NV_K + k] = total[i];
}

__device__ float block_sum256(float v, float* red) {  // 256 threads; result in every thread
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// Intra-normalisation of each cluster's 512-vector, then the global normalisation of the 32768-vector (one workgroup per image).
__global__ __launch_bounds__(256) void nv_vlad_norm_kernel(const float* __restrict__ v, float* __restrict__ out) {
    __shared__ float part[4][NV_K];
    __shared__ float nk[NV_K];
    __shared__ float red[4];
    const int tid = threadIdx.x, k = tid & 63, q = tid >> 6;
    const float* vb = v + (size_t)blockIdx.x * NV_VLAD;
    float* ob = out + (size_t)blockIdx.x * NV_VLAD;
    float ss = 0.f;
    for (int d = q * 128; d < q * 128 + 128; ++d) ss = fmaf(vb[d * NV_K + k], vb[d * NV_K + k], ss);
    part[q][k] = ss;
    __syncthreads();
    if (tid < NV_K) nk[tid] = fmaxf(sqrtf(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]), 1e-12f);
    __syncthreads();
    float g = 0.f;
    for (int idx = tid; idx < NV_VLAD; idx += 256) {
        const float x = vb[idx] / nk[idx & 63];
        ob[idx] = x;
        g = fmaf(x, x, g);
    }
    const float gn = fmaxf(sqrtf(block_sum256(g, red)), 1e-12f);
    for (int idx = tid; idx < NV_VLAD; idx += 256) ob[idx] = ob[idx] / gn;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Retrieval
// ------------------------------------------------------------------------------------------------------------------------------

// desc [n][d] -> [n][dp] with zero columns (exact: the added products are 0 * 0).
__global__ void rt_pad_kernel(const float* __restrict__ src, int n, int d, int dp, float* __restrict__ dst) {
    const size_t total = (size_t)n * dp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t r = idx / dp;
        const int c = (int)(idx % dp);
        dst[idx] = c < d ? src[r * d + c] : 0.f;
    }
}

// Problem r of the strip GEMM: rows [r0, r0 + min(1024, n - r0)) against columns [col0, n), col0 = the start of the block (of
// `blocksize` columns) holding row r0, rounded down to a multiple of 4 (16-byte aligned output rows).
__global__ void rt_problems_kernel(int n, int blocksize, int nstrips, GemmProblem* __restrict__ pr, int* __restrict__ counts) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nstrips) return;
    const int r0 = r * RT_STRIP;
    const int col0 = ((r0 / blocksize) * blocksize) & ~3;
    GemmProblem p;
    p.c_off = (long long)r0 * n + col0;
    p.a_row = r0, p.w_row = col0, p.m_idx = 2 * r, p.n_idx = 2 * r + 1, p.ldc = n, p.pad = 0;
    pr[r] = p;
    counts[2 * r] = min(RT_STRIP, n - r0);
    counts[2 * r + 1] = n - col0;
}

// The reference's block layout of the similarity matrix: (i, j) is 0 unless j / blocksize >= i / blocksize.
__global__ void rt_block_mask_kernel(float* __restrict__ sim, int n, int blocksize) {
    const int i = blockIdx.y;
    const int jend = (i / blocksize) * blocksize;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < jend; j += gridDim.x * blockDim.x) sim[(size_t)i * n + j] = 0.f;
}

__device__ __forceinline__ bool rt_better(float s1, int j1, float s2, int j2) { return s1 > s2 || (s1 == s2 && j1 < j2); }

// Row-wise top-k of the masked similarity (one wave per row). Lane l of the list holds rank base + l; an empty slot is (-inf, INT_MAX).
__global__ __launch_bounds__(256) void rt_topk_kernel(const float* __restrict__ sim, int n, int kk, float min_score, int32_t* __restrict__ idx_out,
                                                    float* __restrict__ score_out) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const float* row = sim + (size_t)i * n;
    float bound_s = INFINITY;
    int bound_j = -1;  // candidates of a pass rank strictly below (bound_s, bound_j)
    for (int base = 0; base < kk; base += 64) {
        const int kp = min(64, kk - base);
        float ls = -INFINITY;
        int lj = INT_MAX;
        for (int j0 = i + 1; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const float s = j < n ? row[j] : 0.f;
            float ts = __shfl(ls, kp - 1, 64);
            int tj = __shfl(lj, kp - 1, 64);
            const bool ok = j < n && isfinite(s) && s >= min_score && rt_better(bound_s, bound_j, s, j) && rt_better(s, j, ts, tj);
            unsigned long long mask = __ballot(ok);
            while (mask) {
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const float cs = __shfl(s, src, 64);
                const int cj = j0 + src;
                ts = __shfl(ls, kp - 1, 64);
                tj = __shfl(lj, kp - 1, 64);
                if (!rt_better(cs, cj, ts, tj)) continue;
                const int pos = __popcll(__ballot(lane < kp && rt_better(ls, lj, cs, cj)));
                const float us = __shfl_up(ls, 1, 64);
                const int uj = __shfl_up(lj, 1, 64);
                if (lane > pos) ls = us, lj = uj;
                else if (lane == pos) ls = cs, lj = cj;
            }
        }
        if (lane < kp) {
            idx_out[(size_t)i * kk + base + lane] = lj == INT_MAX ? -1 : lj;
            score_out[(size_t)i * kk + base + lane] = lj == INT_MAX ? -INFINITY : ls;
        }
        bound_s = __shfl(ls, kp - 1, 64);
        bound_j = __shfl(lj, kp - 1, 64);
        if (bound_j == INT_MAX) {  // this pass ran out of candidates: the remaining ranks are empty
            for (int r = base + 64 + lane; r < kk; r += 64) idx_out[(size_t)i * kk + r] = -1, score_out[(size_t)i * kk + r] = -INFINITY;
            break;
        }
    }
}

int nv_run(const float* wts, const void* image, int layout, int B, int H, int W, int stage, int whiten, float* out, int32_t* range_flag,
           void* ws, size_t ws_bytes, hipStream_t st) {
    GTSFM_CHECK_ARG(wts && image && out && ws, "netvlad: null pointer");
    GTSFM_CHECK_ARG(layout == 0 || layout == 1, "netvlad: layout must be 0 (float [B][3][H][W]) or 1 (uint8 [B][H][W][3]) (got %d)", layout);
    // (the reference raises too below 16 px: its fourth max-pool would have an empty output)
    GTSFM_CHECK_ARG(B >= 1 && H >= 16 && W >= 16, "netvlad: need batch >= 1 and images of at least 16 x 16 (got %d x %d x %d)", B, H, W);
    // every argument check before the first launch: a refused call enqueues nothing
    GTSFM_CHECK_ARG(stage < 2 || gemm_uses_dma(NV_D, NV_D), "netvlad: the score product needs the LDS-DMA GEMM (GTSFM_GEMM=mfma is not supported here)");
    const NvWs s = nv_ws(B, H, W);
    GTSFM_CHECK_ARG(ws_bytes >= s.total, "netvlad: workspace too small (%zu < %zu bytes)", ws_bytes, s.total);
    const NvLayout L = nv_layout();
    char* base = reinterpret_cast<char*>(ws);
    float* act[2] = {reinterpret_cast<float*>(base + s.actA), reinterpret_cast<float*>(base + s.actB)};
    int* flag = range_flag ? range_flag : reinterpret_cast<int*>(base);
    if (!range_flag && hipMemsetAsync(flag, 0, 4, st) != hipSuccess) {
        gtsfm_set_error("netvlad: hipMemsetAsync failed");
        return GTSFM_ERR_HIP;
    }
    vgg_launch_conv1(NvLoad{image, layout, wts + L.mean, flag}, B, H, W, wts + L.w[0], wts + L.b[0], act[0], st);
    GTSFM_CHECK_LAUNCH("vgg_conv1_kernel<NvLoad>");
    if (stage == 0) return hipMemcpyAsync(out, act[0], (size_t)B * H * W * 64 * 4, hipMemcpyDeviceToDevice, st) == hipSuccess ? GTSFM_OK : GTSFM_ERR_HIP;
    int h = H, w = W;
    for (int l = 1; l < NV_LAYERS; ++l) {
        const int rc = vgg_conv_layer(l, act[(l - 1) & 1], act[l & 1], wts + L.w[l], wts + L.b[l], B, h, w, l != NV_LAYERS - 1, kPool[l], false, st);
        if (rc) return rc;
        if (kPool[l]) h >>= 1, w >>= 1;
    }
    float* feat = act[(NV_LAYERS - 1) & 1];  // conv5_3: [B][h][w][512]
    const long long rows = (long long)B * h * w;
    if (stage == 1) return hipMemcpyAsync(out, feat, (size_t)rows * NV_D * 4, hipMemcpyDeviceToDevice, st) == hipSuccess ? GTSFM_OK : GTSFM_ERR_HIP;
    hipLaunchKernelGGL(nv_rownorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, feat, rows);
    GTSFM_CHECK_LAUNCH("nv_rownorm_kernel");
    float* scores = reinterpret_cast<float*>(base + s.scores);
    {
        GemmParams g = {};
        g.A = feat, g.lda = NV_D, g.M = (int)rows, g.K = NV_D;
        g.wraw = wts + L.score, g.ldw = NV_D, g.N = NV_K;
        g.C = scores, g.ldc = NV_K, g.alpha = 1.f;
        g.math = 0;
        const int rc = launch_gemm(g, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(nv_softmax64_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, scores, rows);
    GTSFM_CHECK_LAUNCH("nv_softmax64_kernel");
    float* vlad = reinterpret_cast<float*>(base + s.vlad);
    float* vlad_out = (stage == 2 || !whiten) ? out : vlad;
    hipLaunchKernelGGL(nv_vlad_kernel, dim3(NV_D / 16, B), dim3(256), 0, st, feat, scores, wts + L.centers, h * w, vlad);
    GTSFM_CHECK_LAUNCH("nv_vlad_kernel");
    hipLaunchKernelGGL(nv_vlad_norm_kernel, dim3(B), dim3(256), 0, st, vlad, vlad_out);
    GTSFM_CHECK_LAUNCH("nv_vlad_norm_kernel");
    if (stage == 2 || !whiten) return GTSFM_OK;
    float* part = reinterpret_cast<float*>(base + s.part);
    hipLaunchKernelGGL(sk_linear_kernel<NV_WSLICE / 256>, dim3(NV_WHITE / 64, NV_WSPLIT, ceil_div(B, SK_IMG)), dim3(256), 0, st, vlad, wts + L.ww, NV_VLAD,
                       NV_WHITE, B, part);
    GTSFM_CHECK_LAUNCH("sk_linear_kernel");
    hipLaunchKernelGGL((sk_finish_kernel<NV_WSPLIT, 256>), dim3(B), dim3(256), 0, st, part, wts + L.wb, NV_WHITE, B, out);
    GTSFM_CHECK_LAUNCH("sk_finish_kernel");
    return GTSFM_OK;
}

struct RtWs {
    size_t pad, sim, problems, counts, total;
};

RtWs rt_ws(int n, int d, int with_sim_out) {
    RtWs s;
    const int dp = (d + 31) / 32 * 32;
    const int nstrips = ceil_div(n, RT_STRIP);
    WorkspaceCarver c = {};
    s.pad = c.offset(d % 32 ? (size_t)n * dp * 4 : 0);
    s.sim = c.offset(with_sim_out ? 0 : (size_t)n * n * 4);
    s.problems = c.offset((size_t)nstrips * sizeof(GemmProblem));
    s.counts = c.offset((size_t)nstrips * 2 * 4);
    s.total = c.used;
    return s;
}

}  // namespace

extern "C" {

size_t gtsfm_netvlad_packed_weight_floats(int whiten) {
    const NvLayout L = nv_layout();
    return whiten ? L.total_white : L.total_plain;
}

int gtsfm_netvlad_pack_weights(const float* const* t, int whiten, float* packed) {
    GTSFM_CHECK_ARG(t && packed, "netvlad_pack_weights: null pointer");
    const int count = whiten ? 31 : 29;
    for (int i = 0; i < count; ++i) GTSFM_CHECK_ARG(t[i], "netvlad_pack_weights: tensor %d is null", i);
    const NvLayout L = nv_layout();
    const size_t total = whiten ? L.total_white : L.total_plain;
    for (size_t i = 0; i < L.total_plain; ++i) packed[i] = 0.f;
    vgg_pack_convs(t, NV_LAYERS, L.w, L.b, packed);
    for (int i = 0; i < NV_K * NV_D; ++i) packed[L.score + i] = t[26][i];
    for (int i = 0; i < NV_D * NV_K; ++i) packed[L.centers + i] = t[27][i];
    for (int c = 0; c < 3; ++c) packed[L.mean + c] = t[28][c];
    if (whiten) {
        for (size_t i = 0; i < (size_t)NV_WHITE * NV_VLAD; ++i) packed[L.ww + i] = t[29][i];
        for (size_t i = L.wb; i < total; ++i) packed[i] = 0.f;
        for (int i = 0; i < NV_WHITE; ++i) packed[L.wb + i] = t[30][i];
    }
    return GTSFM_OK;
}

size_t gtsfm_netvlad_workspace_bytes(int batch, int height, int width) {
    if (batch < 1 || height < 16 || width < 16) return 0;
    return nv_ws(batch, height, width).total;
}

int gtsfm_netvlad_forward(const float* packed_weights_dev, const void* image_dev, int layout, int batch, int height, int width, int whiten,
                          float* out_dev, int32_t* range_flag_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    return nv_run(packed_weights_dev, image_dev, layout, batch, height, width, 3, whiten, out_dev, range_flag_dev, workspace_dev, workspace_bytes,
                  (hipStream_t)stream);
}

int gtsfm_netvlad_stage(const float* packed_weights_dev, const void* image_dev, int layout, int batch, int height, int width, int stage, float* out_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream) {
    GTSFM_CHECK_ARG(stage >= 0 && stage <= 2, "netvlad_stage: stage must be 0, 1 or 2 (got %d)", stage);
    return nv_run(packed_weights_dev, image_dev, layout, batch, height, width, stage, 0, out_dev, nullptr, workspace_dev, workspace_bytes,
                  (hipStream_t)stream);
}

size_t gtsfm_retrieval_workspace_bytes(int n, int d, int with_sim_out) {
    if (n < 1 || d < 1) return 0;
    return rt_ws(n, d, with_sim_out).total;
}

int gtsfm_retrieval_topk(const float* desc_dev, int n, int d, int k, float min_score, int blocksize, int32_t* idx_out_dev, float* score_out_dev,
                         float* sim_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GTSFM_CHECK_ARG(n >= 1 && d >= 1 && k >= 0, "retrieval_topk: need n >= 1, d >= 1, k >= 0 (got %d, %d, %d)", n, d, k);
    GTSFM_CHECK_ARG(desc_dev && workspace_dev, "retrieval_topk: null pointer");
    GTSFM_CHECK_ARG(blocksize >= 1, "retrieval_topk: blocksize must be positive (got %d)", blocksize);
    const int kk = k < n ? k : n;
    GTSFM_CHECK_ARG(kk == 0 || (idx_out_dev && score_out_dev), "retrieval_topk: null output");
    GTSFM_CHECK_ARG(!sim_out_dev || n <= 65535, "retrieval_topk: the similarity output takes at most 65535 rows (got %d)", n);
    const RtWs s = rt_ws(n, d, sim_out_dev != nullptr);
    GTSFM_CHECK_ARG(workspace_bytes >= s.total, "retrieval_topk: workspace too small (%zu < %zu bytes)", workspace_bytes, s.total);
    char* base = reinterpret_cast<char*>(workspace_dev);
    const int dp = (d + 31) / 32 * 32;
    GTSFM_CHECK_ARG(gemm_uses_dma(dp, dp), "retrieval_topk: the similarity product needs the LDS-DMA GEMM (GTSFM_GEMM=mfma is not supported here)");
    const float* a = desc_dev;
    if (d % 32) {
        float* padded = reinterpret_cast<float*>(base + s.pad);
        hipLaunchKernelGGL(rt_pad_kernel, dim3(1024), dim3(256), 0, st, desc_dev, n, d, dp, padded);
        GTSFM_CHECK_LAUNCH("rt_pad_kernel");
        a = padded;
    }
    float* sim = sim_out_dev ? sim_out_dev : reinterpret_cast<float*>(base + s.sim);
    const int nstrips = ceil_div(n, RT_STRIP);
    GemmProblem* pr = reinterpret_cast<GemmProblem*>(base + s.problems);
    int* counts = reinterpret_cast<int*>(base + s.counts);
    hipLaunchKernelGGL(rt_problems_kernel, dim3(ceil_div(nstrips, 64)), dim3(64), 0, st, n, sim_out_dev ? blocksize : 1, nstrips, pr, counts);
    GTSFM_CHECK_LAUNCH("rt_problems_kernel");
    GemmParams g = {};
    g.A = a, g.lda = dp, g.M = n < RT_STRIP ? n : RT_STRIP, g.K = dp;
    g.wraw = a, g.ldw = dp, g.N = n;
    g.C = sim, g.ldc = n, g.alpha = 1.f;
    g.math = 0;
    GemmBatch bt = {pr, counts, nstrips};
    int rc = launch_gemm_dma_batched(g, bt, st);
    if (rc) return rc;
    if (sim_out_dev) {
        hipLaunchKernelGGL(rt_block_mask_kernel, dim3(ceil_div(n, 256) < 64 ? ceil_div(n, 256) : 64, n), dim3(256), 0, st, sim_out_dev, n, blocksize);
        GTSFM_CHECK_LAUNCH("rt_block_mask_kernel");
    }
    if (kk > 0) {
        hipLaunchKernelGGL(rt_topk_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, st, sim, n, kk, min_score, idx_out_dev, score_out_dev);
        GTSFM_CHECK_LAUNCH("rt_topk_kernel");
    }
    return GTSFM_OK;
}

}  // extern "C"
