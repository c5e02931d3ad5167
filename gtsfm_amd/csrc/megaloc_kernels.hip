// MegaLoc global descriptors (thirdparty/megaloc/megaloc.py: DINOv2 ViT-B/14 backbone + SALAD aggregation + linear + L2 norm): the
// device side of gtsfm_amd.frontend.global_descriptor.MegaLocGlobalDescriptor. See include/gtsfm_amd.h.
//
// Forward (all exact fp32), hidden size 768, 12 heads of 64, patch 14, T = 1 + n tokens per image (n = (H / 14) (W / 14)):
//   1. ml_patch_embed_kernel: the 14 x 14 stride-14 convolution as a [n][588] x [588][768] product on the fp32 MFMA, patches read
//                             straight from the image (float, or uint8 with / 255 and the mean / std normalisation applied while the
//                             tile is staged: megaloc_global_descriptor.py:52-57), + bias + position table; the cls row is cls + pos[0].
//   2. depth x block        : ml_layernorm_kernel -> Wqkv (launch_gemm) -> launch_attention, scale 1/8, three launches of four heads
//                             (the launcher takes at most four) -> output projection with LayerScale folded into its weights and the
//                             residual in the GEMM epilogue -> ml_layernorm_kernel -> fc1 -> ml_gelu_kernel (exact erf) -> fc2 with
//                             LayerScale folded and the residual in the epilogue.
//   3. final ml_layernorm_kernel: x_norm_clstoken (row 0 of an image) and x_norm_patchtokens (rows 1 .. n), token-major.
//   4. SALAD (megaloc.py:188-283): token MLP on the cls rows; the first layers of cluster_features and score as ONE 768 -> 1024
//      product over the tokens, then 512 -> 256 and 512 -> 64; ml_salad_kernel, one workgroup per image: the 65 x n score matrix
//      with the dustbin row in LDS through three log-space Sinkhorn iterations, exp, the aggregation sum_n f[l][n] p[m][n], the
//      per-cluster and global normalisations (megaloc.py:144-186, 270-283).
//   5. sk_linear_kernel / sk_finish_kernel (splitk_linear.h): 16640 -> feat_dim + bias, L2 norm (megaloc.py:85-93, 100-102).
// A batch is cut into chunks (at most 64 images, fewer when an image has many tokens) that run one after another through one
// workspace, so no activation buffer reaches 2^31 bytes; every image's values follow one operation order whatever the batch.

#include <math.h>
#include <string.h>

#include "../../include/gtsfm_amd.h"
#include "attention_kernels.h"
#include "common.h"
#include "gemm_kernels.h"
#include "splitk_linear.h"

#define ML_D 768
#define ML_HEADS 12
#define ML_PATCH 14
#define ML_PK (3 * ML_PATCH * ML_PATCH)  // 588
#define ML_FF 3072
#define ML_MLP 512
#define ML_CL 64    // clusters
#define ML_CD 256   // channels per cluster
#define ML_TOK 256  // token part
#define ML_SALAD (ML_TOK + ML_CL * ML_CD)  // 16640
#define ML_LIN_F4 5                         // 16640 = 13 slices of 256 * 5
#define ML_LIN_SLICES (ML_SALAD / (256 * ML_LIN_F4))
#define ML_LIN_IMG 8                        // images per workgroup of the output projection (160 registers of inputs)
#define ML_PE_KC 98   // patch embedding: depth of one staged chunk (7 rows of 14 pixels of one channel)
#define ML_PE_LD 99   // its LDS row stride (odd: conflict-free)
#define ML_MAX_CHUNK 64
#define ML_LDS_LIMIT (160 * 1024)
#define ML_BLOCK_TENSORS 14

namespace {

struct MlBlock {
    size_t n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b;
};

// Offsets (floats) of the packed blob; every piece starts at a multiple of 64 floats and is zero-padded to one.
struct MlLayout {
    size_t pw, pb, cls;
    size_t blocks;  // first block; blocks are block_floats apart
    size_t block_floats;
    MlBlock rel;    // offsets inside a block
    size_t normw, normb, t0w, t0b, t1w, t1b, cs0w, cs0b, c1w, c1b, s1w, s1b, dust, linw, linb, total;
};

MlLayout ml_layout(int depth, int feat) {
    MlLayout L;
    size_t o = 0;
    L.pw = o, o += a64((size_t)ML_D * ML_PK);
    L.pb = o, o += ML_D;
    L.cls = o, o += ML_D;
    L.blocks = o;
    size_t r = 0;
    L.rel.n1w = r, r += ML_D;
    L.rel.n1b = r, r += ML_D;
    L.rel.qkvw = r, r += (size_t)3 * ML_D * ML_D;
    L.rel.qkvb = r, r += 3 * ML_D;
    L.rel.projw = r, r += (size_t)ML_D * ML_D;
    L.rel.projb = r, r += ML_D;
    L.rel.n2w = r, r += ML_D;
    L.rel.n2b = r, r += ML_D;
    L.rel.fc1w = r, r += (size_t)ML_FF * ML_D;
    L.rel.fc1b = r, r += ML_FF;
    L.rel.fc2w = r, r += (size_t)ML_D * ML_FF;
    L.rel.fc2b = r, r += ML_D;
    L.block_floats = r;
    o += (size_t)depth * r;
    L.normw = o, o += ML_D;
    L.normb = o, o += ML_D;
    L.t0w = o, o += (size_t)ML_MLP * ML_D;
    L.t0b = o, o += ML_MLP;
    L.t1w = o, o += (size_t)ML_TOK * ML_MLP;
    L.t1b = o, o += ML_TOK;
    L.cs0w = o, o += (size_t)2 * ML_MLP * ML_D;
    L.cs0b = o, o += 2 * ML_MLP;
    L.c1w = o, o += (size_t)ML_CD * ML_MLP;
    L.c1b = o, o += ML_CD;
    L.s1w = o, o += (size_t)ML_CL * ML_MLP;
    L.s1b = o, o += ML_CL;
    L.dust = o, o += 64;
    L.linw = o, o += (size_t)feat * ML_SALAD;
    L.linb = o, o += a64(feat);
    L.total = o;
    return L;
}

bool ml_shape_ok(int depth, int feat) { return depth >= 1 && depth <= 64 && feat >= 64 && feat % 64 == 0; }
bool ml_image_ok(int B, int H, int W) {
    return B >= 1 && H >= ML_PATCH && W >= ML_PATCH && H % ML_PATCH == 0 && W % ML_PATCH == 0 && (long long)(H / ML_PATCH) * (W / ML_PATCH) > ML_CL &&
           (long long)(H / ML_PATCH) * (W / ML_PATCH) < 160000;
}

// Images per chunk: at most 64, and rows * 3072 floats stays below 2^31 bytes.
int ml_chunk(int B, int T) {
    int c = (int)(((1LL << 29) - 1) / ((long long)T * ML_FF));
    if (c > ML_MAX_CHUNK) c = ML_MAX_CHUNK;
    if (c < 1) c = 1;
    return c < B ? c : B;
}

size_t ml_salad_lds_bytes(int n, bool matrix_in_lds) { return (512 + a64(n) + (matrix_in_lds ? (size_t)(ML_CL + 1) * n : 0)) * sizeof(float); }

// Workspace (bytes, 256-aligned pieces) for one chunk of Bc images, R = Bc * T rows:
// flag | x [R][768] | y [R][768] | wide [R][3072] (qkv, the MLP's hidden layer, SALAD's layers) | attention | token MLP | salad vector |
// output-projection slices | attention problems + count | score matrices (only when 65 x n does not fit in LDS)
struct MlWs {
    size_t x, y, wide, attn, attn_floats, th, tk, vec, part, problems, counts, mglob, total;
};

MlWs ml_ws(int B, int H, int W, int feat) {
    MlWs s;
    const int n = (H / ML_PATCH) * (W / ML_PATCH), T = n + 1, Bc = ml_chunk(B, T);
    const size_t R = (size_t)Bc * T;
    WorkspaceCarver c = {};
    c.offset(4);  // the range flag of a call that passes none
    s.x = c.offset(R * ML_D * 4);
    s.y = c.offset(R * ML_D * 4);
    s.wide = c.offset(R * ML_FF * 4);
    s.attn_floats = attention_workspace_floats(Bc, 4, T, T, R, ATTN_MATH_F32);
    s.attn = c.offset(s.attn_floats * 4);
    s.th = c.offset((size_t)Bc * ML_MLP * 4);
    s.tk = c.offset((size_t)Bc * ML_TOK * 4);
    s.vec = c.offset((size_t)Bc * ML_SALAD * 4);
    s.part = c.offset((size_t)ML_LIN_SLICES * Bc * feat * 4);
    s.problems = c.offset((size_t)Bc * sizeof(AttnProblem));
    s.counts = c.offset(256);
    s.mglob = c.offset(ml_salad_lds_bytes(n, true) <= ML_LDS_LIMIT ? 0 : (size_t)Bc * (ML_CL + 1) * n * 4);
    s.total = c.used;
    return s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Patch embedding. Workgroup = 64 patches of one image x 64 output channels, 4 waves of one 32 x 32 MFMA accumulator each; the depth
// k = c * 196 + ky * 14 + kx runs in six chunks of 98 (half a channel) staged in LDS: patches [64][98] gathered from the image,
// weights [64][98] from the row-major conv weight. out row b * T + 1 + p = (acc + bias) + pos[1 + p]; row b * T = cls + pos[0].
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ml_patch_embed_kernel(const void* __restrict__ img, int u8, int H, int W, int gw, int n, const float* __restrict__ pw,
                                                           const float* __restrict__ pb, const float* __restrict__ cls, const float* __restrict__ pos,
                                                           float* __restrict__ out, int* __restrict__ flag) {
    __shared__ float As[64 * ML_PE_LD];
    __shared__ float Ws[64 * ML_PE_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const size_t b = blockIdx.z;
    const int T = n + 1;
    const int mi = wave & 1, nj = wave >> 1;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    bool bad = false;
    for (int ch = 0; ch < 6; ++ch) {
        const int c = ch >> 1, ky0 = (ch & 1) * 7;
        __syncthreads();
        for (int idx = tid; idx < 64 * ML_PE_KC; idx += 256) {
            const int pm = idx / ML_PE_KC, kk = idx % ML_PE_KC;
            const int p = p0 + pm;
            float v = 0.f;
            if (p < n) {
                const int y = (p / gw) * ML_PATCH + ky0 + kk / ML_PATCH, x = (p % gw) * ML_PATCH + kk % ML_PATCH;
                const size_t at = ((b * 3 + c) * H + y) * (size_t)W + x;
                if (u8) {
                    v = ((float)reinterpret_cast<const uint8_t*>(img)[at] / 255.0f - mean[c]) / stdv[c];
                } else {
                    v = reinterpret_cast<const float*>(img)[at];
                    bad |= !isfinite(v);
                }
            }
            As[pm * ML_PE_LD + kk] = v;
            Ws[pm * ML_PE_LD + kk] = pw[(size_t)(n0 + pm) * ML_PK + c * (ML_PATCH * ML_PATCH) + ky0 * ML_PATCH + kk];
        }
        __syncthreads();
        const float* ap = As + (mi * 32 + (lane & 31)) * ML_PE_LD + (lane >> 5);
        const float* wp = Ws + (nj * 32 + (lane & 31)) * ML_PE_LD + (lane >> 5);
#pragma unroll 7
        for (int kk = 0; kk < ML_PE_KC; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], wp[kk], acc, 0, 0, 0);
    }
    if (bad) atomicOr(flag, 1);
    const int col = n0 + nj * 32 + (lane & 31);
    const float bias = pb[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int p = p0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (p < n) out[(b * T + 1 + p) * ML_D + col] = (acc[r] + bias) + pos[(size_t)(1 + p) * ML_D + col];
    }
    if (blockIdx.x == 0 && tid < 64) out[b * T * ML_D + n0 + tid] = cls[n0 + tid] + pos[n0 + tid];
}

// LayerNorm over rows of 768 (one wave per row): y = (x - mean) / sqrt(var + eps) * g + b, var = mean((x - mean)^2).
__global__ __launch_bounds__(256) void ml_layernorm_kernel(const float* __restrict__ x, long long rows, const float* __restrict__ g, const float* __restrict__ bt,
                                                         float eps, float* __restrict__ y) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + row * ML_D);
    f32x4 v[3];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] = xr[lane + 64 * i];
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) / (float)ML_D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[i][e] = v[i][e] - mean;
            q = fmaf(v[i][e], v[i][e], q);
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)ML_D + eps);
    f32x4* yr = reinterpret_cast<f32x4*>(y + row * ML_D);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[lane + 64 * i], bv = reinterpret_cast<const f32x4*>(bt)[lane + 64 * i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[i][e] * rstd * gv[e] + bv[e];
        yr[lane + 64 * i] = o;
    }
}

// Exact GELU in place: x * 0.5 * (1 + erf(x / sqrt 2)) (torch.nn.GELU()).
__global__ __launch_bounds__(256) void ml_gelu_kernel(float* __restrict__ x, size_t count4) {
    f32x4* p = reinterpret_cast<f32x4*>(x);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count4; i += (size_t)gridDim.x * 256) {
        f32x4 v = p[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * 0.5f * (1.0f + erff(v[e] * 0.70710678118654752440f));
        p[i] = v;
    }
}

// Attention problems of a chunk: image b attends over its own T rows; one shared count.
__global__ void ml_problems_kernel(int B, int T, AttnProblem* __restrict__ pr, int* __restrict__ counts) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) counts[0] = T;
    if (b >= B) return;
    AttnProblem p;
    p.q_off = b * T, p.q_cnt_idx = 0, p.k_off = b * T, p.k_cnt_idx = 0;
    pr[b] = p;
}

__device__ float ml_block_sum1024(float v, float* red16) {  // 1024 threads; result in every thread
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red16[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += red16[i];
    return s;
}

// SALAD aggregation of one image (megaloc.py:144-186, 270-283). f: cluster features, row b * T + 1 + j, 256 columns; sc: scores, same
// rows, 64 columns; tok: token features [B][256]. Dynamic LDS: u[128] | reductions[384] | v[a64(n)] | (LDSM) the matrix [65][n];
// without LDSM (65 x n floats past the LDS) the matrix lives in mglob. 1024 threads.
//   M[m][j] = score (m < 64) or dust_bin (m = 64); three times u = log_a - logsumexp_j(M + v), v = log_b - logsumexp_m(M + u);
//   p = exp(((M + u) + v) - norm), rows m < 64; agg[l][m] = sum_j f[j][l] p[m][j] in the order of j; a = agg / max(||agg[:, m]||, 1e-12);
//   out = [t / max(||t||, 1e-12), a at l * 64 + m] / max(||.||, 1e-12).
template <bool LDSM>
__global__ __launch_bounds__(1024) void ml_salad_kernel(const float* __restrict__ f, int ldf, const float* __restrict__ sc, int ldsc,
                                                      const float* __restrict__ tok, const float* __restrict__ dust, int T, float norm, float la_dust,
                                                      float* __restrict__ mglob, float* __restrict__ vec) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = T - 1;
    const size_t b = blockIdx.x;
    float* u = sm;
    float* red = sm + 128;   // [16 waves][16]
    float* nm = sm + 384;    // [64]
    float* red16 = sm + 448;  // [16]
    float* v = sm + 512;
    float* M = LDSM ? v + (n + 63) / 64 * 64 : mglob + b * (size_t)(ML_CL + 1) * n;
    const float* fb = f + (b * T + 1) * (size_t)ldf;
    const float* sb = sc + (b * T + 1) * (size_t)ldsc;
    for (int idx = tid; idx < ML_CL * n; idx += 1024) M[(idx & 63) * n + (idx >> 6)] = sb[(size_t)(idx >> 6) * ldsc + (idx & 63)];
    const float db = dust[0];
    for (int j = tid; j < n; j += 1024) M[ML_CL * n + j] = db, v[j] = 0.f;
    __syncthreads();
    for (int it = 0; it < 3; ++it) {
        for (int m = wave; m <= ML_CL; m += 16) {
            const float* row = M + m * n;
            float mx = -INFINITY;
            for (int j = lane; j < n; j += 64) mx = fmaxf(mx, row[j] + v[j]);
            mx = wave_max(mx);
            float s = 0.f;
            for (int j = lane; j < n; j += 64) s += expf((row[j] + v[j]) - mx);
            s = wave_sum(s);
            if (lane == 0) u[m] = (m < ML_CL ? norm : la_dust) - (logf(s) + mx);
        }
        __syncthreads();
        for (int j = tid; j < n; j += 1024) {
            float mx = -INFINITY;
            for (int m = 0; m <= ML_CL; ++m) mx = fmaxf(mx, M[m * n + j] + u[m]);
            float s = 0.f;
            for (int m = 0; m <= ML_CL; ++m) s += expf((M[m * n + j] + u[m]) - mx);
            v[j] = norm - (logf(s) + mx);
        }
        __syncthreads();
    }
    for (int idx = tid; idx < ML_CL * n; idx += 1024) {
        const int m = idx / n, j = idx - m * n;
        M[idx] = expf(((M[idx] + u[m]) + v[j]) - norm);
    }
    __syncthreads();
    const int l = tid & 255, mg = tid >> 8;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const float* pm = M + (size_t)mg * 16 * n;
    for (int j = 0; j < n; ++j) {
        const float fv = fb[(size_t)j * ldf + l];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = fmaf(fv, pm[i * n + j], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float ss = wave_sum(acc[i] * acc[i]);
        if (lane == 0) red[wave * 16 + i] = ss;
    }
    __syncthreads();
    if (tid < ML_CL) {
        const int w0 = (tid >> 4) * 4, i = tid & 15;
        nm[tid] = fmaxf(sqrtf(((red[w0 * 16 + i] + red[(w0 + 1) * 16 + i]) + red[(w0 + 2) * 16 + i]) + red[(w0 + 3) * 16 + i]), 1e-12f);
    }
    __syncthreads();
    float g = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        acc[i] = acc[i] / nm[mg * 16 + i];
        g = fmaf(acc[i], acc[i], g);
    }
    const float tv = tid < ML_TOK ? tok[b * ML_TOK + tid] : 0.f;
    const float tn = tv / fmaxf(sqrtf(ml_block_sum1024(tv * tv, red16)), 1e-12f);
    const float gn = fmaxf(sqrtf(ml_block_sum1024(fmaf(tn, tn, g), red16)), 1e-12f);
    float* ob = vec + b * ML_SALAD;
    if (tid < ML_TOK) ob[tid] = tn / gn;
    f32x4* dst = reinterpret_cast<f32x4*>(ob + ML_TOK + l * ML_CL + mg * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = f32x4{acc[4 * q] / gn, acc[4 * q + 1] / gn, acc[4 * q + 2] / gn, acc[4 * q + 3] / gn};
}

#define ML_TRY(expr)          \
    do {                      \
        const int rc_ = (expr); \
        if (rc_) return rc_;  \
    } while (0)

int ml_gemm(const float* A, int lda, int M, int K, const float* W, const float* bias, int N, float* Cc, int ldc, const float* res, int ldres, int relu,
            hipStream_t st) {
    GemmParams g = {};
    g.A = A, g.lda = lda, g.M = M, g.K = K;
    g.wraw = W, g.ldw = K, g.bias = bias, g.N = N;
    g.C = Cc, g.ldc = ldc, g.res = res, g.ldres = ldres;
    g.alpha = 1.f, g.relu = relu, g.math = 0;
    return launch_gemm(g, st);
}

// One chunk of Bc images. stage: 0 .. 3 as gtsfm_megaloc_stage, 4 = the descriptors.
int ml_run_chunk(const float* wts, const MlLayout& L, int depth, int feat, const float* pos, const void* image, int layout, int Bc, int H, int W, int stage,
                 float* out, int* flag, char* base, const MlWs& s, hipStream_t st) {
    const int gw = W / ML_PATCH, n = (H / ML_PATCH) * gw, T = n + 1;
    const long long R = (long long)Bc * T;
    float* X = reinterpret_cast<float*>(base + s.x);
    float* Y = reinterpret_cast<float*>(base + s.y);
    float* Wd = reinterpret_cast<float*>(base + s.wide);
    auto copy_out = [&](const float* src, size_t floats) { return hipMemcpyAsync(out, src, floats * 4, hipMemcpyDeviceToDevice, st) == hipSuccess ? GTSFM_OK : GTSFM_ERR_HIP; };
    hipLaunchKernelGGL(ml_patch_embed_kernel, dim3(ceil_div(n, 64), ML_D / 64, Bc), dim3(256), 0, st, image, layout, H, W, gw, n, wts + L.pw, wts + L.pb,
                       wts + L.cls, pos, X, flag);
    GTSFM_CHECK_LAUNCH("ml_patch_embed_kernel");
    if (stage == 0) return copy_out(X, (size_t)R * ML_D);
    AttnProblem* problems = reinterpret_cast<AttnProblem*>(base + s.problems);
    int* counts = reinterpret_cast<int*>(base + s.counts);
    hipLaunchKernelGGL(ml_problems_kernel, dim3(ceil_div(Bc, 64)), dim3(64), 0, st, Bc, T, problems, counts);
    GTSFM_CHECK_LAUNCH("ml_problems_kernel");
    const unsigned ln_grid = (unsigned)((R + 3) / 4);
    const int nblocks = stage == 1 ? 1 : depth;
    for (int l = 0; l < nblocks; ++l) {
        const float* bw = wts + L.blocks + (size_t)l * L.block_floats;
        hipLaunchKernelGGL(ml_layernorm_kernel, dim3(ln_grid), dim3(256), 0, st, X, R, bw + L.rel.n1w, bw + L.rel.n1b, 1e-6f, Y);
        GTSFM_CHECK_LAUNCH("ml_layernorm_kernel");
        ML_TRY(ml_gemm(Y, ML_D, (int)R, ML_D, bw + L.rel.qkvw, bw + L.rel.qkvb, 3 * ML_D, Wd, 3 * ML_D, nullptr, 0, 0, st));
        for (int hg = 0; hg < ML_HEADS / 4; ++hg) {
            AttnParams ap = {};
            ap.q = Wd + hg * 256, ap.ldq = 3 * ML_D, ap.k = Wd + ML_D + hg * 256, ap.ldk = 3 * ML_D, ap.v = Wd + 2 * ML_D + hg * 256, ap.ldv = 3 * ML_D;
            ap.out = Y + hg * 256, ap.ldo = ML_D;
            ap.problems = problems, ap.counts = counts, ap.scale = 0.125f, ap.heads = 4;
            ap.max_k = T, ap.workspace = s.attn_floats ? reinterpret_cast<float*>(base + s.attn) : nullptr, ap.workspace_floats = s.attn_floats;
            ap.part_rows = (size_t)R, ap.math = ATTN_MATH_F32;
            ML_TRY(launch_attention(ap, Bc, T, st));
        }
        ML_TRY(ml_gemm(Y, ML_D, (int)R, ML_D, bw + L.rel.projw, bw + L.rel.projb, ML_D, X, ML_D, X, ML_D, 0, st));
        hipLaunchKernelGGL(ml_layernorm_kernel, dim3(ln_grid), dim3(256), 0, st, X, R, bw + L.rel.n2w, bw + L.rel.n2b, 1e-6f, Y);
        GTSFM_CHECK_LAUNCH("ml_layernorm_kernel");
        ML_TRY(ml_gemm(Y, ML_D, (int)R, ML_D, bw + L.rel.fc1w, bw + L.rel.fc1b, ML_FF, Wd, ML_FF, nullptr, 0, 0, st));
        const size_t c4 = (size_t)R * ML_FF / 4;
        hipLaunchKernelGGL(ml_gelu_kernel, dim3((unsigned)(c4 / 256 + 1 < 8192 ? c4 / 256 + 1 : 8192)), dim3(256), 0, st, Wd, c4);
        GTSFM_CHECK_LAUNCH("ml_gelu_kernel");
        ML_TRY(ml_gemm(Wd, ML_FF, (int)R, ML_FF, bw + L.rel.fc2w, bw + L.rel.fc2b, ML_D, X, ML_D, X, ML_D, 0, st));
    }
    if (stage == 1) return copy_out(X, (size_t)R * ML_D);
    hipLaunchKernelGGL(ml_layernorm_kernel, dim3(ln_grid), dim3(256), 0, st, X, R, wts + L.normw, wts + L.normb, 1e-6f, Y);
    GTSFM_CHECK_LAUNCH("ml_layernorm_kernel");
    if (stage == 2) return copy_out(Y, (size_t)R * ML_D);
    // SALAD. Token MLP on the cls rows (row stride T * 768); cluster_features.0 | score.0 as one product over every row (the cls rows ride
    // along unused), then the two second layers: hidden [R][1024] | f [R][256] | scores [R][64] side by side in the wide buffer.
    float* th = reinterpret_cast<float*>(base + s.th);
    float* tk = reinterpret_cast<float*>(base + s.tk);
    ML_TRY(ml_gemm(Y, T * ML_D, Bc, ML_D, wts + L.t0w, wts + L.t0b, ML_MLP, th, ML_MLP, nullptr, 0, 1, st));
    ML_TRY(ml_gemm(th, ML_MLP, Bc, ML_MLP, wts + L.t1w, wts + L.t1b, ML_TOK, tk, ML_TOK, nullptr, 0, 0, st));
    float* hid = Wd;
    float* fbuf = Wd + (size_t)R * 2 * ML_MLP;
    float* sbuf = fbuf + (size_t)R * ML_CD;
    ML_TRY(ml_gemm(Y, ML_D, (int)R, ML_D, wts + L.cs0w, wts + L.cs0b, 2 * ML_MLP, hid, 2 * ML_MLP, nullptr, 0, 1, st));
    ML_TRY(ml_gemm(hid, 2 * ML_MLP, (int)R, ML_MLP, wts + L.c1w, wts + L.c1b, ML_CD, fbuf, ML_CD, nullptr, 0, 0, st));
    ML_TRY(ml_gemm(hid + ML_MLP, 2 * ML_MLP, (int)R, ML_MLP, wts + L.s1w, wts + L.s1b, ML_CL, sbuf, ML_CL, nullptr, 0, 0, st));
    float* vec = stage == 3 ? out : reinterpret_cast<float*>(base + s.vec);
    // log_a / log_b as get_matching_probs builds them (megaloc.py:167-171): a float32 norm, the dustbin entry a float32 sum
    const float norm = (float)(-log((double)(n + ML_CL)));
    const float la_dust = norm + (float)log((double)(n - ML_CL));
    const bool in_lds = ml_salad_lds_bytes(n, true) <= ML_LDS_LIMIT;
    const size_t salad_lds = ml_salad_lds_bytes(n, in_lds);
    if (in_lds) {
        // per call: the attribute belongs to the current device, and a process may hold engines on several
        const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(ml_salad_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, ML_LDS_LIMIT);
        if (attr != hipSuccess) {
            (void)hipGetLastError();
            gtsfm_set_error("megaloc: cannot allow %zu bytes of dynamic LDS for ml_salad_kernel: %s", salad_lds, hipGetErrorString(attr));
            return GTSFM_ERR_HIP;
        }
        hipLaunchKernelGGL(ml_salad_kernel<true>, dim3(Bc), dim3(1024), salad_lds, st, fbuf, ML_CD, sbuf, ML_CL, tk, wts + L.dust, T, norm, la_dust, (float*)nullptr, vec);
    } else {
        hipLaunchKernelGGL(ml_salad_kernel<false>, dim3(Bc), dim3(1024), salad_lds, st, fbuf, ML_CD, sbuf, ML_CL, tk, wts + L.dust, T, norm, la_dust,
                           reinterpret_cast<float*>(base + s.mglob), vec);
    }
    GTSFM_CHECK_LAUNCH("ml_salad_kernel");
    if (stage == 3) return GTSFM_OK;
    float* part = reinterpret_cast<float*>(base + s.part);
    hipLaunchKernelGGL((sk_linear_kernel<ML_LIN_F4, ML_LIN_IMG>), dim3(feat / 64, ML_LIN_SLICES, ceil_div(Bc, ML_LIN_IMG)), dim3(256), 0, st, vec, wts + L.linw, ML_SALAD, feat, Bc, part);
    GTSFM_CHECK_LAUNCH("sk_linear_kernel");
    hipLaunchKernelGGL((sk_finish_kernel<ML_LIN_SLICES, 1024>), dim3(Bc), dim3(1024), 0, st, part, wts + L.linb, feat, Bc, out);
    GTSFM_CHECK_LAUNCH("sk_finish_kernel");
    return GTSFM_OK;
}

int ml_run(const float* wts, int depth, int feat, const float* pos, const void* image, int layout, int B, int H, int W, int stage, float* out, int32_t* flag_dev,
           void* ws, size_t ws_bytes, hipStream_t st) {
    GTSFM_CHECK_ARG(wts && pos && image && out && ws, "megaloc: null pointer");
    GTSFM_CHECK_ARG(ml_shape_ok(depth, feat), "megaloc: depth must be 1 .. 64 and feat_dim a positive multiple of 64 (got %d, %d)", depth, feat);
    GTSFM_CHECK_ARG(layout == 0 || layout == 1, "megaloc: layout must be 0 (float [B][3][H][W]) or 1 (uint8 [B][3][H][W]) (got %d)", layout);
    GTSFM_CHECK_ARG(ml_image_ok(B, H, W), "megaloc: need batch >= 1, height and width multiples of 14 and more than 64 patches (got %d x %d x %d)", B, H, W);
    // every argument check before the first launch: a refused call enqueues nothing
    GTSFM_CHECK_ARG(gemm_uses_dma(ML_D, ML_D), "megaloc: the products need the LDS-DMA GEMM (GTSFM_GEMM=mfma is not supported here)");
    const MlWs s = ml_ws(B, H, W, feat);
    GTSFM_CHECK_ARG(ws_bytes >= s.total, "megaloc: workspace too small (%zu < %zu bytes)", ws_bytes, s.total);
    const MlLayout L = ml_layout(depth, feat);
    char* base = reinterpret_cast<char*>(ws);
    int* flag = flag_dev ? flag_dev : reinterpret_cast<int*>(base);
    if (!flag_dev && hipMemsetAsync(flag, 0, 4, st) != hipSuccess) {
        gtsfm_set_error("megaloc: hipMemsetAsync failed");
        return GTSFM_ERR_HIP;
    }
    const int T = (H / ML_PATCH) * (W / ML_PATCH) + 1, Bc = ml_chunk(B, T);
    const size_t per_out = stage == 4 ? (size_t)feat : stage == 3 ? (size_t)ML_SALAD : (size_t)T * ML_D;
    const size_t per_in = (size_t)3 * H * W * (layout ? 1 : 4);
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int bc = B - b0 < Bc ? B - b0 : Bc;
        ML_TRY(ml_run_chunk(wts, L, depth, feat, pos, reinterpret_cast<const char*>(image) + (size_t)b0 * per_in, layout, bc, H, W, stage,
                            out + (size_t)b0 * per_out, flag, base, s, st));
    }
    return GTSFM_OK;
}

}  // namespace

extern "C" {

size_t gtsfm_megaloc_packed_weight_floats(int depth, int feat_dim) {
    if (!ml_shape_ok(depth, feat_dim)) return 0;
    return ml_layout(depth, feat_dim).total;
}

int gtsfm_megaloc_pack_weights(const float* const* t, int depth, int feat_dim, float* packed) {
    GTSFM_CHECK_ARG(t && packed, "megaloc_pack_weights: null pointer");
    GTSFM_CHECK_ARG(ml_shape_ok(depth, feat_dim), "megaloc_pack_weights: depth must be 1 .. 64 and feat_dim a positive multiple of 64 (got %d, %d)", depth, feat_dim);
    const int count = 20 + ML_BLOCK_TENSORS * depth;
    for (int i = 0; i < count; ++i) GTSFM_CHECK_ARG(t[i], "megaloc_pack_weights: tensor %d is null", i);
    const MlLayout L = ml_layout(depth, feat_dim);
    memset(packed, 0, L.total * sizeof(float));
    auto put = [&](size_t at, const float* src, size_t count_) { memcpy(packed + at, src, count_ * sizeof(float)); };
    // LayerScale folded into the rows of a projection and its bias: gamma[n] * (W[n] . x + b[n]) -> (gamma[n] W[n]) . x + gamma[n] b[n]
    auto put_scaled = [&](size_t wat, size_t bat, const float* w, const float* b, const float* gamma, int N, int K) {
        for (int n = 0; n < N; ++n) {
            for (int k = 0; k < K; ++k) packed[wat + (size_t)n * K + k] = gamma[n] * w[(size_t)n * K + k];
            packed[bat + n] = gamma[n] * b[n];
        }
    };
    int i = 0;
    put(L.pw, t[i++], (size_t)ML_D * ML_PK);
    put(L.pb, t[i++], ML_D);
    put(L.cls, t[i++], ML_D);
    for (int l = 0; l < depth; ++l) {
        const size_t o = L.blocks + (size_t)l * L.block_floats;
        const float* const* bt = t + i;
        put(o + L.rel.n1w, bt[0], ML_D);
        put(o + L.rel.n1b, bt[1], ML_D);
        put(o + L.rel.qkvw, bt[2], (size_t)3 * ML_D * ML_D);
        put(o + L.rel.qkvb, bt[3], 3 * ML_D);
        put_scaled(o + L.rel.projw, o + L.rel.projb, bt[4], bt[5], bt[6], ML_D, ML_D);
        put(o + L.rel.n2w, bt[7], ML_D);
        put(o + L.rel.n2b, bt[8], ML_D);
        put(o + L.rel.fc1w, bt[9], (size_t)ML_FF * ML_D);
        put(o + L.rel.fc1b, bt[10], ML_FF);
        put_scaled(o + L.rel.fc2w, o + L.rel.fc2b, bt[11], bt[12], bt[13], ML_D, ML_FF);
        i += ML_BLOCK_TENSORS;
    }
    put(L.normw, t[i++], ML_D);
    put(L.normb, t[i++], ML_D);
    put(L.t0w, t[i++], (size_t)ML_MLP * ML_D);
    put(L.t0b, t[i++], ML_MLP);
    put(L.t1w, t[i++], (size_t)ML_TOK * ML_MLP);
    put(L.t1b, t[i++], ML_TOK);
    put(L.cs0w, t[i++], (size_t)ML_MLP * ML_D);  // cluster_features.0
    put(L.cs0b, t[i++], ML_MLP);
    put(L.c1w, t[i++], (size_t)ML_CD * ML_MLP);
    put(L.c1b, t[i++], ML_CD);
    put(L.cs0w + (size_t)ML_MLP * ML_D, t[i++], (size_t)ML_MLP * ML_D);  // score.0, below cluster_features.0
    put(L.cs0b + ML_MLP, t[i++], ML_MLP);
    put(L.s1w, t[i++], (size_t)ML_CL * ML_MLP);
    put(L.s1b, t[i++], ML_CL);
    put(L.dust, t[i++], 1);
    put(L.linw, t[i++], (size_t)feat_dim * ML_SALAD);
    put(L.linb, t[i++], feat_dim);
    return GTSFM_OK;
}

size_t gtsfm_megaloc_workspace_bytes(int batch, int height, int width, int feat_dim) {
    if (!ml_image_ok(batch, height, width) || !ml_shape_ok(1, feat_dim)) return 0;
    return ml_ws(batch, height, width, feat_dim).total;
}

int gtsfm_megaloc_forward(const float* packed_weights_dev, int depth, int feat_dim, const float* pos_dev, const void* image_dev, int layout, int batch,
                          int height, int width, float* out_dev, int32_t* flag_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    return ml_run(packed_weights_dev, depth, feat_dim, pos_dev, image_dev, layout, batch, height, width, 4, out_dev, flag_dev, workspace_dev, workspace_bytes,
                  (hipStream_t)stream);
}

int gtsfm_megaloc_stage(const float* packed_weights_dev, int depth, int feat_dim, const float* pos_dev, const void* image_dev, int layout, int batch, int height,
                        int width, int stage, float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    GTSFM_CHECK_ARG(stage >= 0 && stage <= 3, "megaloc_stage: stage must be 0 .. 3 (got %d)", stage);
    return ml_run(packed_weights_dev, depth, feat_dim, pos_dev, image_dev, layout, batch, height, width, stage, out_dev, nullptr, workspace_dev, workspace_bytes,
                  (hipStream_t)stream);
}

}  // extern "C"
