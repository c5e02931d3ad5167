// D2-Net detector-descriptor, single scale (thirdparty/d2net/lib/{model_test,pyramid,utils}.py,
// gtsfm/frontend/detector_descriptor/d2net.py): the device side of gtsfm_amd.frontend.detector_descriptor.D2NetDetDesc.
// See include/gtsfm_amd.h.
//
// Forward (all exact fp32, NHWC activations, 64-bit offsets):
//   1. vgg_conv1_kernel<D2Load> (vgg_trunk.h, shared with NetVLAD): conv1_1 (3 -> 64) + ReLU on the VALU. A uint8 pixel is normalised through a 3 x 256 table the host built with
//                          the reference's own expression (utils.py:23-38 in float64, rounded to float32), so the input equals the
//                          reference's bit for bit; a float image arrives normalised. Zero padding applies to the normalised image.
//   2. conv1_2 .. conv3_3: launch_conv3x3 (dense_kernels.hip), ReLU after every layer, max-pool fused after conv1_2 and conv2_2.
//   3. d2_avgpool_kernel : AvgPool2d(2, stride 1): ((a00 + a01) + a10) + a11, then / 4.
//   4. conv4_1 .. conv4_3: launch_conv3x3_dil2, ReLU after each (model_test.py:56-57 applies F.relu to the last one's output).
//   5. d2_detect_kernel  : one wave per map pixel. HardDetectionModule + HandcraftedLocalizationModule + the |step| < 0.5 mask
//                          (pyramid.py:84-87) + the valid-corner test (utils.py:111-131) in one pass, in the operation order of the header.
//                          Candidates (channel, i, j, step_i, step_j, score) go to a list through an atomic counter, in any order.
//   6. d2_rank_kernel    : the list sorted by (score descending, then channel, i, j ascending): every candidate counts those before it
//                          (keys are unique, so the ranks are a permutation) and is written to its rank. Deterministic.
//   7. d2_describe_kernel: one wave per kept keypoint (the first min(count, max_keypoints) of that order): bilinear interpolation of the
//                          512 channels (utils.py:149-164), x / max(||x||, 1e-12), coordinates (p * 2 + 0.5) twice as (x, y) = (j, i).
// Every image's values follow the same operation order whatever the batch, so a batch equals its images one at a time, bit for bit.

#include <math.h>

#include "../../include/gtsfm_amd.h"
#include "common.h"
#include "conv_kernels.h"
#include "vgg_trunk.h"

#define D2_LAYERS 10  // the trunk up to conv4_3
#define D2_C 512
#define D2_LUT 768  // 3 x 256

namespace {

const int kPool[D2_LAYERS] = {0, 1, 0, 1, 0, 0, 0, 0, 0, 0};
const int kFirstDilated = 7;  // the average pool sits in front of it

struct D2Cand {
    int32_t c, i, j;
    float si, sj, score;
};
static_assert(sizeof(D2Cand) == 24, "candidate records are six 32-bit words");

// Offsets (floats) of the packed blob: the 10 convolutions (vgg_conv_layout), table [3][256].
struct D2Layout {
    size_t w[D2_LAYERS], b[D2_LAYERS], lut, total;
};

D2Layout d2_layout() {
    D2Layout L;
    size_t o = vgg_conv_layout(D2_LAYERS, L.w, L.b);
    L.lut = o, o += D2_LUT;
    L.total = o;
    return L;
}

// Detection workspace (bytes, 256-aligned pieces): counts [B] | unsorted candidates [B][cap] | sorted candidates [B][cap].
struct D2DetWs {
    size_t counts, cand, sorted, total;
};

D2DetWs d2_det_ws(int B, int cap) {
    D2DetWs s;
    WorkspaceCarver c = {};
    s.counts = c.offset((size_t)B * 4);
    s.cand = c.offset((size_t)B * cap * sizeof(D2Cand));
    s.sorted = c.offset((size_t)B * cap * sizeof(D2Cand));
    s.total = c.used;
    return s;
}

// Forward workspace: act A | act B (each B x H x W x 64 floats: the largest activation is relu(conv1_1)) | detection workspace.
struct D2Ws {
    size_t actA, actB, det, total;
};

D2Ws d2_ws(int B, int H, int W, int cap) {
    D2Ws s;
    WorkspaceCarver c = {};
    s.actA = c.offset((size_t)B * H * W * 64 * 4);
    s.actB = c.offset((size_t)B * H * W * 64 * 4);
    s.det = c.offset(d2_det_ws(B, cap).total);
    s.total = c.used;
    return s;
}

// conv1_1's pixel fetch (vgg_conv1_kernel): the normalised value. layout 0: float [B][3][H][W], normalised already; 1: uint8 [B][H][W][3]
// and 2: uint8 [B][H][W] (gray = three equal channels) through the table.
struct D2Load {
    const void* img;
    int layout;
    const float* lut;
    __device__ float operator()(size_t b, int c, int gy, int gx, int H, int W) const {
        if (layout == 0) return reinterpret_cast<const float*>(img)[((b * 3 + c) * H + gy) * (size_t)W + gx];
        if (layout == 1) return lut[c * 256 + reinterpret_cast<const uint8_t*>(img)[((b * H + gy) * W + gx) * 3 + c]];
        return lut[c * 256 + reinterpret_cast<const uint8_t*>(img)[(b * H + gy) * W + gx]];
    }
};

// AvgPool2d(2, stride 1) on [B][h][w][C] -> [B][h - 1][w - 1][C], one thread per four channels of an output pixel.
__global__ __launch_bounds__(256) void d2_avgpool_kernel(const float* __restrict__ in, int h, int w, int c4, size_t total, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int q = (int)(idx % c4);
    size_t r = idx / c4;
    const int x = (int)(r % (w - 1));
    r /= (w - 1);
    const int y = (int)(r % (h - 1));
    const size_t b = r / (h - 1);
    const f32x4* src = reinterpret_cast<const f32x4*>(in) + ((b * h + y) * w + x) * c4 + q;
    const f32x4 a00 = src[0], a01 = src[c4], a10 = src[(size_t)w * c4], a11 = src[(size_t)w * c4 + c4];
    f32x4 s;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = (((a00[e] + a01[e]) + a10[e]) + a11[e]) / 4.0f;
    reinterpret_cast<f32x4*>(out)[idx] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Detection head on a dense map [B][h][w][512]: one wave per pixel, a lane holds channels 4 lane .. 4 lane + 3 and 256 + 4 lane .. + 3.
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void d2_test_channel(const float* __restrict__ mapb, int h, int w, int i, int j, int c, float x, int cap,
                                                int* __restrict__ count, D2Cand* __restrict__ cand) {
    // the eight neighbours of channel c: zero outside the map for the derivative filters (their padding), skipped for the local maximum
    // (max_pool2d pads with -inf)
    float n[3][3];
    bool local_max = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int y = i + dy, xx = j + dx;
            float v = 0.f;
            if (y >= 0 && y < h && xx >= 0 && xx < w) {
                v = mapb[((size_t)y * w + xx) * D2_C + c];
                if (!(x >= v)) local_max = false;
            }
            n[dy + 1][dx + 1] = v;
        }
    if (!local_max) return;
    const float dii = (n[0][1] - 2.0f * x) + n[2][1];
    const float djj = (n[1][0] - 2.0f * x) + n[1][2];
    const float dij = 0.25f * (((n[0][0] - n[0][2]) - n[2][0]) + n[2][2]);
    const float det = dii * djj - dij * dij;
    const float tr = dii + djj;
    if (!(det > 0.f && tr * tr / det <= 7.2f)) return;  // (edge_threshold + 1)^2 / edge_threshold = 7.2
    const float di = 0.5f * n[2][1] - 0.5f * n[0][1];
    const float dj = 0.5f * n[1][2] - 0.5f * n[1][0];
    const float h00 = djj / det, h01 = -dij / det, h11 = dii / det;
    const float si = -(h00 * di + h01 * dj);
    const float sj = -(h01 * di + h11 * dj);
    if (!(fabsf(si) < 0.5f && fabsf(sj) < 0.5f)) return;
    const float pi = (float)i + si, pj = (float)j + sj;
    if (!(floorf(pi) >= 0.f && floorf(pj) >= 0.f && ceilf(pi) < (float)h && ceilf(pj) < (float)w)) return;
    const int slot = atomicAdd(count, 1);
    if (slot < cap) cand[slot] = D2Cand{c, i, j, si, sj, x};
}

__global__ __launch_bounds__(256) void d2_detect_kernel(const float* __restrict__ map, int h, int w, size_t pixels_total, int cap, int* __restrict__ counts,
                                                      D2Cand* __restrict__ cand) {
    const size_t pix = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= pixels_total) return;
    const int lane = threadIdx.x & 63;
    const size_t hw = (size_t)h * w;
    const size_t b = pix / hw;
    const int r = (int)(pix % hw);
    const int i = r / w, j = r % w;
    const float* mapb = map + b * hw * D2_C;
    const f32x4* row = reinterpret_cast<const f32x4*>(mapb + (size_t)r * D2_C);
    const f32x4 v0 = row[lane], v1 = row[lane + 64];
    const float m = wave_max(fmaxf(fmaxf(fmaxf(v0[0], v0[1]), fmaxf(v0[2], v0[3])), fmaxf(fmaxf(v1[0], v1[1]), fmaxf(v1[2], v1[3]))));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (v0[e] == m) d2_test_channel(mapb, h, w, i, j, 4 * lane + e, v0[e], cap, counts + b, cand + b * cap);
        if (v1[e] == m) d2_test_channel(mapb, h, w, i, j, 256 + 4 * lane + e, v1[e], cap, counts + b, cand + b * cap);
    }
}

__device__ __forceinline__ bool d2_before(float s1, unsigned long long k1, float s2, unsigned long long k2) { return s1 > s2 || (s1 == s2 && k1 < k2); }

// sorted[rank] = cand[t], rank = the number of candidates before t in (score descending; channel, i, j ascending). grid (ceil(cap / 256), B).
__global__ __launch_bounds__(256) void d2_rank_kernel(const D2Cand* __restrict__ cand, const int* __restrict__ counts, int cap, int h, int w,
                                                    D2Cand* __restrict__ sorted) {
    __shared__ float ss[256];
    __shared__ unsigned long long sk[256];
    const size_t b = blockIdx.y;
    const int n = min(counts[b], cap);
    if ((int)(blockIdx.x * 256) >= n) return;  // the whole workgroup
    const D2Cand* cb = cand + b * cap;
    const int t = blockIdx.x * 256 + threadIdx.x;
    D2Cand mine = {};
    unsigned long long mykey = 0;
    if (t < n) {
        mine = cb[t];
        mykey = ((unsigned long long)mine.c * h + mine.i) * w + mine.j;
    }
    int rank = 0;
    for (int base = 0; base < n; base += 256) {
        const int o = base + threadIdx.x;
        __syncthreads();
        if (o < n) {
            const D2Cand other = cb[o];
            ss[threadIdx.x] = other.score;
            sk[threadIdx.x] = ((unsigned long long)other.c * h + other.i) * w + other.j;
        }
        __syncthreads();
        const int m = min(256, n - base);
        for (int q = 0; q < m; ++q) rank += d2_before(ss[q], sk[q], mine.score, mykey) ? 1 : 0;
    }
    if (t < n) sorted[b * cap + rank] = mine;
}

// One wave per kept keypoint k < min(count, cap, K). grid (ceil(K / 4), B). Outputs have K rows per image.
__global__ __launch_bounds__(256) void d2_describe_kernel(const float* __restrict__ map, int h, int w, const D2Cand* __restrict__ sorted,
                                                        const int* __restrict__ counts, int cap, int K, float* __restrict__ kp, float* __restrict__ scores,
                                                        float* __restrict__ desc) {
    const size_t b = blockIdx.y;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= min(min(counts[b], cap), K)) return;
    const int lane = threadIdx.x & 63;
    const D2Cand cd = sorted[b * cap + k];
    const float pi = (float)cd.i + cd.si, pj = (float)cd.j + cd.sj;
    const float fi = floorf(pi), fj = floorf(pj);
    const int i0 = (int)fi, j0 = (int)fj, i1 = (int)ceilf(pi), j1 = (int)ceilf(pj);
    const float ddi = pi - fi, ddj = pj - fj;
    const float wtl = (1.0f - ddi) * (1.0f - ddj), wtr = (1.0f - ddi) * ddj, wbl = ddi * (1.0f - ddj), wbr = ddi * ddj;
    const float* mapb = map + b * (size_t)h * w * D2_C;
    const f32x4* tl = reinterpret_cast<const f32x4*>(mapb + ((size_t)i0 * w + j0) * D2_C);
    const f32x4* tr = reinterpret_cast<const f32x4*>(mapb + ((size_t)i0 * w + j1) * D2_C);
    const f32x4* bl = reinterpret_cast<const f32x4*>(mapb + ((size_t)i1 * w + j0) * D2_C);
    const f32x4* br = reinterpret_cast<const f32x4*>(mapb + ((size_t)i1 * w + j1) * D2_C);
    f32x4 d[2];
    float ss = 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const f32x4 a = tl[lane + 64 * g], bb = tr[lane + 64 * g], c = bl[lane + 64 * g], e4 = br[lane + 64 * g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            d[g][e] = ((wtl * a[e] + wtr * bb[e]) + wbl * c[e]) + wbr * e4[e];
            ss = fmaf(d[g][e], d[g][e], ss);
        }
    }
    const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    f32x4* out = reinterpret_cast<f32x4*>(desc + (b * K + k) * D2_C);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = d[g][e] / nrm;
        out[lane + 64 * g] = o;
    }
    if (lane == 0) {
        kp[(b * K + k) * 2] = (pj * 2.0f + 0.5f) * 2.0f + 0.5f;
        kp[(b * K + k) * 2 + 1] = (pi * 2.0f + 0.5f) * 2.0f + 0.5f;
        scores[b * K + k] = cd.score;
    }
}

// The head on a map: candidates, their sorted list (into sorted_out), and for K > 0 the first min(count, K) keypoints.
int d2_head(const float* map, int B, int h, int w, int K, int cap, int32_t* counts_out, D2Cand* sorted_out, float* kp, float* scores, float* desc,
            char* ws, hipStream_t st) {
    const D2DetWs s = d2_det_ws(B, cap);
    int* counts = reinterpret_cast<int*>(ws + s.counts);
    D2Cand* cand = reinterpret_cast<D2Cand*>(ws + s.cand);
    D2Cand* sorted = sorted_out ? sorted_out : reinterpret_cast<D2Cand*>(ws + s.sorted);
    if (hipMemsetAsync(counts, 0, (size_t)B * 4, st) != hipSuccess) {
        gtsfm_set_error("d2net: hipMemsetAsync failed");
        return GTSFM_ERR_HIP;
    }
    const size_t pixels = (size_t)B * h * w;
    hipLaunchKernelGGL(d2_detect_kernel, dim3((unsigned)((pixels + 3) / 4)), dim3(256), 0, st, map, h, w, pixels, cap, counts, cand);
    GTSFM_CHECK_LAUNCH("d2_detect_kernel");
    hipLaunchKernelGGL(d2_rank_kernel, dim3(ceil_div(cap, 256), B), dim3(256), 0, st, cand, counts, cap, h, w, sorted);
    GTSFM_CHECK_LAUNCH("d2_rank_kernel");
    if (K > 0) {
        hipLaunchKernelGGL(d2_describe_kernel, dim3(ceil_div(K, 4), B), dim3(256), 0, st, map, h, w, sorted, counts, cap, K, kp, scores, desc);
        GTSFM_CHECK_LAUNCH("d2_describe_kernel");
    }
    if (hipMemcpyAsync(counts_out, counts, (size_t)B * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        gtsfm_set_error("d2net: hipMemcpyAsync failed");
        return GTSFM_ERR_HIP;
    }
    return GTSFM_OK;
}

// Why a shape is refused (nullptr: it is fine). The dense map is (H / 4 - 1) x (W / 4 - 1) (floor at both pools): below 8 pixels the average
// pool has nothing to produce. The largest launch grid is conv1_2's: batch x 8 x 16 pixel tiles of the full image, computed in int.
const char* d2_shape_error(int B, int H, int W, int cap) {
    if (B < 1 || cap < 1) return "need batch >= 1 and a candidate capacity >= 1";
    if (H < 8 || W < 8) return "need images of at least 8 x 8 pixels";
    if ((size_t)B * cap > ((size_t)1 << 28)) return "batch x candidate capacity exceeds 2^28 records";
    if ((size_t)B * ceil_div(H, 8) * ceil_div(W, 16) >= ((size_t)1 << 31)) return "batch x image tiles exceeds the launch grid (2^31 workgroups)";
    return nullptr;
}

int d2_copy_out(void* out, const float* src, size_t floats, hipStream_t st) {
    if (hipMemcpyAsync(out, src, floats * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        gtsfm_set_error("d2net: hipMemcpyAsync of a stage output failed");
        return GTSFM_ERR_HIP;
    }
    return GTSFM_OK;
}

int d2_run(const float* wts, const void* image, int layout, int B, int H, int W, int stage, int K, int cap, void* out, int32_t* counts_out, float* kp,
           float* scores, float* desc, void* ws, size_t ws_bytes, hipStream_t st) {
    GTSFM_CHECK_ARG(wts && image && ws, "d2net: null pointer");
    GTSFM_CHECK_ARG(layout >= 0 && layout <= 2, "d2net: layout must be 0 (float [B][3][H][W]), 1 (uint8 [B][H][W][3]) or 2 (uint8 [B][H][W]) (got %d)", layout);
    const char* why = d2_shape_error(B, H, W, cap);
    GTSFM_CHECK_ARG(!why, "d2net: %s (got %d x %d x %d, capacity %d)", why, B, H, W, cap);
    const D2Ws s = d2_ws(B, H, W, cap);
    GTSFM_CHECK_ARG(ws_bytes >= s.total, "d2net: workspace too small (%zu < %zu bytes)", ws_bytes, s.total);
    const D2Layout L = d2_layout();
    char* base = reinterpret_cast<char*>(ws);
    float* act[2] = {reinterpret_cast<float*>(base + s.actA), reinterpret_cast<float*>(base + s.actB)};
    vgg_launch_conv1(D2Load{image, layout, wts + L.lut}, B, H, W, wts + L.w[0], wts + L.b[0], act[0], st);
    GTSFM_CHECK_LAUNCH("vgg_conv1_kernel<D2Load>");
    if (stage == 0) return d2_copy_out(out, act[0], (size_t)B * H * W * 64, st);
    int h = H, w = W, cur = 0;
    for (int l = 1; l < D2_LAYERS; ++l) {
        if (l == kFirstDilated) {
            if (stage == 1) return d2_copy_out(out, act[cur], (size_t)B * h * w * 256, st);
            const size_t total = (size_t)B * (h - 1) * (w - 1) * 64;
            hipLaunchKernelGGL(d2_avgpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, act[cur], h, w, 64, total, act[cur ^ 1]);
            GTSFM_CHECK_LAUNCH("d2_avgpool_kernel");
            cur ^= 1, --h, --w;
        }
        const int rc = vgg_conv_layer(l, act[cur], act[cur ^ 1], wts + L.w[l], wts + L.b[l], B, h, w, 1, kPool[l], l >= kFirstDilated, st);
        if (rc) return rc;
        cur ^= 1;
        if (kPool[l]) h >>= 1, w >>= 1;
    }
    const float* map = act[cur];  // [B][h][w][512]
    if (stage == 2) return d2_copy_out(out, map, (size_t)B * h * w * D2_C, st);
    GTSFM_CHECK_ARG(counts_out, "d2net: null counts");
    if (stage == 3) return d2_head(map, B, h, w, 0, cap, counts_out, reinterpret_cast<D2Cand*>(out), nullptr, nullptr, nullptr, base + s.det, st);
    return d2_head(map, B, h, w, K, cap, counts_out, nullptr, kp, scores, desc, base + s.det, st);
}

}  // namespace

extern "C" {

int gtsfm_conv3x3_dil2_f32(const float* in_dev, int in_stride, int in_coff, float* out_dev, int out_stride, int out_coff, const float* packed_w_dev,
                           const float* bias_dev, int batch, int h, int w, int cin, int cout, int relu, void* stream) {
    GTSFM_CHECK_ARG(in_dev && out_dev && packed_w_dev && bias_dev, "conv3x3_dil2: null pointer");
    GTSFM_CHECK_ARG(batch >= 0 && h >= 0 && w >= 0 && cout > 0, "conv3x3_dil2: bad shape");
    if (batch == 0 || h == 0 || w == 0) return GTSFM_OK;
    ConvParams p = {};
    p.in = in_dev, p.in_stride = in_stride, p.in_coff = in_coff;
    p.out = out_dev, p.out_stride = out_stride, p.out_coff = out_coff;
    p.wpack = packed_w_dev, p.bias = bias_dev;
    p.B = batch, p.H = h, p.W = w, p.Cin = cin, p.Cout = cout, p.relu = relu;
    return launch_conv3x3_dil2(p, (hipStream_t)stream);
}

size_t gtsfm_d2net_packed_weight_floats(void) { return d2_layout().total; }

int gtsfm_d2net_pack_weights(const float* const* t, float* packed) {
    GTSFM_CHECK_ARG(t && packed, "d2net_pack_weights: null pointer");
    for (int i = 0; i < 2 * D2_LAYERS + 1; ++i) GTSFM_CHECK_ARG(t[i], "d2net_pack_weights: tensor %d is null", i);
    const D2Layout L = d2_layout();
    for (size_t i = 0; i < L.total; ++i) packed[i] = 0.f;
    vgg_pack_convs(t, D2_LAYERS, L.w, L.b, packed);
    for (int i = 0; i < D2_LUT; ++i) packed[L.lut + i] = t[2 * D2_LAYERS][i];
    return GTSFM_OK;
}

size_t gtsfm_d2net_workspace_bytes(int batch, int height, int width, int cand_capacity) {
    const char* why = d2_shape_error(batch, height, width, cand_capacity);
    if (why) {
        gtsfm_set_error("d2net: %s (got %d x %d x %d, capacity %d)", why, batch, height, width, cand_capacity);
        return 0;
    }
    return d2_ws(batch, height, width, cand_capacity).total;
}

int gtsfm_d2net_forward(const float* packed_weights_dev, const void* image_dev, int layout, int batch, int height, int width, int max_keypoints,
                        int cand_capacity, int32_t* counts_dev, float* keypoints_dev, float* scores_dev, float* desc_dev, void* workspace_dev,
                        size_t workspace_bytes, void* stream) {
    GTSFM_CHECK_ARG(max_keypoints >= 1 && keypoints_dev && scores_dev && desc_dev && counts_dev, "d2net_forward: need max_keypoints >= 1 and the four outputs");
    return d2_run(packed_weights_dev, image_dev, layout, batch, height, width, 4, max_keypoints, cand_capacity, nullptr, counts_dev, keypoints_dev, scores_dev,
                  desc_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int gtsfm_d2net_stage(const float* packed_weights_dev, const void* image_dev, int layout, int batch, int height, int width, int stage, int cand_capacity,
                      void* out_dev, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    GTSFM_CHECK_ARG(stage >= 0 && stage <= 3, "d2net_stage: stage must be 0, 1, 2 or 3 (got %d)", stage);
    GTSFM_CHECK_ARG(out_dev, "d2net_stage: null output");
    return d2_run(packed_weights_dev, image_dev, layout, batch, height, width, stage, 0, cand_capacity, out_dev, counts_dev, nullptr, nullptr, nullptr,
                  workspace_dev, workspace_bytes, (hipStream_t)stream);
}

size_t gtsfm_d2net_detect_workspace_bytes(int batch, int cand_capacity) {
    if (batch < 1 || cand_capacity < 1 || (size_t)batch * cand_capacity > (size_t)1 << 28) return 0;
    return d2_det_ws(batch, cand_capacity).total;
}

int gtsfm_d2net_detect(const float* map_dev, int batch, int map_height, int map_width, int max_keypoints, int cand_capacity, int32_t* counts_dev,
                       void* candidates_dev, float* keypoints_dev, float* scores_dev, float* desc_dev, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
    GTSFM_CHECK_ARG(map_dev && counts_dev && workspace_dev, "d2net_detect: null pointer");
    GTSFM_CHECK_ARG(batch >= 1 && map_height >= 1 && map_width >= 1 && cand_capacity >= 1 && (size_t)batch * cand_capacity <= (size_t)1 << 28 &&
                        (size_t)batch * map_height * map_width < ((size_t)1 << 33),
                    "d2net_detect: need batch, map size and capacity >= 1 (got %d x %d x %d, %d)", batch, map_height, map_width, cand_capacity);
    GTSFM_CHECK_ARG(max_keypoints >= 0 && (max_keypoints == 0 || (keypoints_dev && scores_dev && desc_dev)), "d2net_detect: max_keypoints > 0 needs the three outputs");
    const size_t need = d2_det_ws(batch, cand_capacity).total;
    GTSFM_CHECK_ARG(workspace_bytes >= need, "d2net_detect: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    return d2_head(map_dev, batch, map_height, map_width, max_keypoints, cand_capacity, counts_dev, reinterpret_cast<D2Cand*>(candidates_dev), keypoints_dev,
                   scores_dev, desc_dev, reinterpret_cast<char*>(workspace_dev), (hipStream_t)stream);
}

}  // extern "C"
