// The VGG-16 convolution trunk that NetVLAD (all 13 layers) and D2-Net (the first 10) share: the channel table, the conv part of the
// packed blob, its packing, the launch of one 3x3 layer and conv1_1. Pool flags, activation buffers and the layer loop stay with each net.
#pragma once

#include "common.h"
#include "conv_kernels.h"

#define VGG_LAYERS 13
#define VGG_C1_T 16  // conv1_1 output tile: 16 x 16 pixels

static const int kVggCin[VGG_LAYERS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
static const int kVggCout[VGG_LAYERS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};

// Offsets (floats) of the first `layers` convolutions in a packed blob: conv1_1 raw [64][27] + bias, the rest packed
// (pack_conv3x3_weights) + bias, each piece rounded up to 64 floats. Returns the offset behind the last bias.
static inline size_t vgg_conv_layout(int layers, size_t* w, size_t* b) {
    size_t o = 0;
    for (int l = 0; l < layers; ++l) {
        w[l] = o, o += a64(l == 0 ? (size_t)64 * 27 : packed_conv3x3_floats(kVggCin[l], kVggCout[l]));
        b[l] = o, o += a64(kVggCout[l]);
    }
    return o;
}

// t[2 l] / t[2 l + 1]: weight [Cout][Cin][3][3] / bias of layer l, into a zeroed blob at the offsets of vgg_conv_layout.
static inline void vgg_pack_convs(const float* const* t, int layers, const size_t* w, const size_t* b, float* packed) {
    for (int l = 0; l < layers; ++l) {
        if (l == 0)
            for (int i = 0; i < 64 * 27; ++i) packed[w[0] + i] = t[0][i];
        else
            pack_conv3x3_weights(t[2 * l], kVggCin[l], kVggCout[l], packed + w[l]);
        for (int o = 0; o < kVggCout[l]; ++o) packed[b[l] + o] = t[2 * l + 1][o];
    }
}

// Layer l >= 1 on dense NHWC activations [B][H][W][Cin] -> [B][H or H/2][W or W/2][Cout].
static inline int vgg_conv_layer(int l, const float* in, float* out, const float* wpack, const float* bias, int B, int H, int W, int relu, int pool,
                                 bool dilated, hipStream_t st) {
    ConvParams p = {};
    p.in = in, p.in_stride = kVggCin[l], p.in_coff = 0;
    p.out = out, p.out_stride = kVggCout[l], p.out_coff = 0;
    p.wpack = wpack, p.bias = bias;
    p.B = B, p.H = H, p.W = W, p.Cin = kVggCin[l], p.Cout = kVggCout[l];
    p.relu = relu, p.pool = pool;
    return dilated ? launch_conv3x3_dil2(p, st) : launch_conv3x3(p, st);
}

// ------------------------------------------------------------------------------------------------------------------------------
// conv1_1 (3 -> 64) + ReLU with a net's preprocessing. One thread per output pixel, 64 output channels in registers; weights as
// [27 taps][64] in LDS (read as broadcast float4), the preprocessed 3 x 18 x 18 input patch in LDS (zero outside the image: the padding
// of conv1_1's input, which is the preprocessed image). acc = bias, then fmaf over the taps in torch's (c, ky, kx) order.
// load(b, c, y, x, H, W) returns the preprocessed value of one pixel inside the image.
// ------------------------------------------------------------------------------------------------------------------------------
template <class Load>
__global__ __launch_bounds__(256) void vgg_conv1_kernel(Load load, int H, int W, int tiles_x, int tiles_y, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float wt[27 * 64];
    __shared__ float patch[3][VGG_C1_T + 2][VGG_C1_T + 2];
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const size_t b = bid / tiles_y;
    const int x0 = tx * VGG_C1_T, y0 = ty * VGG_C1_T;
    for (int idx = tid; idx < 27 * 64; idx += 256) {
        const int tap = idx >> 6, o = idx & 63;
        wt[idx] = w1[o * 27 + tap];
    }
    for (int idx = tid; idx < 3 * (VGG_C1_T + 2) * (VGG_C1_T + 2); idx += 256) {
        const int c = idx / ((VGG_C1_T + 2) * (VGG_C1_T + 2)), r = idx % ((VGG_C1_T + 2) * (VGG_C1_T + 2));
        const int py = r / (VGG_C1_T + 2), px = r % (VGG_C1_T + 2);
        const int gy = y0 - 1 + py, gx = x0 - 1 + px;
        patch[c][py][px] = gy >= 0 && gy < H && gx >= 0 && gx < W ? load(b, c, gy, gx, H, W) : 0.f;
    }
    __syncthreads();
    const int px = tid & 15, py = tid >> 4;
    float acc[64];
#pragma unroll
    for (int o = 0; o < 64; ++o) acc[o] = b1[o];
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float v = patch[c][py + t / 3][px + t % 3];
            const f32x4* wrow = reinterpret_cast<const f32x4*>(wt + (c * 9 + t) * 64);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const f32x4 w = wrow[q];
                acc[4 * q] = fmaf(w[0], v, acc[4 * q]);
                acc[4 * q + 1] = fmaf(w[1], v, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(w[2], v, acc[4 * q + 2]);
                acc[4 * q + 3] = fmaf(w[3], v, acc[4 * q + 3]);
            }
        }
    const int y = y0 + py, x = x0 + px;
    if (y < H && x < W) {
        f32x4* dst = reinterpret_cast<f32x4*>(out + ((b * H + y) * W + x) * 64);
#pragma unroll
        for (int q = 0; q < 16; ++q)
            dst[q] = f32x4{fmaxf(acc[4 * q], 0.f), fmaxf(acc[4 * q + 1], 0.f), fmaxf(acc[4 * q + 2], 0.f), fmaxf(acc[4 * q + 3], 0.f)};
    }
}

template <class Load>
static inline void vgg_launch_conv1(const Load& load, int B, int H, int W, const float* w1, const float* b1, float* out, hipStream_t st) {
    const int tx = ceil_div(W, VGG_C1_T), ty = ceil_div(H, VGG_C1_T);
    hipLaunchKernelGGL(vgg_conv1_kernel<Load>, dim3((unsigned)B * tx * ty), dim3(256), 0, st, load, H, W, tx, ty, w1, b1, out);
}
