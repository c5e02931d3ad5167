// Two-way (mutual nearest neighbour) descriptor matching with an optional ratio test: the device side of
// gtsfm_amd.frontend.matcher.twoway_matcher.TwoWayMatcher (GTSfM's brute-force TwoWayMatcher). See include/gtsfm_amd.h.
//
// One call matches a ragged batch of pairs whose descriptor rows live in one table (row offset + count per side):
//   1. tw_prep_kernel   : one wave per table row. EUCLIDEAN: squared norm (and, when the table cannot be read in place,
//                         an fp32 copy padded with zeros to a multiple of 8 columns). HAMMING: the bytes as 32-bit words.
//   2. tw_tile_kernel   : the product G = A B^T of a pair is computed ONCE and reduced in both directions. A workgroup
//                         owns 128 rows of A (32 per wave) and walks a chunk of B's columns in 64-wide sub-tiles; the
//                         N1 x N2 matrix is never stored. Per element e = (|a|^2 + |b|^2) - 2 g (or the popcount of
//                         a XOR b); each lane keeps a running top-2 per row over the columns it has seen, and each
//                         sub-tile's column top-2 over the workgroup's 128 rows is written as a partial.
//   3. tw_decide_kernel : folds the partials into a per-row and per-column top-2 (real-valued input: the two candidates'
//                         values recomputed directly as sum (a - b)^2), takes the correctly rounded sqrtf, applies the
//                         ratio test in double, the mutual check, and writes matches0 / dist0.
// Top-2 lists are ordered lexicographically by (value, index), so the result does not depend on tiling, the chunking
// of B or the batch a pair is launched in. With integer descriptors (SIFT, ORB, BRISK as OpenCV emits them) and
// max|a|^2 + max|b|^2 < 2^24 every value above is exact (-ffp-contract=off), so the distances equal the reference's.

#include <algorithm>
#include <vector>

#include "../../include/gtsfm_amd.h"
#include "common.h"

#define TW_ROWS 128           // rows of A per workgroup (4 waves x 32)
#define TW_COLS 64            // columns of B per sub-tile (2 MFMA accumulators per wave)
#define TW_NONE 0x7fffffff    // index of an empty top-2 slot

namespace {

struct TwPair {
    long long rowPart, colPart;  // first Top2 entry of this pair's row / column partials (64-bit: a batch's partials may exceed 2^31)
    int offA, nA, offB, nB;      // table rows
    int nChunks, nRowBlocks;
    int out;                     // first output row
    int pad;
};

struct TwItem {
    int pair, rowBlock, chunk, c0, c1;  // c0..c1: columns of B this workgroup covers
    int pad[3];
};

struct Top2 {
    float v1, v2;
    int i1, i2;
};

struct TwLayout {
    size_t pairs, items, rows, norms, rowPart, colPart, total;
    int nItems, rowsTotal, ld;  // ld: row stride (elements) of the operand table the tile kernel reads
    bool direct;                // EUCLIDEAN fp32 table read in place (no converted copy)
};

__device__ __forceinline__ bool lex_less(float v, int i, float w, int j) { return v < w || (v == w && i < j); }

// Insert (v, i) into a lexicographically ordered top-2; entries of the two lists must be distinct indices.
__device__ __forceinline__ void t2_insert(Top2& t, float v, int i) {
    if (lex_less(v, i, t.v1, t.i1)) {
        t.v2 = t.v1, t.i2 = t.i1, t.v1 = v, t.i1 = i;
    } else if (lex_less(v, i, t.v2, t.i2)) {
        t.v2 = v, t.i2 = i;
    }
}
__device__ __forceinline__ void t2_merge(Top2& t, const Top2& o) {
    t2_insert(t, o.v1, o.i1);
    t2_insert(t, o.v2, o.i2);
}
__device__ __forceinline__ Top2 t2_empty() { return Top2{INFINITY, INFINITY, TW_NONE, TW_NONE}; }

// Running update when the candidates arrive in increasing index order: a strict `<` is the lexicographic order.
__device__ __forceinline__ void t2_push(float& v1, int& i1, float& v2, int& i2, float v, int i) {
    const bool c1 = v < v1, c2 = v < v2;
    v2 = c1 ? v1 : (c2 ? v : v2);
    i2 = c1 ? i1 : (c2 ? i : i2);
    v1 = c1 ? v : v1;
    i1 = c1 ? i : i1;
}

__device__ __forceinline__ Top2 t2_shfl_xor(const Top2& t, int m) {
    return Top2{__shfl_xor(t.v1, m, 64), __shfl_xor(t.v2, m, 64), __shfl_xor(t.i1, m, 64), __shfl_xor(t.i2, m, 64)};
}

// ---------------------------------------------------------------------------------------------------------------
// 1. pre-pass
// ---------------------------------------------------------------------------------------------------------------

// One wave per row. EUCLIDEAN: norms[r] = sum x^2 (fp32); out (if not NULL) = the row as fp32, zero-padded to `ld`.
// HAMMING: out = the row's bytes packed little-endian into `ld` 32-bit words (zero-padded); norms[r] = 0.
__global__ __launch_bounds__(256) void tw_prep_kernel(const void* __restrict__ table, int is_u8, int hamming, int dim, int stride,
                                                      int rows, void* __restrict__ out, int ld, float* __restrict__ norms) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    if (hamming) {
        const uint8_t* src = (const uint8_t*)table + (size_t)r * stride;
        uint32_t* dst = (uint32_t*)out + (size_t)r * ld;
        for (int w = lane; w < ld; w += 64) {
            uint32_t word = 0;
            for (int b = 0; b < 4; ++b) {
                const int k = 4 * w + b;
                if (k < dim) word |= (uint32_t)src[k] << (8 * b);
            }
            dst[w] = word;
        }
        if (lane == 0) norms[r] = 0.f;
        return;
    }
    float s = 0.f;
    float* dst = out ? (float*)out + (size_t)r * ld : nullptr;
    for (int k = lane; k < (dst ? ld : dim); k += 64) {
        float x = 0.f;
        if (k < dim) x = is_u8 ? (float)((const uint8_t*)table)[(size_t)r * stride + k] : ((const float*)table)[(size_t)r * stride + k];
        s += x * x;
        if (dst) dst[k] = x;
    }
    s = wave_sum(s);
    if (lane == 0) norms[r] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// 2. fused product + bidirectional top-2
// ---------------------------------------------------------------------------------------------------------------

// Accumulator element r of a 32x32 tile lives at row (r&3) + 8*(r>>2) + 4*(lane>>5), column lane&31 (mfma_tiles.h).
__device__ __forceinline__ int tw_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// EUCLIDEAN sub-tile: g[n] = A(32 rows) . B(32 columns of half n)^T over ksteps x 8 columns, v_mfma_f32_32x32x2_f32.
// Lane l supplies row l&31 of each operand and the 4 consecutive columns 8t + 4(l>>5) .. +3 of k-step t.
__device__ __forceinline__ void tw_product_l2(const float* __restrict__ a, const float* __restrict__ b0, const float* __restrict__ b1,
                                              int ksteps, f32x16& g0, f32x16& g1) {
    for (int i = 0; i < 16; ++i) g0[i] = 0.f, g1[i] = 0.f;
    f32x4 av = *reinterpret_cast<const f32x4*>(a), bv0 = *reinterpret_cast<const f32x4*>(b0), bv1 = *reinterpret_cast<const f32x4*>(b1);
    for (int t = 0; t < ksteps; ++t) {
        const f32x4 ca = av, cb0 = bv0, cb1 = bv1;
        if (t + 1 < ksteps) {  // next k-step's operands in flight during this step's 8 MFMAs
            av = *reinterpret_cast<const f32x4*>(a + 8 * (t + 1));
            bv0 = *reinterpret_cast<const f32x4*>(b0 + 8 * (t + 1));
            bv1 = *reinterpret_cast<const f32x4*>(b1 + 8 * (t + 1));
        }
        g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca.x, cb0.x, g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca.x, cb1.x, g1, 0, 0, 0);
        g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca.y, cb0.y, g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca.y, cb1.y, g1, 0, 0, 0);
        g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca.z, cb0.z, g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca.z, cb1.z, g1, 0, 0, 0);
        g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca.w, cb0.w, g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca.w, cb1.w, g1, 0, 0, 0);
    }
}

// HAMMING sub-tile: the same accumulator layout, popcount(a XOR b) summed over `words` 32-bit words (VALU).
__device__ __forceinline__ void tw_product_hamming(const uint32_t* __restrict__ X, int ld, int words, const int* arow, int bcol0, int bcol1,
                                                   f32x16& g0, f32x16& g1) {
    int c0[16], c1[16];
    for (int i = 0; i < 16; ++i) c0[i] = 0, c1[i] = 0;
    for (int w = 0; w < words; ++w) {
        const uint32_t b0 = X[(size_t)bcol0 * ld + w], b1 = X[(size_t)bcol1 * ld + w];
        for (int i = 0; i < 16; ++i) {
            const uint32_t a = X[(size_t)arow[i] * ld + w];
            c0[i] += __popc(a ^ b0);
            c1[i] += __popc(a ^ b1);
        }
    }
    for (int i = 0; i < 16; ++i) g0[i] = (float)c0[i], g1[i] = (float)c1[i];
}

template <bool HAMMING>
__global__ __launch_bounds__(256) void tw_tile_kernel(const void* __restrict__ Xv, int ld, int ksteps, const float* __restrict__ norms,
                                                      const TwPair* __restrict__ pairs, const TwItem* __restrict__ items,
                                                      Top2* __restrict__ rowPart, Top2* __restrict__ colPart) {
    __shared__ Top2 colBuf[2][4][TW_COLS];
    const TwItem it = items[blockIdx.x];
    const TwPair P = pairs[it.pair];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
    const int r0 = it.rowBlock * TW_ROWS + wave * 32;  // this wave's first row (pair-local)
    const bool active = r0 < P.nA;                     // wave-uniform

    // Rows this lane touches: the load row l32 (clamped: the epilogue masks it) and the 16 accumulator rows.
    const int ra = min(r0 + l32, P.nA - 1);
    float na[16];
    int arow[16];
    for (int i = 0; i < 16; ++i) {
        const int row = r0 + tw_acc_row(i, lane);
        na[i] = row < P.nA ? norms[P.offA + row] : INFINITY;  // masked rows: e = inf, never enters a top-2
        arow[i] = P.offA + min(row, P.nA - 1);
    }
    float rv1[16], rv2[16];
    int ri1[16], ri2[16];
    for (int i = 0; i < 16; ++i) rv1[i] = rv2[i] = INFINITY, ri1[i] = ri2[i] = TW_NONE;

    int buf = 0;
    for (int c = it.c0; c < it.c1; c += TW_COLS, buf ^= 1) {
        if (active) {
            const int col0 = c + l32, col1 = c + 32 + l32;
            const int bc0 = P.offB + min(col0, P.nB - 1), bc1 = P.offB + min(col1, P.nB - 1);
            f32x16 g0, g1;
            if constexpr (HAMMING) {
                tw_product_hamming((const uint32_t*)Xv, ld, ksteps, arow, bc0, bc1, g0, g1);
            } else {
                const float* X = (const float*)Xv;
                tw_product_l2(X + (size_t)(P.offA + ra) * ld + 4 * half, X + (size_t)bc0 * ld + 4 * half, X + (size_t)bc1 * ld + 4 * half,
                              ksteps, g0, g1);
            }
            const float nb0 = col0 < P.nB ? norms[bc0] : INFINITY, nb1 = col1 < P.nB ? norms[bc1] : INFINITY;
            float cv1[2] = {INFINITY, INFINITY}, cv2[2] = {INFINITY, INFINITY};
            int ci1[2] = {TW_NONE, TW_NONE}, ci2[2] = {TW_NONE, TW_NONE};
            for (int i = 0; i < 16; ++i) {
                const int row = r0 + tw_acc_row(i, lane);
                float e0, e1;
                if constexpr (HAMMING) {
                    e0 = (na[i] + nb0) + g0[i];
                    e1 = (na[i] + nb1) + g1[i];
                } else {
                    e0 = (na[i] + nb0) - 2.f * g0[i];
                    e1 = (na[i] + nb1) - 2.f * g1[i];
                }
                t2_push(rv1[i], ri1[i], rv2[i], ri2[i], e0, col0);  // columns arrive in increasing order per lane
                t2_push(rv1[i], ri1[i], rv2[i], ri2[i], e1, col1);
                t2_push(cv1[0], ci1[0], cv2[0], ci2[0], e0, row);  // rows increase with i for a fixed lane
                t2_push(cv1[1], ci1[1], cv2[1], ci2[1], e1, row);
            }
            for (int n = 0; n < 2; ++n) {  // the two lane halves hold the same column, different rows
                Top2 t{cv1[n], cv2[n], ci1[n], ci2[n]};
                t2_merge(t, t2_shfl_xor(t, 32));
                if (half == 0) colBuf[buf][wave][n * 32 + l32] = t;
            }
        } else if (lane < 32) {
            colBuf[buf][wave][lane] = t2_empty();
            colBuf[buf][wave][32 + lane] = t2_empty();
        }
        __syncthreads();  // double-buffered: one barrier per sub-tile
        if (threadIdx.x < TW_COLS && c + (int)threadIdx.x < P.nB) {
            Top2 t = colBuf[buf][0][threadIdx.x];
            for (int w = 1; w < 4; ++w) t2_merge(t, colBuf[buf][w][threadIdx.x]);
            colPart[P.colPart + (size_t)it.rowBlock * P.nB + c + threadIdx.x] = t;
        }
    }
    if (!active) return;
    // Row partials: merge the 32 lanes of each half (disjoint column sets), lexicographically.
    for (int i = 0; i < 16; ++i) {
        Top2 t{rv1[i], rv2[i], ri1[i], ri2[i]};
        for (int m = 1; m < 32; m <<= 1) t2_merge(t, t2_shfl_xor(t, m));
        const int row = r0 + tw_acc_row(i, lane);
        if (l32 == 0 && row < P.nA) rowPart[P.rowPart + (size_t)it.chunk * P.nA + row] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 3. fold, ratio test, mutual check
// ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float tw_dist(float e, bool hamming) { return hamming ? e : sqrtf(fmaxf(e, 0.f)); }

// Direct sum (a - b)^2 over the padded fp32 rows (the padding is zero): the reported distance of a selected candidate.
__device__ float tw_direct_l2(const float* __restrict__ X, int ld, int len, int ra, int rb) {
    const float* a = X + (size_t)ra * ld;
    const float* b = X + (size_t)rb * ld;
    float s = 0.f;
    for (int k = 0; k < len; ++k) {
        const float d = a[k] - b[k];
        s += d * d;
    }
    return s;
}

// Folded top-2 of one row (of A: parts over chunks, stride nA) or one column (of B: parts over row blocks, stride nB).
// EUCLIDEAN (refine): both candidates' values are recomputed directly and the pair re-ordered if that changes their order.
__device__ Top2 tw_fold(const Top2* __restrict__ part, int nparts, size_t stride, const float* X, int ld, int len, bool refine,
                        int self_row, int other_off) {
    Top2 t = part[0];
    for (int s = 1; s < nparts; ++s) t2_merge(t, part[(size_t)s * stride]);
    if (refine) {
        if (t.i1 != TW_NONE) t.v1 = tw_direct_l2(X, ld, len, self_row, other_off + t.i1);
        if (t.i2 != TW_NONE) t.v2 = tw_direct_l2(X, ld, len, self_row, other_off + t.i2);
        if (t.i2 != TW_NONE && lex_less(t.v2, t.i2, t.v1, t.i1)) {
            const float v = t.v1;
            const int i = t.i1;
            t.v1 = t.v2, t.i1 = t.i2, t.v2 = v, t.i2 = i;
        }
    }
    return t;
}

__device__ __forceinline__ bool tw_ratio_ok(const Top2& t, bool hamming, int use_ratio, double ratio) {
    if (!use_ratio) return true;
    return (double)tw_dist(t.v1, hamming) <= ratio * (double)tw_dist(t.v2, hamming);
}

__global__ __launch_bounds__(256) void tw_decide_kernel(const TwPair* __restrict__ pairs, const Top2* __restrict__ rowPart,
                                                        const Top2* __restrict__ colPart, const float* __restrict__ X, int ld, int len, int hamming,
                                                        int refine, int use_ratio, double ratio, int32_t* __restrict__ matches0,
                                                        float* __restrict__ dist0) {
    const TwPair P = pairs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.nA) return;
    const Top2 r = tw_fold(rowPart + P.rowPart + i, P.nChunks, P.nA, X, ld, len, refine, P.offA + i, P.offB);
    int out = -1;
    const int j = r.i1;
    if (j != TW_NONE && tw_ratio_ok(r, hamming, use_ratio, ratio)) {
        const Top2 c = tw_fold(colPart + P.colPart + j, P.nRowBlocks, P.nB, X, ld, len, refine, P.offB + j, P.offA);
        if (c.i1 == i && tw_ratio_ok(c, hamming, use_ratio, ratio)) out = j;
    }
    matches0[P.out + i] = out;
    dist0[P.out + i] = tw_dist(r.v1, hamming);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

int tw_words(int metric, int dim) { return metric == 1 ? ceil_div(dim, 4) : ceil_div(dim, 8) * 8; }

// Column chunks per pair: enough workgroups to fill the chip several times over (results do not depend on it).
// Returns GTSFM_OK, or GTSFM_ERR_INVALID when the batch needs more workgroups than one launch can have.
int tw_plan(int npairs, const int32_t* p4, std::vector<TwPair>& pairs, std::vector<TwItem>& items, int& rowsTotal) {
    long long rowBlocks = 0;
    rowsTotal = 0;
    for (int p = 0; p < npairs; ++p) rowBlocks += ceil_div(p4[4 * p + 1], TW_ROWS);
    const long long target = 8LL * gtsfm_cu_count();
    const int split = (int)((target + rowBlocks - 1) / (rowBlocks > 0 ? rowBlocks : 1));
    long long nItems = 0;
    for (int p = 0; p < npairs; ++p) {
        const int subTiles = ceil_div(p4[4 * p + 3], TW_COLS);
        const int perChunk = ceil_div(subTiles, split < 1 ? 1 : (split > subTiles ? subTiles : split));
        nItems += (long long)ceil_div(subTiles, perChunk) * ceil_div(p4[4 * p + 1], TW_ROWS);
    }
    GTSFM_CHECK_ARG(nItems < (1LL << 31), "twoway: the batch needs %lld workgroups (at most 2^31 - 1 per call): split it", nItems);
    pairs.assign(npairs, TwPair{});
    items.clear();
    items.reserve((size_t)nItems);
    long long rowPart = 0, colPart = 0;
    int out = 0;
    for (int p = 0; p < npairs; ++p) {
        TwPair& P = pairs[p];
        P.offA = p4[4 * p], P.nA = p4[4 * p + 1], P.offB = p4[4 * p + 2], P.nB = p4[4 * p + 3];
        const int subTiles = ceil_div(P.nB, TW_COLS);
        const int perChunk = ceil_div(subTiles, split < 1 ? 1 : (split > subTiles ? subTiles : split));
        P.nChunks = ceil_div(subTiles, perChunk);
        P.nRowBlocks = ceil_div(P.nA, TW_ROWS);
        P.rowPart = rowPart, P.colPart = colPart, P.out = out;
        rowPart += (long long)P.nChunks * P.nA, colPart += (long long)P.nRowBlocks * P.nB, out += P.nA;
        for (int ch = 0; ch < P.nChunks; ++ch)
            for (int rb = 0; rb < P.nRowBlocks; ++rb)
                items.push_back(TwItem{p, rb, ch, ch * perChunk * TW_COLS, std::min((ch + 1) * perChunk * TW_COLS, subTiles * TW_COLS), {0, 0, 0}});
        rowsTotal = std::max(rowsTotal, std::max(P.offA + P.nA, P.offB + P.nB));
    }
    return GTSFM_OK;
}

// direct: an fp32 table whose rows are 16-byte aligned multiples of 8 columns is read in place (no converted copy).
bool tw_direct(int desc_is_u8, int metric, int dim, int row_stride, const void* desc_dev) {
    return metric == 2 && !desc_is_u8 && dim % 8 == 0 && row_stride % 4 == 0 && ((uintptr_t)desc_dev % 16) == 0;
}

TwLayout tw_layout(int metric, int dim, int row_stride, bool direct, int npairs, const std::vector<TwItem>& items,
                   const std::vector<TwPair>& pairs, int rowsTotal) {
    TwLayout L{};
    L.nItems = (int)items.size(), L.rowsTotal = rowsTotal;
    L.direct = direct;
    L.ld = L.direct ? row_stride : tw_words(metric, dim);
    size_t rowParts = 0, colParts = 0;
    for (const TwPair& P : pairs) rowParts += (size_t)P.nChunks * P.nA, colParts += (size_t)P.nRowBlocks * P.nB;
    WorkspaceCarver c = {};
    L.pairs = c.offset(sizeof(TwPair) * npairs);
    L.items = c.offset(sizeof(TwItem) * items.size());
    L.rows = c.offset(L.direct ? 0 : (size_t)rowsTotal * L.ld * 4);
    L.norms = c.offset((size_t)rowsTotal * 4);
    L.rowPart = c.offset(rowParts * sizeof(Top2));
    L.colPart = c.offset(colParts * sizeof(Top2));
    L.total = c.used;
    return L;
}

int tw_check(int desc_is_u8, int metric, int dim, int row_stride, int npairs, const int32_t* pairs_host) {
    GTSFM_CHECK_ARG(metric == 1 || metric == 2, "twoway: metric is 1 (HAMMING) or 2 (EUCLIDEAN)");
    GTSFM_CHECK_ARG(metric == 2 || desc_is_u8, "twoway: HAMMING needs uint8 descriptors");
    GTSFM_CHECK_ARG(dim >= 1 && row_stride >= dim && npairs >= 1 && pairs_host, "twoway: bad arguments");
    GTSFM_CHECK_ARG(npairs <= 65535, "twoway: at most 65535 pairs per call (got %d): split the batch", npairs);
    long long outRows = 0;
    for (int p = 0; p < npairs; ++p) {
        const int32_t* q = pairs_host + 4 * p;
        GTSFM_CHECK_ARG(q[0] >= 0 && q[1] > 0 && q[2] >= 0 && q[3] > 0, "twoway: pair %d has an empty side or a negative offset", p);
        GTSFM_CHECK_ARG(q[1] <= (1 << 30) && q[3] <= (1 << 30), "twoway: pair %d has more than 2^30 rows on a side", p);
        GTSFM_CHECK_ARG((long long)q[0] + q[1] < (1LL << 31) && (long long)q[2] + q[3] < (1LL << 31), "twoway: pair %d exceeds the table", p);
        outRows += q[1];
    }
    GTSFM_CHECK_ARG(outRows < (1LL << 31), "twoway: too many rows");
    return GTSFM_OK;
}

}  // namespace

extern "C" size_t gtsfm_twoway_workspace_bytes(int desc_is_u8, int metric, int dim, int row_stride, int npairs, const int32_t* pairs_host) {
    if (tw_check(desc_is_u8, metric, dim, row_stride, npairs, pairs_host) != GTSFM_OK) return 0;
    std::vector<TwPair> pairs;
    std::vector<TwItem> items;
    int rowsTotal = 0;
    if (tw_plan(npairs, pairs_host, pairs, items, rowsTotal) != GTSFM_OK) return 0;
    // sized for the converted copy, so that any table pointer fits
    return tw_layout(metric, dim, row_stride, false, npairs, items, pairs, rowsTotal).total;
}

extern "C" int gtsfm_twoway_match(const void* desc_dev, int desc_is_u8, int metric, int dim, int row_stride, int npairs, const int32_t* pairs_host,
                                  int use_ratio, double ratio, void* workspace_dev, size_t workspace_bytes, int32_t* matches0_dev,
                                  float* dist0_dev, void* stream_) {
    const int rc = tw_check(desc_is_u8, metric, dim, row_stride, npairs, pairs_host);
    if (rc != GTSFM_OK) return rc;
    GTSFM_CHECK_ARG(desc_dev && workspace_dev && matches0_dev && dist0_dev, "twoway: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<TwPair> pairs;
    std::vector<TwItem> items;
    int rowsTotal = 0;
    if (tw_plan(npairs, pairs_host, pairs, items, rowsTotal) != GTSFM_OK) return GTSFM_ERR_INVALID;
    const TwLayout L = tw_layout(metric, dim, row_stride, tw_direct(desc_is_u8, metric, dim, row_stride, desc_dev), npairs, items, pairs, rowsTotal);
    if (workspace_bytes < L.total) {
        gtsfm_set_error("twoway: workspace too small (%zu < %zu bytes)", workspace_bytes, L.total);
        return GTSFM_ERR_WORKSPACE;
    }
    char* ws = (char*)workspace_dev;
    TwPair* pairs_dev = (TwPair*)(ws + L.pairs);
    TwItem* items_dev = (TwItem*)(ws + L.items);
    float* norms = (float*)(ws + L.norms);
    void* rows = L.direct ? nullptr : (void*)(ws + L.rows);
    if (hipMemcpyAsync(pairs_dev, pairs.data(), sizeof(TwPair) * pairs.size(), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(items_dev, items.data(), sizeof(TwItem) * items.size(), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {  // `pairs` / `items` go out of scope below
        gtsfm_set_error("twoway: copying the batch descriptor failed");
        return GTSFM_ERR_HIP;
    }
    const bool hamming = metric == 1;
    hipLaunchKernelGGL(tw_prep_kernel, dim3(ceil_div(rowsTotal, 4)), dim3(256), 0, stream, desc_dev, desc_is_u8, (int)hamming, dim, row_stride,
                       rowsTotal, rows, L.ld, norms);
    GTSFM_CHECK_LAUNCH("tw_prep_kernel");
    const void* X = L.direct ? desc_dev : rows;
    Top2* rowPart = (Top2*)(ws + L.rowPart);
    Top2* colPart = (Top2*)(ws + L.colPart);
    if (hamming) {
        hipLaunchKernelGGL(tw_tile_kernel<true>, dim3(L.nItems), dim3(256), 0, stream, X, L.ld, L.ld, norms, pairs_dev, items_dev, rowPart, colPart);
    } else {
        hipLaunchKernelGGL(tw_tile_kernel<false>, dim3(L.nItems), dim3(256), 0, stream, X, L.ld, ceil_div(dim, 8), norms, pairs_dev, items_dev,
                           rowPart, colPart);
    }
    GTSFM_CHECK_LAUNCH("tw_tile_kernel");
    int maxA = 0;
    for (const TwPair& P : pairs) maxA = std::max(maxA, P.nA);
    // uint8 rows with 2 * dim * 255^2 < 2^24: every product value is already exact, the direct recomputation would change nothing
    const int refine = !hamming && !(desc_is_u8 && 2LL * dim * 255 * 255 < (1LL << 24));
    hipLaunchKernelGGL(tw_decide_kernel, dim3(ceil_div(maxA, 256), npairs), dim3(256), 0, stream, pairs_dev, rowPart, colPart, (const float*)X,
                       L.ld, L.direct ? dim : L.ld, (int)hamming, refine, use_ratio, ratio, matches0_dev, dist0_dev);
    GTSFM_CHECK_LAUNCH("tw_decide_kernel");
    return GTSFM_OK;
}
