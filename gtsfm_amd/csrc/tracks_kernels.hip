// Feature tracks from verified matches on the device: a union-find over keypoints. See include/gtsfm_amd.h.
//
// A node is a keypoint, node = node_off[image] + k; an edge is an active match row. Every connected component becomes a track unless it
// holds two keypoints of one image. The result is a set partition, so everything here is integer and every output byte is fixed by the
// input's edge SET: not by the order of pairs or rows, not by the grid, not by timing.
//
// LABELLING. The union-find rounds of graph_prims.h (its header comment states the algorithm and its four invariants): trk_hook_kernel decodes
// a match row into its two nodes and calls uf_hook, trk_compress_kernel calls uf_compress, and uf_run_rounds owns the host's loop.
//
// ASSEMBLY (after the fixed point; every step is a launch of its own).
//   count    : atomicAdd(&cnt[label[v]], 1) per touched node: integer adds, any order.
//   A component with more members than images holds two keypoints of one image by pigeonhole: it is counted as discarded and never
//   gathered, so the giant components a few wrong matches create cost nothing. The others ("small") get a segment of cnt members:
//   scan     : exclusive prefix sum of the segment lengths over the nodes (block sums, a scan of the sums, an add).
//   gather   : a touched node of a small component takes slot seg[root] + atomicAdd(&cursor[root], 1): arbitrary order, in bounds because
//              exactly cnt[root] nodes ask.
//   rank     : per such node, over the at most num_images members of its segment: rank = members with a smaller id, and the largest
//              smaller id is its predecessor in node order. Node order is (image, keypoint) order, so an image seen twice shows up as
//              a predecessor of the same image: the track is flagged invalid (stores of the same 1).
//   scan     : exclusive prefix sum over the nodes of (valid root ? 1 : 0, its length): track index and measurement offset, in root order.
//   write    : measurement moff[root] + rank <- (image, keypoint, xy); the root writes track_off; one thread the counts.

#include "../../include/gtsfm_amd.h"
#include "stage_runner.h"

#define TRK_THREADS 256
#define TRK_SCAN_ITEMS 4                                // values per thread of a scan block
#define TRK_SCAN_BLOCK (TRK_THREADS * TRK_SCAN_ITEMS)   // values per scan block
#define TRK_MAX_BLOCKS (1 << 20)                        // grid of the edge kernel; more rows loop inside the kernel

typedef unsigned long long trk_u64;  // a scan value: (count << 32) | length, both below 2^31 in total, so the halves never carry

namespace {

struct TrkWorkspace {
    int *parent, *label, *mark, *cnt, *cursor, *members, *rank, *invalid, *flags;
    trk_u64 *seg, *out, *seg_sums, *out_sums;
    size_t bytes;
};

// the one place that lays the workspace out (the size query passes a null base)
TrkWorkspace trk_layout(void* base, long long num_nodes) {
    TrkWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t n = (size_t)num_nodes;
    w.parent = (int*)ws.take(n * 4);
    w.label = (int*)ws.take(n * 4);
    w.mark = (int*)ws.take(n * 4);
    w.cnt = (int*)ws.take(n * 4);
    w.cursor = (int*)ws.take(n * 4);
    w.members = (int*)ws.take(n * 4);
    w.rank = (int*)ws.take(n * 4);
    w.invalid = (int*)ws.take(n * 4);
    w.seg = (trk_u64*)ws.take(n * 8);
    w.out = (trk_u64*)ws.take(n * 8);
    w.seg_sums = (trk_u64*)ws.take(((n + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK + 1) * 8);
    w.out_sums = (trk_u64*)ws.take(((n + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK + 1) * 8);
    w.flags = (int*)ws.take(UF_FLAG_WORDS * 4);
    w.bytes = ws.used;
    return w;
}

// the image of node v: the largest i with node_off[i] <= v (images without keypoints share an offset with their successor)
__device__ __forceinline__ int trk_image_of(const long long* __restrict__ node_off, int num_images, long long v) {
    int lo = 0, hi = num_images;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (node_off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(TRK_THREADS) void trk_init_kernel(int* __restrict__ parent, int* __restrict__ label, int* __restrict__ mark,
                                                               int* __restrict__ cnt, int* __restrict__ cursor, int* __restrict__ invalid,
                                                               int* __restrict__ flags, long long num_nodes) {
    const long long v = (long long)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (v < UF_FLAG_WORDS) flags[v] = 0;
    if (v >= num_nodes) return;
    parent[v] = (int)v;
    label[v] = (int)v;
    mark[v] = 0;
    cnt[v] = 0;
    cursor[v] = 0;
    invalid[v] = 0;
}

// One thread per match row; the row's pair is found by bisection of match_off. A row whose pair or keypoint index lies outside the
// tables raises flags[0] and touches nothing.
__global__ __launch_bounds__(TRK_THREADS) void trk_hook_kernel(const int* __restrict__ match_idx, const long long* __restrict__ match_off,
                                                               const int* __restrict__ match_count, const uint8_t* __restrict__ mask,
                                                               const uint8_t* __restrict__ pair_enable, const int* __restrict__ pair_images,
                                                               int num_pairs, long long total_matches, const long long* __restrict__ node_off,
                                                               int num_images, long long num_nodes, const int* __restrict__ label, int* parent,
                                                               int* mark, int* flags, int round) {
    for (long long e = (long long)blockIdx.x * TRK_THREADS + threadIdx.x; e < total_matches; e += (long long)gridDim.x * TRK_THREADS) {
        int lo = 0, hi = num_pairs;  // the largest p with match_off[p] <= e
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (match_off[mid] <= e) lo = mid; else hi = mid;
        }
        const int p = lo;
        const long long row = e - match_off[p];
        if (row < 0 || e >= match_off[p + 1]) continue;  // offsets that do not cover this row
        if (pair_enable && !pair_enable[p]) continue;
        if (match_count && row >= match_count[p]) continue;
        if (mask && !mask[e]) continue;
        const int i1 = pair_images[2 * p], i2 = pair_images[2 * p + 1];
        const int k1 = match_idx[2 * e], k2 = match_idx[2 * e + 1];
        bool ok = i1 >= 0 && i1 < num_images && i2 >= 0 && i2 < num_images && k1 >= 0 && k2 >= 0;
        long long u = 0, v = 0;
        if (ok) {
            u = node_off[i1] + k1;
            v = node_off[i2] + k2;
            ok = node_off[i1] >= 0 && node_off[i2] >= 0 && u < node_off[i1 + 1] && v < node_off[i2 + 1] && u < num_nodes && v < num_nodes;
        }
        if (!ok) {
            flags[0] = 1;
            continue;
        }
        uf_hook(parent, label, mark, flags, u, v, round);
    }
}

__global__ __launch_bounds__(TRK_THREADS) void trk_compress_kernel(int* parent, int* __restrict__ label, long long num_nodes) {
    const long long v = (long long)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (v >= num_nodes) return;
    uf_compress(parent, label, v);
}

__global__ __launch_bounds__(TRK_THREADS) void trk_count_kernel(const int* __restrict__ label, const int* __restrict__ mark, int* cnt,
                                                                long long num_nodes) {
    const long long v = (long long)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (v < num_nodes && mark[v]) atomicAdd(&cnt[label[v]], 1);
}

// scan value of node v before the gather: (is a component's root, its segment length or 0 when it is too large to be a track)
__global__ __launch_bounds__(TRK_THREADS) void trk_segment_value_kernel(const int* __restrict__ cnt, int num_images, trk_u64* __restrict__ val,
                                                                        long long num_nodes) {
    const long long v = (long long)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (v >= num_nodes) return;
    const int c = cnt[v];
    val[v] = c > 0 ? ((trk_u64)1 << 32) | (trk_u64)(c <= num_images ? c : 0) : 0;
}

__global__ __launch_bounds__(TRK_THREADS) void trk_gather_kernel(const int* __restrict__ label, const int* __restrict__ mark,
                                                                 const int* __restrict__ cnt, const trk_u64* __restrict__ seg, int num_images,
                                                                 int* cursor, int* __restrict__ members, long long num_nodes) {
    const long long v = (long long)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (v >= num_nodes || !mark[v]) return;
    const int r = label[v], c = cnt[r];
    if (c > num_images) return;
    const int slot = atomicAdd(&cursor[r], 1);
    if (slot < c) members[(long long)(unsigned int)seg[r] + slot] = (int)v;  // always true: exactly c nodes carry this label
}

__global__ __launch_bounds__(TRK_THREADS) void trk_rank_kernel(const int* __restrict__ label, const int* __restrict__ mark,
                                                               const int* __restrict__ cnt, const trk_u64* __restrict__ seg,
                                                               const int* __restrict__ members, const long long* __restrict__ node_off,
                                                               int num_images, int* __restrict__ rank, int* invalid, long long num_nodes) {
    const long long v = (long long)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (v >= num_nodes || !mark[v]) return;
    const int r = label[v], c = cnt[r];
    if (c > num_images) return;
    const int* m = members + (long long)(unsigned int)seg[r];
    int below = 0, pred = -1;
    for (int j = 0; j < c; ++j) {
        const int w = m[j];
        if (w < (int)v) {
            ++below;
            pred = w > pred ? w : pred;
        }
    }
    rank[v] = below;
    if (pred >= 0 && trk_image_of(node_off, num_images, pred) == trk_image_of(node_off, num_images, v)) invalid[r] = 1;
}

// scan value of node v for the output: (is a valid track's root, its length)
__global__ __launch_bounds__(TRK_THREADS) void trk_track_value_kernel(const int* __restrict__ cnt, const int* __restrict__ invalid, int num_images,
                                                                      trk_u64* __restrict__ val, long long num_nodes) {
    const long long v = (long long)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (v >= num_nodes) return;
    const int c = cnt[v];
    val[v] = (c > 0 && c <= num_images && !invalid[v]) ? ((trk_u64)1 << 32) | (trk_u64)c : 0;
}

__global__ __launch_bounds__(TRK_THREADS) void trk_write_kernel(const int* __restrict__ label, const int* __restrict__ mark,
                                                                const int* __restrict__ cnt, const int* __restrict__ invalid,
                                                                const int* __restrict__ rank, const trk_u64* __restrict__ out,
                                                                const trk_u64* __restrict__ seg_total, const trk_u64* __restrict__ out_total,
                                                                const long long* __restrict__ node_off, int num_images,
                                                                const float* __restrict__ kp_xy, long long* __restrict__ track_off,
                                                                int* __restrict__ track_image, int* __restrict__ track_kp,
                                                                float* __restrict__ track_uv, int* __restrict__ counts, int rounds,
                                                                long long num_nodes) {
    const long long v = (long long)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (v == 0) {
        const trk_u64 tot = *out_total;
        const int tracks = (int)(tot >> 32), components = (int)(*seg_total >> 32);
        track_off[tracks] = (long long)(unsigned int)tot;
        counts[0] = tracks;
        counts[1] = (int)(unsigned int)tot;
        counts[2] = components - tracks;
        counts[3] = components;
        counts[4] = rounds;
        counts[5] = counts[6] = counts[7] = 0;
    }
    if (v >= num_nodes || !mark[v]) return;
    const int r = label[v];
    if (cnt[r] > num_images || invalid[r]) return;
    const trk_u64 o = out[r];
    const long long first = (long long)(unsigned int)o;
    if (v == r) track_off[o >> 32] = first;
    const long long at = first + rank[v];
    const int image = trk_image_of(node_off, num_images, v);
    track_image[at] = image;
    track_kp[at] = (int)(v - node_off[image]);
    if (track_uv) {
        track_uv[2 * at] = kp_xy[2 * v];
        track_uv[2 * at + 1] = kp_xy[2 * v + 1];
    }
}

// ---- exclusive prefix sums of trk_u64 values: block sums, a scan of the sums by one workgroup, then an add ----

__global__ __launch_bounds__(TRK_THREADS) void trk_scan_reduce_kernel(const trk_u64* __restrict__ val, long long n, trk_u64* __restrict__ sums) {
    __shared__ trk_u64 lds[TRK_THREADS];
    const long long base = (long long)blockIdx.x * TRK_SCAN_BLOCK + (long long)threadIdx.x * TRK_SCAN_ITEMS;
    trk_u64 s = 0;
#pragma unroll
    for (int k = 0; k < TRK_SCAN_ITEMS; ++k) s += base + k < n ? val[base + k] : 0;
    trk_u64 total;
    block_exclusive_scan<TRK_THREADS>(s, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. m) -> their exclusive scan in place, sums[m] = the total
__global__ __launch_bounds__(TRK_THREADS) void trk_scan_sums_kernel(trk_u64* sums, long long m) {
    __shared__ trk_u64 lds[TRK_THREADS];
    trk_u64 carry = 0;
    for (long long base = 0; base < m; base += TRK_THREADS) {  // m and base are uniform: the barriers inside stay matched
        const long long i = base + threadIdx.x;
        const trk_u64 x = i < m ? sums[i] : 0;
        trk_u64 total;
        const trk_u64 excl = block_exclusive_scan<TRK_THREADS>(x, lds, &total);
        if (i < m) sums[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) sums[m] = carry;
}

__global__ __launch_bounds__(TRK_THREADS) void trk_scan_apply_kernel(trk_u64* val, long long n, const trk_u64* __restrict__ sums) {
    __shared__ trk_u64 lds[TRK_THREADS];
    const long long base = (long long)blockIdx.x * TRK_SCAN_BLOCK + (long long)threadIdx.x * TRK_SCAN_ITEMS;
    trk_u64 x[TRK_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < TRK_SCAN_ITEMS; ++k) {
        x[k] = base + k < n ? val[base + k] : 0;
        s += x[k];
    }
    trk_u64 total;
    trk_u64 run = sums[blockIdx.x] + block_exclusive_scan<TRK_THREADS>(s, lds, &total);
#pragma unroll
    for (int k = 0; k < TRK_SCAN_ITEMS; ++k) {
        if (base + k < n) val[base + k] = run;
        run += x[k];
    }
}

// val[0 .. n) -> its exclusive scan in place; sums[blocks] holds the total afterwards
int trk_exclusive_scan(trk_u64* val, long long n, trk_u64* sums, hipStream_t stream) {
    const long long blocks = (n + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK;
    hipLaunchKernelGGL(trk_scan_reduce_kernel, dim3((unsigned)blocks), dim3(TRK_THREADS), 0, stream, val, n, sums);
    GTSFM_CHECK_LAUNCH("trk_scan_reduce_kernel");
    hipLaunchKernelGGL(trk_scan_sums_kernel, dim3(1), dim3(TRK_THREADS), 0, stream, sums, blocks);
    GTSFM_CHECK_LAUNCH("trk_scan_sums_kernel");
    hipLaunchKernelGGL(trk_scan_apply_kernel, dim3((unsigned)blocks), dim3(TRK_THREADS), 0, stream, val, n, sums);
    GTSFM_CHECK_LAUNCH("trk_scan_apply_kernel");
    return GTSFM_OK;
}

}  // namespace

extern "C" size_t gtsfm_tracks_workspace_bytes(long long num_nodes, long long total_matches) {
    if (num_nodes < 0 || total_matches < 0 || num_nodes >= (1ll << 31)) return 0;
    // the match rows are read where they lie, so only the node count sizes the workspace
    return trk_layout(nullptr, num_nodes).bytes;
}

extern "C" int gtsfm_tracks_from_matches(const int32_t* match_idx_dev, const long long* match_off_dev, const int32_t* match_count_dev,
                                         const uint8_t* inlier_mask_dev, const uint8_t* pair_enable_dev, const int32_t* pair_images_dev, int num_pairs,
                                         long long total_matches, const long long* node_off_dev, int num_images, const float* kp_xy_dev,
                                         void* workspace_dev, size_t workspace_bytes, long long* track_off_dev, int32_t* track_image_dev,
                                         int32_t* track_kp_dev, float* track_uv_dev, int32_t* counts_dev, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GTSFM_CHECK_ARG(num_pairs >= 0 && total_matches >= 0 && num_images >= 0, "gtsfm_tracks_from_matches: negative size (%d pairs, %lld matches, %d images)",
                    num_pairs, total_matches, num_images);
    GTSFM_CHECK_ARG(track_off_dev && counts_dev, "gtsfm_tracks_from_matches: null output pointer");
    const bool empty = num_pairs == 0 || total_matches == 0;
    if (!empty) {
        GTSFM_CHECK_ARG(match_idx_dev && match_off_dev && pair_images_dev && node_off_dev && workspace_dev && track_image_dev && track_kp_dev,
                        "gtsfm_tracks_from_matches: null pointer");
        GTSFM_CHECK_ARG(num_images >= 1, "gtsfm_tracks_from_matches: matches without images");
        GTSFM_CHECK_ARG(!track_uv_dev || kp_xy_dev, "gtsfm_tracks_from_matches: track_uv_dev needs kp_xy_dev");
    }
    if (empty) {
        if (hipMemsetAsync(counts_dev, 0, 8 * sizeof(int32_t), stream) != hipSuccess || hipMemsetAsync(track_off_dev, 0, sizeof(long long), stream) != hipSuccess) {
            gtsfm_set_error("gtsfm_tracks_from_matches: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
            return GTSFM_ERR_HIP;
        }
        return GTSFM_OK;
    }
    long long num_nodes = -1;
    if (hipMemcpyAsync(&num_nodes, node_off_dev + num_images, sizeof(long long), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        gtsfm_set_error("gtsfm_tracks_from_matches: reading node_off_dev[%d] failed: %s", num_images, hipGetErrorString(hipGetLastError()));
        return GTSFM_ERR_HIP;
    }
    GTSFM_CHECK_ARG(((uintptr_t)workspace_dev & 255) == 0, "gtsfm_tracks_from_matches: the workspace must be aligned to 256 bytes");
    GTSFM_CHECK_ARG(num_nodes >= 1 && num_nodes < (1ll << 31), "gtsfm_tracks_from_matches: %lld nodes outside 1 .. 2^31 - 1", num_nodes);
    const TrkWorkspace w = trk_layout(workspace_dev, num_nodes);
    if (workspace_bytes < w.bytes) {
        gtsfm_set_error("gtsfm_tracks_from_matches: workspace of %zu bytes, %zu needed for %lld nodes", workspace_bytes, w.bytes, num_nodes);
        return GTSFM_ERR_WORKSPACE;
    }

    const dim3 threads(TRK_THREADS);
    const long long want_blocks = (num_nodes > UF_FLAG_WORDS ? num_nodes : UF_FLAG_WORDS) + TRK_THREADS - 1;
    const dim3 node_grid((unsigned)(want_blocks / TRK_THREADS));
    const long long edge_blocks = (total_matches + TRK_THREADS - 1) / TRK_THREADS;
    const dim3 edge_grid((unsigned)(edge_blocks < TRK_MAX_BLOCKS ? edge_blocks : TRK_MAX_BLOCKS));

    hipLaunchKernelGGL(trk_init_kernel, node_grid, threads, 0, stream, w.parent, w.label, w.mark, w.cnt, w.cursor, w.invalid, w.flags, num_nodes);
    GTSFM_CHECK_LAUNCH("trk_init_kernel");
    const auto hook = [&](int round) -> int {
        hipLaunchKernelGGL(trk_hook_kernel, edge_grid, threads, 0, stream, match_idx_dev, match_off_dev, match_count_dev, inlier_mask_dev, pair_enable_dev,
                           pair_images_dev, num_pairs, total_matches, node_off_dev, num_images, num_nodes, w.label, w.parent, w.mark, w.flags, round);
        GTSFM_CHECK_LAUNCH("trk_hook_kernel");
        return GTSFM_OK;
    };
    const auto compress = [&]() -> int {
        hipLaunchKernelGGL(trk_compress_kernel, node_grid, threads, 0, stream, w.parent, w.label, num_nodes);
        GTSFM_CHECK_LAUNCH("trk_compress_kernel");
        return GTSFM_OK;
    };
    int rounds = 0;
    DeviceRunner run{stream, "gtsfm_tracks_from_matches"};  // the rounds read their flags back through it
    const UfOutcome labelled = uf_run_rounds(run, w.flags, hook, compress, &rounds);
    if (labelled == UF_FAILED) return GTSFM_ERR_HIP;
    GTSFM_CHECK_ARG(labelled != UF_NO_FIXED_POINT, "gtsfm_tracks_from_matches: no fixed point after %d rounds (%lld nodes, %lld match rows, %d pairs); nothing was written",
                    rounds, num_nodes, total_matches, num_pairs);
    GTSFM_CHECK_ARG(labelled != UF_BAD_INPUT, "gtsfm_tracks_from_matches: an active match row names an image outside 0 .. %d or a keypoint outside its image's table; nothing was written",
                    num_images - 1);

    hipLaunchKernelGGL(trk_count_kernel, node_grid, threads, 0, stream, w.label, w.mark, w.cnt, num_nodes);
    GTSFM_CHECK_LAUNCH("trk_count_kernel");
    hipLaunchKernelGGL(trk_segment_value_kernel, node_grid, threads, 0, stream, w.cnt, num_images, w.seg, num_nodes);
    GTSFM_CHECK_LAUNCH("trk_segment_value_kernel");
    const long long scan_blocks = (num_nodes + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK;
    int rc = trk_exclusive_scan(w.seg, num_nodes, w.seg_sums, stream);
    if (rc != GTSFM_OK) return rc;
    hipLaunchKernelGGL(trk_gather_kernel, node_grid, threads, 0, stream, w.label, w.mark, w.cnt, w.seg, num_images, w.cursor, w.members, num_nodes);
    GTSFM_CHECK_LAUNCH("trk_gather_kernel");
    hipLaunchKernelGGL(trk_rank_kernel, node_grid, threads, 0, stream, w.label, w.mark, w.cnt, w.seg, w.members, node_off_dev, num_images, w.rank, w.invalid,
                       num_nodes);
    GTSFM_CHECK_LAUNCH("trk_rank_kernel");
    hipLaunchKernelGGL(trk_track_value_kernel, node_grid, threads, 0, stream, w.cnt, w.invalid, num_images, w.out, num_nodes);
    GTSFM_CHECK_LAUNCH("trk_track_value_kernel");
    rc = trk_exclusive_scan(w.out, num_nodes, w.out_sums, stream);
    if (rc != GTSFM_OK) return rc;
    hipLaunchKernelGGL(trk_write_kernel, node_grid, threads, 0, stream, w.label, w.mark, w.cnt, w.invalid, w.rank, w.out, w.seg_sums + scan_blocks, w.out_sums + scan_blocks,
                       node_off_dev, num_images, kp_xy_dev, track_off_dev, track_image_dev, track_kp_dev, track_uv_dev, counts_dev,
                       rounds, num_nodes);
    GTSFM_CHECK_LAUNCH("trk_write_kernel");
    return GTSFM_OK;
}
