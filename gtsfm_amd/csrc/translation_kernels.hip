// 1DSfM translation outlier rejection on the device: TranslationAveraging1DSFM.compute_inliers with gtsam's greedy minimum-feedback-arc-set
// ordering (MFAS) per projection direction. See include/gtsfm_amd.h; the specification is tests/translation_inliers_reference.py.
//
// NODES AND EDGES. Camera i is node i, landmark (track) j is node num_images + j. Row m of the unified edge table is pair row m for m < E
// (key1, key2) = (i2, i1), and measurement m - E otherwise, (key1, key2) = (camera, num_images + track). Everything is float64 + - * / sqrt
// and comparisons in one stated order (-ffp-contract=off), and no floating-point atomic exists anywhere: the bytes are the specification's.
//   phase 1  edge table : one lane per row: validity, the world direction unit(wRi . v), the two keys; integer atomicAdd on both degrees.
//   phase 2  adjacency  : has-an-edge flags and degrees are scanned (one workgroup) into compact node ids (ascending node id, so "smallest
//            id" means the same in both numberings) and list offsets; an edge takes an arbitrary slot of both lists (atomic cursor), then
//            every entry is ranked within its node's list by (key1, key2) and moved to its place: the lists are in ascending edge order,
//            which is the order the specification sums a node's weights in. Two entries with one key are a duplicate and raise a flag.
//            The host reads the flags and the node count G here, before any output but the world directions is written.
//   phase 3  MFAS       : one workgroup per projection direction (a fixed number of workgroups walks the directions). Lane l owns nodes
//            l, l + 256, ...: it sums its nodes' inW / outW serially from the lists and keeps score = +inf for a root (inW < 1e-8), else
//            (outW + 1) / (inW + 1); a removed node has score -1. Per step every lane reduces its nodes to (score, id), a fixed tree (wave
//            shuffles, then the four wave results through LDS) picks the largest score with the smallest id -- among roots that is the
//            smallest root, as specified -- and the lanes stride over the chosen node's list: each remaining neighbour is a distinct
//            node, so the updates are plain read-modify-writes, followed by the neighbour's new score by the same expression. Two
//            barriers per step. inW, outW and score live in LDS up to lds_node_limit nodes (24 bytes per node) and in a per-workgroup
//            slice of the workspace beyond it, through the same code: the pointer differs, the bytes do not.
//   phase 4  aggregate  : one lane per row walks the directions in order, recomputes |w| by the same instruction sequence, reads the two
//            positions, adds and thresholds; inlier pairs mark their cameras (plain stores of 1), then a measurement stays an inlier only
//            when its camera is marked. The intermediate is D x G int32, not D x rows float64.
// Every per-index step is a GTSFM_HD function, and the call is one function over a runner of stage_runner.h (tr_inliers_stages): the device
// call launches its stages, tools/translation_inliers_host_main.cpp walks the same stages in another order and lane partition on a CPU,
// where the atomics become plain updates.

#include <math.h>

#include "../../include/gtsfm_amd.h"
#include "stage_runner.h"

#define TR_THREADS 256
#define TR_WAVE 64
#define TR_MAX_ROWS (1ll << 28)
#define TR_MAX_NODES (1ll << 28)
#define TR_MAX_DIRECTIONS (1ll << 20)
#define TR_MAX_GROUPS 768   // workgroups of the MFAS kernel: three per CU of an MI355X; the result does not depend on it
#define TR_LDS_NODES 2048   // 48 KiB of LDS per workgroup: three workgroups per CU
#define TR_FLAG_WORDS 8     // 0: a bad pair row; 1: a duplicate; 2: a measurement's camera out of range; 3: its camera has no rotation
#define TR_ROOT_EPSILON 1e-8
#define TR_DEAD (-1.0)

namespace {

struct TrWorkspace {
    long long *row_off, *cid, *coff;  // [NT + 1] degrees then list offsets by node id; [NT + 1] has-an-edge then compact ids; [cap + 1] compact offsets
    int *cursor, *key1, *key2, *raw_edge, *raw_owner, *adj_nbr, *adj_edge, *flags, *pos;
    double* state;  // [groups][3][cap] beyond the LDS tier
    size_t bytes;
};

GTSFM_HD long long tr_groups(long long num_directions) { return num_directions < TR_MAX_GROUPS ? (num_directions > 0 ? num_directions : 1) : TR_MAX_GROUPS; }
GTSFM_HD long long tr_lds_limit(int lds_node_limit) { return lds_node_limit < 0 || lds_node_limit > TR_LDS_NODES ? TR_LDS_NODES : lds_node_limit; }

TrWorkspace tr_layout(void* base, long long rows, long long nodes, long long num_directions, long long node_capacity, int lds_node_limit) {
    TrWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t m = (size_t)rows, nt = (size_t)nodes, cap = (size_t)node_capacity, d = (size_t)(num_directions > 0 ? num_directions : 0);
    w.row_off = (long long*)ws.take((nt + 1) * 8);
    w.cid = (long long*)ws.take((nt + 1) * 8);
    w.coff = (long long*)ws.take((cap + 1) * 8);
    w.cursor = (int*)ws.take(nt * 4);
    w.key1 = (int*)ws.take(m * 4);
    w.key2 = (int*)ws.take(m * 4);
    w.raw_edge = (int*)ws.take(2 * m * 4);
    w.raw_owner = (int*)ws.take(2 * m * 4);
    w.adj_nbr = (int*)ws.take(2 * m * 4);
    w.adj_edge = (int*)ws.take(2 * m * 4);
    w.flags = (int*)ws.take(TR_FLAG_WORDS * 4);
    w.pos = (int*)ws.take(d * cap * 4);
    w.state = (double*)ws.take((long long)cap > tr_lds_limit(lds_node_limit) ? (size_t)tr_groups(num_directions) * 3 * cap * 8 : 0);
    w.bytes = ws.used;
    return w;
}

struct TrGraph {  // what the per-index functions read and write
    const int* pair_images;
    const double* pair_direction;
    const uint8_t* pair_enable;
    const double* rotation;
    const uint8_t* rotation_valid;
    const double* intrinsics;
    const long long* track_off;
    const int* image;
    const float* uv;
    const uint8_t* track_enable;
    const uint8_t* meas_enable;
    const double* directions;
    long long num_pairs, num_meas, num_tracks, num_directions;
    int num_images, directions_given;
    double *world_pair, *world_meas;
    TrWorkspace w;
};

GTSFM_HD long long tr_rows(const TrGraph& g) { return g.num_pairs + g.num_meas; }
GTSFM_HD long long tr_nodes(const TrGraph& g) { return (long long)g.num_images + g.num_tracks; }
GTSFM_HD double* tr_world_row(const TrGraph& g, long long m) { return m < g.num_pairs ? g.world_pair + 3 * m : g.world_meas + 3 * (m - g.num_pairs); }

// w = (mx dx + my dy) + mz dz
GTSFM_HD double tr_project(const double* __restrict__ m, const double* __restrict__ d) { return (m[0] * d[0] + m[1] * d[1]) + m[2] * d[2]; }

GTSFM_HD void tr_unit(double* v) {
    const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] = v[0] / n, v[1] = v[1] / n, v[2] = v[2] / n;
}

// out = unit(R v), every row of the product summed as (r0 x + r1 y) + r2 z
GTSFM_HD void tr_rotate_unit(const double* __restrict__ r, const double* v, double* out) {
    for (int k = 0; k < 3; ++k) out[k] = (r[3 * k] * v[0] + r[3 * k + 1] * v[1]) + r[3 * k + 2] * v[2];
    tr_unit(out);
}

GTSFM_HD double tr_score(double in_w, double out_w) { return in_w < TR_ROOT_EPSILON ? HUGE_VAL : (out_w + 1.0) / (in_w + 1.0); }

// the track of measurement s: the last t with track_off[t] <= s, held inside 0 .. T - 1 whatever the array holds
GTSFM_HD long long tr_track_of(const TrGraph& g, long long s) {
    long long lo = 0, hi = g.num_tracks - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) / 2;
        if (g.track_off[mid] <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- phase 1 and 2 ----

GTSFM_HD void tr_init(const TrGraph& g, long long i, uint8_t* __restrict__ camera_inlier) {
    if (i < TR_FLAG_WORDS) g.w.flags[i] = 0;
    if (i <= tr_nodes(g)) g.w.row_off[i] = 0, g.w.cid[i] = 0;
    if (i < tr_nodes(g)) g.w.cursor[i] = 0;
    if (i < g.num_images) camera_inlier[i] = 0;
}

GTSFM_HD void tr_edge_table(const TrGraph& g, long long m) {
    const double nan = __builtin_nan("");
    double* out = tr_world_row(g, m);
    double w[3] = {nan, nan, nan};
    int k1 = -1, k2 = -1;
    if (m < g.num_pairs) {
        if (!g.pair_enable || g.pair_enable[m]) {
            const int i1 = g.pair_images[2 * m], i2 = g.pair_images[2 * m + 1];
            if (!(i1 >= 0 && i1 < i2 && i2 < g.num_images)) {
                g.w.flags[0] = 1;
            } else if (g.directions_given) {
                w[0] = out[0], w[1] = out[1], w[2] = out[2];
                k1 = i2, k2 = i1;
            } else if (g.rotation_valid[i2]) {  // wRi[i1] is not looked at: the reference's quirk
                tr_rotate_unit(g.rotation + 9 * (long long)i2, g.pair_direction + 3 * m, w);
                k1 = i2, k2 = i1;
            }
        }
    } else {
        const long long s = m - g.num_pairs, t = tr_track_of(g, s);
        if (g.track_enable[t] && (!g.meas_enable || g.meas_enable[s])) {
            const int cam = g.image[s];
            if (!(cam >= 0 && cam < g.num_images)) {
                g.w.flags[2] = 1;
            } else if (g.directions_given) {
                w[0] = out[0], w[1] = out[1], w[2] = out[2];
                k1 = cam, k2 = (int)(g.num_images + t);
            } else if (!g.rotation_valid[cam]) {
                g.w.flags[3] = 1;
            } else {
                const double* k = g.intrinsics + 4 * (long long)cam;
                double ray[3] = {((double)g.uv[2 * s] - k[2]) / k[0], ((double)g.uv[2 * s + 1] - k[3]) / k[1], 1.0};
                tr_unit(ray);
                tr_rotate_unit(g.rotation + 9 * (long long)cam, ray, w);
                k1 = cam, k2 = (int)(g.num_images + t);
            }
        }
    }
    if (k1 >= 0 && !(isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]))) k1 = k2 = -1;
    if (k1 < 0) w[0] = w[1] = w[2] = nan;
    out[0] = w[0], out[1] = w[1], out[2] = w[2];
    g.w.key1[m] = k1, g.w.key2[m] = k2;
    if (k1 >= 0) {
        hd_atomic_add(&g.w.row_off[k1], 1);
        hd_atomic_add(&g.w.row_off[k2], 1);
    }
}

GTSFM_HD void tr_node_flag(const TrGraph& g, long long n) { g.w.cid[n] = g.w.row_off[n] > 0 ? 1 : 0; }

// after both scans: the compact offsets
GTSFM_HD void tr_node_compact(const TrGraph& g, long long n, long long node_capacity) {
    const long long c = g.w.cid[n];
    if (n == tr_nodes(g)) {
        if (c <= node_capacity) g.w.coff[c] = g.w.row_off[n];
    } else if (g.w.cid[n + 1] > c && c < node_capacity) {
        g.w.coff[c] = g.w.row_off[n];
    }
}

GTSFM_HD void tr_edge_fill(const TrGraph& g, long long m) {
    const int k1 = g.w.key1[m], k2 = g.w.key2[m];
    if (k1 < 0) return;
    const long long s1 = g.w.row_off[k1] + hd_atomic_add(&g.w.cursor[k1], 1), s2 = g.w.row_off[k2] + hd_atomic_add(&g.w.cursor[k2], 1);
    if (s1 < g.w.row_off[k1 + 1]) g.w.raw_edge[s1] = (int)m, g.w.raw_owner[s1] = k1;  // always true: exactly degree rows ask
    if (s2 < g.w.row_off[k2 + 1]) g.w.raw_edge[s2] = (int)m, g.w.raw_owner[s2] = k2;
}

GTSFM_HD void tr_slot_rank(const TrGraph& g, long long s) {
    if (s >= g.w.row_off[tr_nodes(g)]) return;
    const int edge = g.w.raw_edge[s], owner = g.w.raw_owner[s], k1 = g.w.key1[edge], k2 = g.w.key2[edge];
    const long long lo = g.w.row_off[owner], hi = g.w.row_off[owner + 1];
    long long rank = 0;
    for (long long j = lo; j < hi; ++j) {
        const int ej = g.w.raw_edge[j], j1 = g.w.key1[ej], j2 = g.w.key2[ej];
        if (j1 < k1 || (j1 == k1 && j2 < k2)) ++rank;
        if (j1 == k1 && j2 == k2 && ej != edge) {
            g.w.flags[1] = 1;
            if (ej < edge) ++rank;  // keeps the slots distinct; the call is refused anyway
        }
    }
    g.w.adj_nbr[lo + rank] = (int)g.w.cid[owner == k1 ? k2 : k1];
    g.w.adj_edge[lo + rank] = 2 * edge + (owner == k1 ? 1 : 0);
}

// ---- phase 3 ----

struct TrState {
    double *in_w, *out_w, *score;
    int* pos;
};
struct TrKey {
    double score;
    int id;
};

GTSFM_HD TrKey tr_key_max(const TrKey a, const TrKey b) { return (b.score > a.score || (b.score == a.score && b.id < a.id)) ? b : a; }

// |w| of list entry j of node c, and whether c is the source of that edge (the edge runs key1 -> key2 when w >= 0, +-0 included)
GTSFM_HD double tr_entry_weight(const TrGraph& g, long long j, const double* __restrict__ d, bool* node_is_source) {
    const int e2 = g.w.adj_edge[j];
    const double w = tr_project(tr_world_row(g, e2 >> 1), d);
    const bool forward = !(w < 0);
    *node_is_source = forward == ((e2 & 1) != 0);
    return fabs(w);
}

GTSFM_HD void tr_mfas_init_lane(const TrGraph& g, const TrState& st, const double* __restrict__ d, int num_nodes, int lane, int lanes) {
    for (int c = lane; c < num_nodes; c += lanes) {
        double in_w = 0.0, out_w = 0.0;
        for (long long j = g.w.coff[c]; j < g.w.coff[c + 1]; ++j) {
            bool source;
            const double a = tr_entry_weight(g, j, d, &source);
            if (source) out_w = out_w + a; else in_w = in_w + a;
        }
        st.in_w[c] = in_w, st.out_w[c] = out_w, st.score[c] = tr_score(in_w, out_w);
    }
}

GTSFM_HD TrKey tr_mfas_lane_best(const TrState& st, int num_nodes, int lane, int lanes) {
    TrKey best = {TR_DEAD, 0x7FFFFFFF};
    for (int c = lane; c < num_nodes; c += lanes) {
        const double s = st.score[c];
        if (s > best.score) best.score = s, best.id = c;  // ascending c: the first of equal scores stays
    }
    return best;
}

GTSFM_HD void tr_mfas_update_lane(const TrGraph& g, const TrState& st, const double* __restrict__ d, int choice, int step, int lane, int lanes) {
    for (long long j = g.w.coff[choice] + lane; j < g.w.coff[choice + 1]; j += lanes) {
        const int nbr = g.w.adj_nbr[j];
        if (st.score[nbr] == TR_DEAD) continue;
        bool choice_is_source;
        const double a = tr_entry_weight(g, j, d, &choice_is_source);
        if (choice_is_source) st.in_w[nbr] = st.in_w[nbr] - a; else st.out_w[nbr] = st.out_w[nbr] - a;
        st.score[nbr] = tr_score(st.in_w[nbr], st.out_w[nbr]);
    }
    if (lane == 0) st.pos[choice] = step, st.score[choice] = TR_DEAD;  // no list of `choice` holds `choice`: no edge joins a node to itself
}

// ---- phase 4 ----

GTSFM_HD void tr_row_aggregate(const TrGraph& g, long long m, int num_nodes, double threshold, double* __restrict__ pair_weight, double* __restrict__ meas_weight,
                            uint8_t* __restrict__ pair_inlier, uint8_t* __restrict__ meas_inlier, uint8_t* __restrict__ camera_inlier) {
    const int k1 = g.w.key1[m], k2 = g.w.key2[m];
    double mean = __builtin_nan("");
    bool inlier = false;
    if (k1 >= 0) {
        const long long c1 = g.w.cid[k1], c2 = g.w.cid[k2];
        const double* row = tr_world_row(g, m);
        double sum = 0.0;
        for (long long k = 0; k < g.num_directions; ++k) {
            const double w = tr_project(row, g.directions + 3 * k);
            const int p1 = g.w.pos[k * num_nodes + c1], p2 = g.w.pos[k * num_nodes + c2];
            const bool violated = !(w < 0) ? p1 > p2 : p2 > p1;
            sum = sum + (violated ? fabs(w) : 0.0);
        }
        mean = sum / (double)g.num_directions;
        inlier = mean < threshold;
    }
    if (m < g.num_pairs) {
        pair_weight[m] = mean, pair_inlier[m] = inlier ? 1 : 0;
        if (inlier) camera_inlier[k1] = 1, camera_inlier[k2] = 1;
    } else {
        meas_weight[m - g.num_pairs] = mean, meas_inlier[m - g.num_pairs] = inlier ? 1 : 0;
    }
}

// only add an inlier camera-track measurement if the camera has camera-camera inliers
GTSFM_HD void tr_meas_filter(const TrGraph& g, long long s, const uint8_t* __restrict__ camera_inlier, uint8_t* __restrict__ meas_inlier) {
    if (meas_inlier[s] && !camera_inlier[g.image[s]]) meas_inlier[s] = 0;  // an inlier is a valid row: its camera is in range
}

GTSFM_HD void tr_position_out(const TrGraph& g, long long i, int num_nodes, int* __restrict__ position) {
    const long long nt = tr_nodes(g), n = i % nt, k = i / nt;
    position[i] = g.w.cid[n + 1] > g.w.cid[n] ? g.w.pos[k * num_nodes + g.w.cid[n]] : -1;
}

// One workgroup per direction, gridDim.x workgroups walking the directions. num_nodes, the step count and the direction index are uniform:
// the barriers stay matched. Dynamic LDS: 3 * num_nodes doubles when use_lds.
__global__ __launch_bounds__(TR_THREADS) void tr_mfas_kernel(TrGraph g, int num_nodes, int use_lds, long long node_capacity) {
    extern __shared__ double tr_lds[];
    __shared__ double wave_score[TR_THREADS / TR_WAVE];
    __shared__ int wave_id[TR_THREADS / TR_WAVE];
    const int tid = threadIdx.x;
    double* base = use_lds ? tr_lds : g.w.state + (size_t)blockIdx.x * 3 * (size_t)node_capacity;
    for (long long k = blockIdx.x; k < g.num_directions; k += gridDim.x) {
        const TrState st = {base, base + num_nodes, base + 2 * (size_t)num_nodes, g.w.pos + k * num_nodes};
        const double* d = g.directions + 3 * k;
        tr_mfas_init_lane(g, st, d, num_nodes, tid, TR_THREADS);
        __syncthreads();
        for (int step = 0; step < num_nodes; ++step) {
            TrKey key = tr_mfas_lane_best(st, num_nodes, tid, TR_THREADS);
#pragma unroll
            for (int off = TR_WAVE / 2; off > 0; off >>= 1) {
                TrKey other;
                other.score = __shfl_xor(key.score, off, TR_WAVE);
                other.id = __shfl_xor(key.id, off, TR_WAVE);
                key = tr_key_max(key, other);
            }
            if (tid % TR_WAVE == 0) wave_score[tid / TR_WAVE] = key.score, wave_id[tid / TR_WAVE] = key.id;
            __syncthreads();
            key.score = wave_score[0], key.id = wave_id[0];
#pragma unroll
            for (int w = 1; w < TR_THREADS / TR_WAVE; ++w) key = tr_key_max(key, TrKey{wave_score[w], wave_id[w]});
            // key.id < num_nodes: step < num_nodes nodes have been removed, so some lane saw a score above TR_DEAD
            if (key.id < num_nodes) tr_mfas_update_lane(g, st, d, key.id, step, tid, TR_THREADS);
            __syncthreads();
        }
    }
}
// its stand-in on a CPU: one workgroup at a time, so every direction takes the first state slice; one lane, or the device's 256
void tr_mfas_host(const HostRunner& run, const TrGraph& g, int num_nodes) {
    const int lanes = run.device_lanes ? TR_THREADS : 1;
    TrKey keys[TR_THREADS];
    run.walk(g.num_directions, [&](long long k) {
        double* base = g.w.state;
        const TrState st = {base, base + num_nodes, base + 2 * (size_t)num_nodes, g.w.pos + k * num_nodes};
        const double* d = g.directions + 3 * k;
        run.walk(lanes, [&](long long lane) { tr_mfas_init_lane(g, st, d, num_nodes, (int)lane, lanes); });
        for (int step = 0; step < num_nodes; ++step) {
            run.walk(lanes, [&](long long lane) { keys[lane] = tr_mfas_lane_best(st, num_nodes, (int)lane, lanes); });
            TrKey key = keys[run.descending ? lanes - 1 : 0];
            run.walk(lanes, [&](long long lane) { key = tr_key_max(key, keys[lane]); });
            if (key.id < num_nodes) run.walk(lanes, [&](long long lane) { tr_mfas_update_lane(g, st, d, key.id, step, (int)lane, lanes); });
        }
    });
}

// the counts: one workgroup walks the rows (integer sums by a tree, no atomics on one word)
__global__ __launch_bounds__(SCAN_THREADS) void tr_counts_kernel(TrGraph g, int num_nodes, const uint8_t* __restrict__ pair_inlier, const uint8_t* __restrict__ meas_inlier,
                                                                   const uint8_t* __restrict__ camera_inlier, int* __restrict__ counts) {
    __shared__ long long lds[SCAN_THREADS];
    long long pe = 0, me = 0, pi = 0, mi = 0, ci = 0;
    for (long long m = threadIdx.x; m < g.num_pairs; m += SCAN_THREADS) pe += g.w.key1[m] >= 0 ? 1 : 0, pi += pair_inlier[m] ? 1 : 0;
    for (long long s = threadIdx.x; s < g.num_meas; s += SCAN_THREADS) me += g.w.key1[g.num_pairs + s] >= 0 ? 1 : 0, mi += meas_inlier[s] ? 1 : 0;
    for (long long c = threadIdx.x; c < g.num_images; c += SCAN_THREADS) ci += camera_inlier[c] ? 1 : 0;
    const auto add = [](long long a, long long b) { return a + b; };
    pe = block_reduce<SCAN_THREADS>(pe, lds, add), me = block_reduce<SCAN_THREADS>(me, lds, add), pi = block_reduce<SCAN_THREADS>(pi, lds, add);
    mi = block_reduce<SCAN_THREADS>(mi, lds, add), ci = block_reduce<SCAN_THREADS>(ci, lds, add);
    if (threadIdx.x == 0) {
        counts[0] = (int)pe, counts[1] = (int)me, counts[2] = num_nodes, counts[3] = (int)pi, counts[4] = (int)mi, counts[5] = (int)ci;
        counts[6] = counts[7] = 0;
    }
}
// its stand-in on a CPU
void tr_counts_host(const HostRunner& run, const TrGraph& g, int num_nodes, const uint8_t* pair_inlier, const uint8_t* meas_inlier, const uint8_t* camera_inlier,
                    int* counts) {
    memset(counts, 0, 8 * sizeof(int));
    counts[2] = num_nodes;
    run.walk(g.num_pairs, [&](long long m) { counts[0] += g.w.key1[m] >= 0 ? 1 : 0, counts[3] += pair_inlier[m] ? 1 : 0; });
    run.walk(g.num_meas, [&](long long s) { counts[1] += g.w.key1[g.num_pairs + s] >= 0 ? 1 : 0, counts[4] += meas_inlier[s] ? 1 : 0; });
    run.walk(g.num_images, [&](long long c) { counts[5] += camera_inlier[c] ? 1 : 0; });
}

bool tr_sizes_ok(long long num_pairs, long long num_meas, long long num_images, long long num_tracks, long long num_directions, long long node_capacity) {
    return num_pairs >= 0 && num_meas >= 0 && num_images >= 0 && num_tracks >= 0 && num_directions >= 0 && node_capacity >= 0 && num_pairs + num_meas < TR_MAX_ROWS &&
           num_images + num_tracks < TR_MAX_NODES && num_directions < TR_MAX_DIRECTIONS && node_capacity <= num_images + num_tracks &&
           (num_directions == 0 || node_capacity < (1ll << 31) / num_directions);
}

// ---- the pipeline: every stage once, for the device call and for tools/translation_inliers_host_main.cpp (stage_runner.h) ----

// g.w is laid out for node_capacity nodes with an edge and lds_node_limit
template <class Runner>
int tr_inliers_stages(Runner& run, const char* me, const TrGraph& g, double threshold, long long node_capacity, int lds_node_limit, double* pair_weight,
                      double* meas_weight, uint8_t* pair_inlier, uint8_t* meas_inlier, uint8_t* camera_inlier, int* position, int* counts) {
    const long long rows = tr_rows(g), nodes = tr_nodes(g);
    GTSFM_CHECK_ARG(g.num_directions > 0 || rows == 0, "%s: no projection direction for %lld rows; nothing was written", me, rows);
    run.template each<struct tr_init_stage>(nodes + 1 > TR_FLAG_WORDS ? nodes + 1 : TR_FLAG_WORDS, STAGE_FN(long long i) { tr_init(g, i, camera_inlier); });
    run.template each<struct tr_edge_table_stage>(rows, STAGE_FN(long long i) { tr_edge_table(g, i); });
    run.template each<struct tr_node_flag_stage>(nodes, STAGE_FN(long long i) { tr_node_flag(g, i); });
    run.scan(g.w.row_off, nodes);
    run.scan(g.w.cid, nodes);
    run.template each<struct tr_node_compact_stage>(nodes + 1, STAGE_FN(long long i) { tr_node_compact(g, i, node_capacity); });
    run.template each<struct tr_edge_fill_stage>(rows, STAGE_FN(long long i) { tr_edge_fill(g, i); });
    run.template each<struct tr_slot_rank_stage>(2 * rows, STAGE_FN(long long i) { tr_slot_rank(g, i); });
    int flags[4] = {0, 0, 0, 0};
    long long graph_nodes = -1;
    run.copy(flags, g.w.flags, 4, "building the adjacency");
    if (run.fetch(&graph_nodes, g.w.cid + nodes, 1, "building the adjacency") != GTSFM_OK) return run.status;
    GTSFM_CHECK_ARG(!flags[0], "%s: an enabled pair row has i1 >= i2 or names an image outside 0 .. %d", me, g.num_images - 1);
    GTSFM_CHECK_ARG(!flags[2], "%s: an enabled measurement names a camera outside 0 .. %d", me, g.num_images - 1);
    GTSFM_CHECK_ARG(!flags[3], "%s: an enabled measurement's camera has no valid rotation", me);
    GTSFM_CHECK_ARG(!flags[1], "%s: a measurement is listed twice", me);
    GTSFM_CHECK_ARG(graph_nodes >= 0 && graph_nodes <= nodes, "%s: %lld graph nodes of %lld", me, graph_nodes, nodes);
    if (graph_nodes > node_capacity) {
        gtsfm_set_error("%s: %lld nodes have an edge, the workspace holds %lld (node_capacity)", me, graph_nodes, node_capacity);
        return GTSFM_ERR_WORKSPACE;
    }
    const int num_nodes = (int)graph_nodes;
    const int use_lds = graph_nodes <= tr_lds_limit(lds_node_limit) ? 1 : 0;
    GTSFM_CHECK_ARG(use_lds || node_capacity > tr_lds_limit(lds_node_limit), "%s: internal: no state slice", me);
    if (num_nodes > 0)
        run.block(
            "tr_mfas_kernel",
            [&](hipStream_t stream) {
                hipLaunchKernelGGL(tr_mfas_kernel, dim3((unsigned)tr_groups(g.num_directions)), dim3(TR_THREADS), use_lds ? (size_t)3 * num_nodes * sizeof(double) : 0, stream, g,
                                   num_nodes, use_lds, node_capacity);
            },
            [&](const HostRunner& host) { tr_mfas_host(host, g, num_nodes); });
    run.template each<struct tr_row_aggregate_stage>(rows, STAGE_FN(long long i) {
        tr_row_aggregate(g, i, num_nodes, threshold, pair_weight, meas_weight, pair_inlier, meas_inlier, camera_inlier);
    });
    run.template each<struct tr_meas_filter_stage>(g.num_meas, STAGE_FN(long long i) { tr_meas_filter(g, i, camera_inlier, meas_inlier); });
    run.block(
        "tr_counts_kernel",
        [&](hipStream_t stream) {
            hipLaunchKernelGGL(tr_counts_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, g, num_nodes, pair_inlier, meas_inlier, camera_inlier, counts);
        },
        [&](const HostRunner& host) { tr_counts_host(host, g, num_nodes, pair_inlier, meas_inlier, camera_inlier, counts); });
    if (position && g.num_directions * nodes > 0)
        run.template each<struct tr_position_out_stage>(g.num_directions * nodes, STAGE_FN(long long i) { tr_position_out(g, i, num_nodes, position); });
    return run.status;
}

}  // namespace

extern "C" size_t gtsfm_translation_inliers_workspace_bytes(long long num_pairs, long long num_meas, long long num_images, long long num_tracks,
                                                            long long num_directions, long long node_capacity, int lds_node_limit) {
    if (!tr_sizes_ok(num_pairs, num_meas, num_images, num_tracks, num_directions, node_capacity)) return 0;
    return tr_layout(nullptr, num_pairs + num_meas, num_images + num_tracks, num_directions, node_capacity, lds_node_limit).bytes;
}

extern "C" int gtsfm_translation_inliers_f64(const int32_t* pair_images_dev, const double* pair_direction_dev, const uint8_t* pair_enable_dev, long long num_pairs,
                                             const double* rotation_dev, const uint8_t* rotation_valid_dev, const double* intrinsics_dev, int num_images,
                                             const long long* track_off_dev, const int32_t* image_dev, const float* uv_dev, const uint8_t* track_enable_dev,
                                             const uint8_t* meas_enable_dev, long long num_tracks, long long num_meas, const double* directions_dev,
                                             long long num_directions, double threshold, int directions_given, long long node_capacity, int lds_node_limit,
                                             void* workspace_dev, size_t workspace_bytes, double* world_pair_dev, double* world_meas_dev, double* pair_weight_dev,
                                             double* meas_weight_dev, uint8_t* pair_inlier_dev, uint8_t* meas_inlier_dev, uint8_t* camera_inlier_dev,
                                             int32_t* position_dev, int32_t* counts_dev, void* stream_) {
    const char* me = "gtsfm_translation_inliers_f64";
    GTSFM_CHECK_ARG(tr_sizes_ok(num_pairs, num_meas, num_images, num_tracks, num_directions, node_capacity),
                    "%s: sizes out of range (%lld pairs, %lld measurements, %d images, %lld tracks, %lld directions, node capacity %lld)", me, num_pairs, num_meas, num_images,
                    num_tracks, num_directions, node_capacity);
    GTSFM_CHECK_ARG(counts_dev && workspace_dev && (num_images == 0 || camera_inlier_dev), "%s: null pointer", me);
    GTSFM_CHECK_ARG(num_pairs == 0 || (pair_images_dev && world_pair_dev && pair_weight_dev && pair_inlier_dev && (directions_given || (pair_direction_dev && rotation_dev && rotation_valid_dev))),
                    "%s: null pair pointer", me);
    GTSFM_CHECK_ARG(num_meas == 0 || (num_tracks > 0 && track_off_dev && image_dev && track_enable_dev && world_meas_dev && meas_weight_dev && meas_inlier_dev &&
                                      (directions_given || (uv_dev && rotation_dev && rotation_valid_dev && intrinsics_dev))),
                    "%s: null measurement pointer", me);
    GTSFM_CHECK_ARG(num_directions == 0 || directions_dev, "%s: null directions_dev", me);
    const long long rows = num_pairs + num_meas, nodes = (long long)num_images + num_tracks;
    TrGraph g{pair_images_dev, pair_direction_dev, pair_enable_dev, rotation_dev, rotation_valid_dev, intrinsics_dev, track_off_dev, image_dev, uv_dev, track_enable_dev,
              meas_enable_dev, directions_dev, num_pairs, num_meas, num_tracks, num_directions, num_images, directions_given ? 1 : 0, world_pair_dev, world_meas_dev,
              tr_layout(workspace_dev, rows, nodes, num_directions, node_capacity, lds_node_limit)};
    const int fits = gtsfm_check_workspace(me, workspace_dev, workspace_bytes >= g.w.bytes, workspace_bytes, g.w.bytes, "%lld rows, %lld nodes, %lld directions and a node capacity of %lld", rows, nodes,
                                           num_directions, node_capacity);
    if (fits != GTSFM_OK) return fits;
    DeviceRunner run{(hipStream_t)stream_, me};
    return tr_inliers_stages(run, me, g, threshold, node_capacity, lds_node_limit, pair_weight_dev, meas_weight_dev, pair_inlier_dev, meas_inlier_dev, camera_inlier_dev,
                             position_dev, counts_dev);
}
