// View-graph estimation on the device: the rotation cycle-consistency filter and the largest connected component. See include/gtsfm_amd.h.
//
// A vertex is an image, an edge is a row (i1, i2, i2Ri1) of the two-view stage's arrays. Everything but the cycle angle is integer work,
// and every output byte is fixed by the SET of input edges and their rotations: not by the order of the rows, the grid, or timing.
//
// ADJACENCY: CSR with per-vertex sorted neighbour lists, each entry carrying the row of its edge. An N x N bit matrix would find the common
// neighbours of (a, b) by AND / popcount, but the cycle error needs the ROWS of (a, c) and (b, c) to fetch their rotations, which a bit does
// not give, and its size grows with the square of the image count where the pair graph of a scene is sparse (a retrieval window): CSR is
// 8 bytes per list entry whatever num_images is, and a merge of two sorted lists yields both rows of every common neighbour.
//   degree : per enabled edge, atomicAdd on both endpoints' degree (integer adds, any order); the edge's input flag (nine finite numbers).
//   scan   : exclusive prefix sum of the degrees (one workgroup).
//   fill   : an edge takes slot row_off[v] + atomicAdd(&cursor[v], 1) in both lists: arbitrary order, in bounds since exactly degree ask.
//   rank   : per list entry, over its vertex's list: rank = entries with a smaller (neighbour, row); the entry moves to that place of the
//            sorted list. Another entry with the same neighbour is a duplicate edge and raises a flag. Lists are short (the degree), so
//            this costs the sum of squared degrees and needs no sort.
//   The host reads the two flags (bad pair, duplicate) here, before any output is written.
//
// TRIPLETS. The slot of edge (a, b), a < b, in a's sorted list is its place in the lexicographic order of all edges. Per such slot:
//   count  : merge the lists of a and b; a common neighbour c whose two edges are input edges is a triplet. All of them, and those with
//            c > b (the triplet's lexicographically first edge owns it: each distinct triplet once, in lexicographic order).
//   scan   : both counts over the slots; the host reads the two totals (the second and last readback) and checks the capacities.
//   fill   : the same merge; the j-th common neighbour's cycle error goes to the edge's own segment, so the segment's order is that of c.
//            Each edge evaluates its triplets itself, on the SORTED triplet by one instruction sequence (vg_cycle_error_deg), so the three
//            edges of a triplet hold the same bytes and nothing is scattered.
//   aggregate : one wave per edge row; a lane takes the elements lane, lane + 64, ... of the segment and ranks each against the whole
//            segment by (value, index). The lane holding rank (n - 1) / 2 (or 0 for MIN) also finds its successor's value and writes the
//            aggregate: any count is handled by the same loop, no lane or wave capacity exists. A NaN in the segment gives NaN (numpy's
//            min and median) and the edge is dropped.
//
// COMPONENTS (gtsfm_largest_component): the union-find rounds of graph_prims.h over the images (uf_hook, uf_compress and uf_run_rounds;
// its header comment states the invariants). Then the size of every component at its root; the winner is the largest, of equally
// large ones the owner of the smallest enabled row.
// COUNTS are taken by one workgroup that walks the rows, not by atomics on one word.
//
// Every per-index step is a GTSFM_HD function, and each call is one function over a runner of stage_runner.h (vg_cycle_filter_stages,
// vg_largest_component_stages): the device call launches its stages, tools/view_graph_host_main.cpp walks the same stages in another
// order on a CPU, where the atomics become plain updates.

#include <math.h>

#include "../../include/gtsfm_amd.h"
#include "stage_runner.h"

#define VG_THREADS 256
#define VG_WAVE 64
#define VG_FLAG_WORDS UF_FLAG_WORDS  // word 0: a bad pair; word 1: a duplicate edge; word 8 + r: round r hooked something
#define VG_MAX_EDGES (1ll << 28)
#define VG_MAX_IMAGES (1ll << 28)
#define VG_MAX_TRIPLETS ((1ll << 31) / 3)
#define VG_RAD_TO_DEG 57.29577951308232  // 180 / pi, numpy's rad2deg factor

typedef unsigned long long vg_u64;

namespace {

// ---- the cycle error ----

// The angle in degrees of M = i2Ri0^T . i2Ri1 . i1Ri0 (products in that order, sums left to right), the way scipy's
// Rotation.from_matrix(M).as_rotvec() norm finds it: the quaternion from the largest of the diagonal and the trace (the first largest),
// normalised, then 2 atan2(|q_xyz|, |q_w|).
GTSFM_HD double vg_cycle_error_deg(const double* __restrict__ i1Ri0, const double* __restrict__ i2Ri1, const double* __restrict__ i2Ri0) {
    double a[9], m[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a[3 * r + c] = i2Ri0[r] * i2Ri1[c] + i2Ri0[3 + r] * i2Ri1[3 + c] + i2Ri0[6 + r] * i2Ri1[6 + c];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) m[3 * r + c] = a[3 * r] * i1Ri0[c] + a[3 * r + 1] * i1Ri0[3 + c] + a[3 * r + 2] * i1Ri0[6 + c];
    const double trace = m[0] + m[4] + m[8];
    int choice = 0;
    double best = m[0];
    if (m[4] > best) best = m[4], choice = 1;
    if (m[8] > best) best = m[8], choice = 2;
    if (trace > best) choice = 3;
    double qx, qy, qz, qw;  // scipy's (i, j, k) = (choice, choice + 1, choice + 2) mod 3, written out: no indexed registers
    if (choice == 0) {
        qx = 1 - trace + 2 * m[0], qy = m[3] + m[1], qz = m[6] + m[2], qw = m[7] - m[5];
    } else if (choice == 1) {
        qy = 1 - trace + 2 * m[4], qz = m[7] + m[5], qx = m[1] + m[3], qw = m[2] - m[6];
    } else if (choice == 2) {
        qz = 1 - trace + 2 * m[8], qx = m[2] + m[6], qy = m[5] + m[7], qw = m[3] - m[1];
    } else {
        qx = m[7] - m[5], qy = m[2] - m[6], qz = m[3] - m[1], qw = 1 + trace;
    }
    const double norm = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    qx /= norm, qy /= norm, qz /= norm, qw /= norm;
    const double angle = 2 * atan2(sqrt(qx * qx + qy * qy + qz * qz), fabs(qw));
    return angle * VG_RAD_TO_DEG;
}

// ---- the cycle filter ----

struct VgWorkspace {
    long long *row_off, *seg_off, *trip_off;  // [N + 1] degrees then list offsets; [2 E + 1] per slot: triplets, those it owns, then offsets
    int *cursor, *raw_nbr, *raw_edge, *adj_nbr, *adj_edge, *slot_of_edge, *flags;
    uint8_t* input;
    double* errs;  // [3 triplet_capacity] the per-edge error lists
    size_t fixed_bytes, bytes;
};

VgWorkspace vg_layout(void* base, long long num_edges, long long num_images, long long triplet_capacity) {
    VgWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t e = (size_t)num_edges, n = (size_t)num_images;
    w.row_off = (long long*)ws.take((n + 1) * 8);
    w.seg_off = (long long*)ws.take((2 * e + 1) * 8);
    w.trip_off = (long long*)ws.take((2 * e + 1) * 8);
    w.cursor = (int*)ws.take(n * 4);
    w.raw_nbr = (int*)ws.take(2 * e * 4);
    w.raw_edge = (int*)ws.take(2 * e * 4);
    w.adj_nbr = (int*)ws.take(2 * e * 4);
    w.adj_edge = (int*)ws.take(2 * e * 4);
    w.slot_of_edge = (int*)ws.take(e * 4);
    w.flags = (int*)ws.take(VG_FLAG_WORDS * 4);
    w.input = (uint8_t*)ws.take(e);
    w.fixed_bytes = ws.used;
    w.errs = (double*)ws.take(3 * (size_t)triplet_capacity * 8);
    w.bytes = ws.used;
    return w;
}

struct VgGraph {  // what the per-index functions of the filter read and write
    const int* pair_images;
    const double* rotation;
    const uint8_t* pair_enable;
    long long num_edges;
    int num_images;
    VgWorkspace w;
};

// an enabled row whose pair is in order and in range; every kernel tests it again, so a bad row is never followed anywhere
GTSFM_HD bool vg_edge_usable(const VgGraph& g, long long e, int* i1, int* i2) {
    if (g.pair_enable && !g.pair_enable[e]) return false;
    *i1 = g.pair_images[2 * e];
    *i2 = g.pair_images[2 * e + 1];
    return *i1 >= 0 && *i1 < *i2 && *i2 < g.num_images;
}

GTSFM_HD void vg_init(const VgGraph& g, long long i) {
    if (i < VG_FLAG_WORDS) g.w.flags[i] = 0;
    if (i <= g.num_images) g.w.row_off[i] = 0;
    if (i < g.num_images) g.w.cursor[i] = 0;
}

GTSFM_HD void vg_edge_degree(const VgGraph& g, long long e) {
    int i1, i2;
    g.w.input[e] = 0;
    if (!vg_edge_usable(g, e, &i1, &i2)) {
        if (!g.pair_enable || g.pair_enable[e]) g.w.flags[0] = 1;
        return;
    }
    hd_atomic_add(&g.w.row_off[i1], 1);
    hd_atomic_add(&g.w.row_off[i2], 1);
    bool finite = true;
    for (int k = 0; k < 9; ++k) finite = finite && isfinite(g.rotation[9 * e + k]);
    g.w.input[e] = finite ? 1 : 0;
}

GTSFM_HD void vg_edge_fill(const VgGraph& g, long long e) {
    int i1, i2;
    if (!vg_edge_usable(g, e, &i1, &i2)) return;
    const long long s1 = g.w.row_off[i1] + hd_atomic_add(&g.w.cursor[i1], 1), s2 = g.w.row_off[i2] + hd_atomic_add(&g.w.cursor[i2], 1);
    if (s1 < g.w.row_off[i1 + 1]) g.w.raw_nbr[s1] = i2, g.w.raw_edge[s1] = (int)e;  // always true: exactly degree rows ask
    if (s2 < g.w.row_off[i2 + 1]) g.w.raw_nbr[s2] = i1, g.w.raw_edge[s2] = (int)e;
}

// the vertex whose list holds an entry (neighbour, row): the row's other endpoint
GTSFM_HD int vg_owner(const VgGraph& g, int nbr, int edge) {
    const int i1 = g.pair_images[2 * (long long)edge], i2 = g.pair_images[2 * (long long)edge + 1];
    return i1 == nbr ? i2 : i1;
}

GTSFM_HD void vg_slot_rank(const VgGraph& g, long long s) {
    if (s >= g.w.row_off[g.num_images]) return;
    const int nbr = g.w.raw_nbr[s], edge = g.w.raw_edge[s], owner = vg_owner(g, nbr, edge);
    const long long lo = g.w.row_off[owner], hi = g.w.row_off[owner + 1];
    long long rank = 0;
    for (long long j = lo; j < hi; ++j) {
        const int nj = g.w.raw_nbr[j], ej = g.w.raw_edge[j];
        if (nj < nbr || (nj == nbr && ej < edge)) ++rank;
        if (nj == nbr && ej != edge) g.w.flags[1] = 1;
    }
    g.w.adj_nbr[lo + rank] = nbr;
    g.w.adj_edge[lo + rank] = edge;
    if (owner < nbr) g.w.slot_of_edge[edge] = (int)(lo + rank);
}

// The triplets of sorted slot s = edge (a, b) with a < b, by a merge of the two sorted lists. fill == false: seg_off[s] / trip_off[s]
// receive the counts (all, and those with c > b). fill == true (after the scans): the errors go to the edge's segment, and the triplets
// this edge owns to the triplet list.
GTSFM_HD void vg_slot_triplets(const VgGraph& g, long long s, bool fill, int* __restrict__ triplets, double* __restrict__ cycle_error) {
    long long all = 0, own = 0;
    if (s < g.w.row_off[g.num_images]) {
        const int b = g.w.adj_nbr[s], e = g.w.adj_edge[s], a = vg_owner(g, b, e);
        if (a < b && g.w.input[e]) {
            long long pa = g.w.row_off[a], pb = g.w.row_off[b];
            const long long ea = g.w.row_off[a + 1], eb = g.w.row_off[b + 1];
            const long long seg = fill ? g.w.seg_off[s] : 0, trip = fill ? g.w.trip_off[s] : 0;
            while (pa < ea && pb < eb) {
                const int ca = g.w.adj_nbr[pa], cb = g.w.adj_nbr[pb];
                if (ca < cb) {
                    ++pa;
                } else if (cb < ca) {
                    ++pb;
                } else {
                    const int eac = g.w.adj_edge[pa], ebc = g.w.adj_edge[pb];
                    if (g.w.input[eac] && g.w.input[ebc]) {
                        const int c = ca;
                        if (fill) {
                            const double *rab = g.rotation + 9 * (long long)e, *rac = g.rotation + 9 * (long long)eac, *rbc = g.rotation + 9 * (long long)ebc;
                            // (i1Ri0, i2Ri1, i2Ri0) of the sorted triplet
                            const double err = c < a ? vg_cycle_error_deg(rac, rab, rbc) : (c < b ? vg_cycle_error_deg(rac, rbc, rab) : vg_cycle_error_deg(rab, rbc, rac));
                            g.w.errs[seg + all] = err;
                            if (c > b && triplets) {
                                triplets[3 * (trip + own)] = a, triplets[3 * (trip + own) + 1] = b, triplets[3 * (trip + own) + 2] = c;
                                cycle_error[trip + own] = err;
                            }
                        }
                        ++all;
                        if (c > b) ++own;
                    }
                    ++pa, ++pb;
                }
            }
        }
    }
    if (!fill) g.w.seg_off[s] = all, g.w.trip_off[s] = own;
}

// Lane `lane` of `lanes` for edge row e: see the header comment.
GTSFM_HD void vg_edge_aggregate(const VgGraph& g, long long e, int lane, int lanes, int criterion, double threshold, int* __restrict__ num_triplets,
                             double* __restrict__ aggregate, uint8_t* __restrict__ keep) {
    const double nan = __builtin_nan("");
    if (!g.w.input[e]) {
        if (lane == 0) num_triplets[e] = 0, aggregate[e] = nan, keep[e] = 0;
        return;
    }
    const long long s = g.w.slot_of_edge[e], base = g.w.seg_off[s], n = g.w.seg_off[s + 1] - base;
    if (n == 0) {
        if (lane == 0) num_triplets[e] = 0, aggregate[e] = nan, keep[e] = 1;
        return;
    }
    const bool median = criterion == 1;
    const long long k = median ? (n - 1) / 2 : 0;
    const bool two = median && n % 2 == 0;
    const double* x = g.w.errs + base;
    for (long long j = lane; j < n; j += lanes) {
        const double xj = x[j];
        long long rank = 0;
        bool has_nan = false;
        double succ = HUGE_VAL;
        for (long long i = 0; i < n; ++i) {
            const double xi = x[i];
            has_nan = has_nan || xi != xi;
            if (xi < xj || (xi == xj && i < j)) ++rank;
            if ((xi > xj || (xi == xj && i > j)) && xi < succ) succ = xi;
        }
        if (has_nan ? j != 0 : rank != k) continue;
        const double value = has_nan ? nan : (two ? (xj + succ) / 2 : xj);
        const bool kept = value < threshold;
        num_triplets[e] = (int)n, aggregate[e] = value, keep[e] = kept ? 1 : 0;
    }
}

// ---- the largest component ----

struct VgComponents {
    const int* pair_images;
    const uint8_t* pair_enable;
    long long num_edges;
    int num_images;
    int *parent, *label, *mark, *cnt, *flags;
    vg_u64* best;  // (size << 32) | (INT_MAX - smallest enabled row) of the winning component; 0: no enabled edge
    size_t bytes;
};

VgComponents vg_cc_layout(void* base, long long num_images) {
    VgComponents w;
    WorkspaceCarver ws{base, 0};
    const size_t n = (size_t)num_images;
    w.parent = (int*)ws.take(n * 4);
    w.label = (int*)ws.take(n * 4);
    w.mark = (int*)ws.take(n * 4);
    w.cnt = (int*)ws.take(n * 4);
    w.flags = (int*)ws.take(VG_FLAG_WORDS * 4);
    w.best = (vg_u64*)ws.take(8);
    w.bytes = ws.used;
    return w;
}

GTSFM_HD bool vg_cc_edge(const VgComponents& g, long long e, int* i1, int* i2) {
    if (g.pair_enable && !g.pair_enable[e]) return false;
    *i1 = g.pair_images[2 * e];
    *i2 = g.pair_images[2 * e + 1];
    return *i1 >= 0 && *i1 < g.num_images && *i2 >= 0 && *i2 < g.num_images;
}

GTSFM_HD void vg_cc_init(const VgComponents& g, long long v) {
    if (v < VG_FLAG_WORDS) g.flags[v] = 0;
    if (v == 0) *g.best = 0;
    if (v >= g.num_images) return;
    g.parent[v] = g.label[v] = (int)v;
    g.mark[v] = g.cnt[v] = 0;
}

GTSFM_HD void vg_cc_hook(const VgComponents& g, long long e, int round) {
    int u, v;
    if (!vg_cc_edge(g, e, &u, &v)) {
        if (!g.pair_enable || g.pair_enable[e]) g.flags[0] = 1;
        return;
    }
    uf_hook(g.parent, g.label, g.mark, g.flags, u, v, round);
}

GTSFM_HD void vg_cc_node_count(const VgComponents& g, long long v) {
    if (g.mark[v]) hd_atomic_add(&g.cnt[g.label[v]], 1);
}

// The winner is the largest component, and of equally large ones the one that owns the first edge listed: an enabled row bids when its
// component has the largest size, INT_MAX - row, and the largest bid wins. (A per-root minimum row by atomicMin would put every edge of a
// connected scene on one word: measured 0.5 ms at 43 867 edges.)
GTSFM_HD vg_u64 vg_cc_edge_bid(const VgComponents& g, long long e, int largest) {
    int u, v;
    return vg_cc_edge(g, e, &u, &v) && g.cnt[g.label[u]] == largest ? (vg_u64)(0x7FFFFFFF - e) : 0;
}

// the winner's label, or -1 without an enabled edge
GTSFM_HD int vg_cc_root_of_key(const VgComponents& g, vg_u64 best) {
    if (best == 0) return -1;
    const long long row = 0x7FFFFFFF - (long long)(unsigned)(best & 0xFFFFFFFFull);
    return g.label[g.pair_images[2 * row]];
}

GTSFM_HD bool vg_cc_edge_kept(const VgComponents& g, long long e, int root) {
    int u, v;
    return root >= 0 && vg_cc_edge(g, e, &u, &v) && g.label[u] == root;
}

GTSFM_HD void vg_cc_write_node(const VgComponents& g, long long v, uint8_t* __restrict__ node_mask) {
    const int root = vg_cc_root_of_key(g, *g.best);
    node_mask[v] = (root >= 0 && g.mark[v] && g.label[v] == root) ? 1 : 0;
}

GTSFM_HD void vg_cc_write_edge(const VgComponents& g, long long e, uint8_t* __restrict__ pair_keep) {
    pair_keep[e] = vg_cc_edge_kept(g, e, vg_cc_root_of_key(g, *g.best)) ? 1 : 0;
}

// ---- the counts: ONE workgroup walks the rows and combines by a tree. Tens of thousands of atomics on one word would serialise (measured:
// 11 ns each, 1.6 ms of the aggregate kernel's 1.65 ms at 48 725 edges); a walk of the same rows by 1024 lanes does not.

__global__ __launch_bounds__(SCAN_THREADS) void vg_filter_counts_kernel(const uint8_t* __restrict__ input, const uint8_t* __restrict__ keep,
                                                                          const int* __restrict__ num_triplets, long long num_edges, long long total_triplets,
                                                                          int* __restrict__ counts) {
    __shared__ long long lds[SCAN_THREADS];
    long long in = 0, kept = 0, most = 0;
    for (long long e = threadIdx.x; e < num_edges; e += SCAN_THREADS) {
        in += input[e] ? 1 : 0;
        kept += keep[e] ? 1 : 0;
        most = num_triplets[e] > most ? num_triplets[e] : most;
    }
    const auto add = [](long long a, long long b) { return a + b; };
    in = block_reduce<SCAN_THREADS>(in, lds, add);
    kept = block_reduce<SCAN_THREADS>(kept, lds, add);
    most = block_reduce<SCAN_THREADS>(most, lds, [](long long a, long long b) { return a > b ? a : b; });
    if (threadIdx.x == 0) {
        counts[0] = (int)in, counts[1] = (int)kept, counts[2] = (int)total_triplets, counts[3] = (int)most;
        counts[4] = counts[5] = counts[6] = counts[7] = 0;
    }
}
// its stand-in on a CPU
void vg_filter_counts_host(const HostRunner& run, const uint8_t* input, const uint8_t* keep, const int* num_triplets, long long num_edges, long long total_triplets,
                           int* counts) {
    long long in = 0, kept = 0, most = 0;
    run.walk(num_edges, [&](long long e) {
        in += input[e] ? 1 : 0;
        kept += keep[e] ? 1 : 0;
        most = num_triplets[e] > most ? num_triplets[e] : most;
    });
    memset(counts, 0, 8 * sizeof(int));
    counts[0] = (int)in, counts[1] = (int)kept, counts[2] = (int)total_triplets, counts[3] = (int)most;
}

// the largest size and the roots over the nodes, the winning bid over the rows (stored with the size in *g.best for the two write
// kernels), then the component's edges
__global__ __launch_bounds__(SCAN_THREADS) void vg_cc_summary_kernel(VgComponents g, int* __restrict__ counts) {
    __shared__ vg_u64 lds[SCAN_THREADS];
    vg_u64 largest = 0, components = 0, bid = 0, edges = 0;
    for (long long v = threadIdx.x; v < g.num_images; v += SCAN_THREADS) {
        const vg_u64 size = g.cnt[v] > 0 ? (vg_u64)g.cnt[v] : 0;  // cnt is nonzero at the roots of components with an edge only
        components += size ? 1 : 0;
        largest = size > largest ? size : largest;
    }
    const auto add = [](vg_u64 a, vg_u64 b) { return a + b; };
    const auto most = [](vg_u64 a, vg_u64 b) { return a > b ? a : b; };
    largest = block_reduce<SCAN_THREADS>(largest, lds, most);
    components = block_reduce<SCAN_THREADS>(components, lds, add);
    for (long long e = threadIdx.x; e < g.num_edges && largest; e += SCAN_THREADS) {
        const vg_u64 b = vg_cc_edge_bid(g, e, (int)largest);
        bid = b > bid ? b : bid;
    }
    bid = block_reduce<SCAN_THREADS>(bid, lds, most);
    const vg_u64 best = largest ? (largest << 32) | bid : 0;
    const int root = vg_cc_root_of_key(g, best);
    for (long long e = threadIdx.x; e < g.num_edges; e += SCAN_THREADS) edges += vg_cc_edge_kept(g, e, root) ? 1 : 0;
    edges = block_reduce<SCAN_THREADS>(edges, lds, add);
    if (threadIdx.x == 0) {
        *g.best = best;
        counts[0] = (int)(best >> 32), counts[1] = (int)edges, counts[2] = (int)components;
        counts[3] = counts[4] = counts[5] = counts[6] = counts[7] = 0;
    }
}
// its stand-in on a CPU
void vg_cc_summary_host(const HostRunner& run, const VgComponents& g, int* counts) {
    vg_u64 largest = 0, components = 0, bid = 0, edges = 0;
    run.walk(g.num_images, [&](long long v) {
        const vg_u64 size = g.cnt[v] > 0 ? (vg_u64)g.cnt[v] : 0;
        components += size ? 1 : 0;
        largest = size > largest ? size : largest;
    });
    if (largest) run.walk(g.num_edges, [&](long long e) {
        const vg_u64 b = vg_cc_edge_bid(g, e, (int)largest);
        bid = b > bid ? b : bid;
    });
    const vg_u64 best = largest ? (largest << 32) | bid : 0;
    const int root = vg_cc_root_of_key(g, best);
    run.walk(g.num_edges, [&](long long e) { edges += vg_cc_edge_kept(g, e, root) ? 1 : 0; });
    *g.best = best;
    memset(counts, 0, 8 * sizeof(int));
    counts[0] = (int)(best >> 32), counts[1] = (int)edges, counts[2] = (int)components;
}

// ---- the two pipelines: every stage once, for the device call and for tools/view_graph_host_main.cpp (stage_runner.h) ----

// g.w is laid out for triplet_capacity triplets. With more triplets than that, *num_triplets_host tells how many and nothing is written.
template <class Runner>
int vg_cycle_filter_stages(Runner& run, const char* me, const VgGraph& g, int criterion, double error_threshold, long long triplet_capacity, int* num_triplets,
                           double* aggregate_error, uint8_t* keep, int* counts, int* triplets, double* cycle_error, long long* num_triplets_host) {
    const long long E = g.num_edges, slots = 2 * E;
    if (E == 0) {
        if (run.zero(counts, 8 * sizeof(int)) == GTSFM_OK && num_triplets_host) *num_triplets_host = 0;
        return run.status;
    }
    const long long init_n = (long long)g.num_images + 1 > VG_FLAG_WORDS ? (long long)g.num_images + 1 : VG_FLAG_WORDS;
    run.template each<struct vg_init_stage>(init_n, STAGE_FN(long long i) { vg_init(g, i); });
    run.template each<struct vg_edge_degree_stage>(E, STAGE_FN(long long i) { vg_edge_degree(g, i); });
    run.scan(g.w.row_off, g.num_images);
    run.template each<struct vg_edge_fill_stage>(E, STAGE_FN(long long i) { vg_edge_fill(g, i); });
    run.template each<struct vg_slot_rank_stage>(slots, STAGE_FN(long long i) { vg_slot_rank(g, i); });
    int flags[2] = {0, 0};
    if (run.fetch(flags, g.w.flags, 2, "building the adjacency") != GTSFM_OK) return run.status;
    GTSFM_CHECK_ARG(!flags[0], "%s: an enabled edge has i1 >= i2 or names an image outside 0 .. %d; nothing was written", me, g.num_images - 1);
    GTSFM_CHECK_ARG(!flags[1], "%s: an enabled edge is listed twice; nothing was written", me);

    const auto slot_triplets = [&](bool fill, int* triplets_out, double* cycle_error_out) {  // one kernel, launched to count and then to fill
        run.template each<struct vg_slot_triplets_stage>(slots, STAGE_FN(long long i) { vg_slot_triplets(g, i, fill, triplets_out, cycle_error_out); });
    };
    slot_triplets(false, nullptr, nullptr);
    run.scan(g.w.seg_off, slots);
    run.scan(g.w.trip_off, slots);
    long long entries = -1, total = -1;  // entries of the per-edge lists, distinct triplets
    run.copy(&entries, g.w.seg_off + slots, 1, "counting the triplets");
    if (run.fetch(&total, g.w.trip_off + slots, 1, "counting the triplets") != GTSFM_OK) return run.status;
    GTSFM_CHECK_ARG(total >= 0 && entries == 3 * total, "%s: %lld list entries for %lld triplets; nothing was written", me, entries, total);
    if (num_triplets_host) *num_triplets_host = total;
    if (total > triplet_capacity) {
        gtsfm_set_error("%s: %lld triplets, capacity (workspace and triplet outputs) for %lld; nothing was written", me, total, triplet_capacity);
        return GTSFM_ERR_WORKSPACE;
    }

    slot_triplets(true, triplets, cycle_error);
    run.template group<struct vg_edge_aggregate_stage, VG_THREADS, VG_WAVE>(E, STAGE_FN(long long e, int lane, int lanes) {
        vg_edge_aggregate(g, e, lane, lanes, criterion, error_threshold, num_triplets, aggregate_error, keep);
    });
    return run.block(
        "vg_filter_counts_kernel",
        [&](hipStream_t stream) { hipLaunchKernelGGL(vg_filter_counts_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, g.w.input, keep, num_triplets, E, total, counts); },
        [&](const HostRunner& host) { vg_filter_counts_host(host, g.w.input, keep, num_triplets, E, total, counts); });
}

template <class Runner>
int vg_largest_component_stages(Runner& run, const char* me, const VgComponents& g, uint8_t* node_mask, uint8_t* pair_keep, int* counts) {
    const long long E = g.num_edges, N = g.num_images;
    run.template each<struct vg_cc_init_stage>(N > VG_FLAG_WORDS ? N : VG_FLAG_WORDS, STAGE_FN(long long i) { vg_cc_init(g, i); });
    if (E > 0) {
        int rounds = 0;
        const UfOutcome labelled = uf_run_rounds(
            run, g.flags, [&](int round) { return run.template each<struct vg_cc_hook_stage>(E, STAGE_FN(long long i) { vg_cc_hook(g, i, round); }); },
            [&] { return run.template each<struct vg_cc_compress_stage>(N, STAGE_FN(long long i) { uf_compress(g.parent, g.label, i); }); }, &rounds);
        if (labelled == UF_FAILED) return run.status;
        GTSFM_CHECK_ARG(labelled != UF_NO_FIXED_POINT, "%s: no fixed point after %d rounds (%d images, %lld edges); nothing was written", me, rounds, g.num_images, E);
        GTSFM_CHECK_ARG(labelled != UF_BAD_INPUT, "%s: an enabled edge names an image outside 0 .. %d; nothing was written", me, g.num_images - 1);
        run.template each<struct vg_cc_node_count_stage>(N, STAGE_FN(long long i) { vg_cc_node_count(g, i); });
    }
    run.block(
        "vg_cc_summary_kernel", [&](hipStream_t stream) { hipLaunchKernelGGL(vg_cc_summary_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, g, counts); },
        [&](const HostRunner& host) { vg_cc_summary_host(host, g, counts); });
    run.template each<struct vg_cc_write_node_stage>(N, STAGE_FN(long long i) { vg_cc_write_node(g, i, node_mask); });
    if (E > 0) run.template each<struct vg_cc_write_edge_stage>(E, STAGE_FN(long long i) { vg_cc_write_edge(g, i, pair_keep); });
    return run.status;
}

}  // namespace

extern "C" size_t gtsfm_view_graph_workspace_bytes(long long num_edges, long long num_images, long long triplet_capacity) {
    if (num_edges < 0 || num_images < 0 || triplet_capacity < 0 || num_edges >= VG_MAX_EDGES || num_images >= VG_MAX_IMAGES || triplet_capacity >= VG_MAX_TRIPLETS)
        return 0;
    const size_t filter = vg_layout(nullptr, num_edges, num_images, triplet_capacity).bytes, components = vg_cc_layout(nullptr, num_images).bytes;
    return filter > components ? filter : components;
}

extern "C" int gtsfm_view_graph_cycle_filter_f64(const int32_t* pair_images_dev, const double* rotation_dev, const uint8_t* pair_enable_dev, long long num_edges,
                                                 int num_images, int criterion, double error_threshold, long long triplet_capacity, void* workspace_dev,
                                                 size_t workspace_bytes, int32_t* num_triplets_dev, double* aggregate_error_dev, uint8_t* keep_dev,
                                                 int32_t* counts_dev, int32_t* triplets_dev, double* cycle_error_dev, long long* num_triplets_host, void* stream_) {
    const char* me = "gtsfm_view_graph_cycle_filter_f64";
    if (num_triplets_host) *num_triplets_host = -1;
    GTSFM_CHECK_ARG(num_edges >= 0 && num_edges < VG_MAX_EDGES && num_images >= 0 && num_images < VG_MAX_IMAGES && triplet_capacity >= 0 && triplet_capacity < VG_MAX_TRIPLETS,
                    "%s: sizes out of range (%lld edges, %d images, %lld triplets)", me, num_edges, num_images, triplet_capacity);
    GTSFM_CHECK_ARG(criterion == 0 || criterion == 1, "%s: criterion %d is neither MIN_EDGE_ERROR (0) nor MEDIAN_EDGE_ERROR (1)", me, criterion);
    GTSFM_CHECK_ARG(counts_dev, "%s: null counts_dev", me);
    GTSFM_CHECK_ARG((triplets_dev == nullptr) == (cycle_error_dev == nullptr), "%s: triplets_dev and cycle_error_dev come together", me);
    VgGraph g{pair_images_dev, rotation_dev, pair_enable_dev, num_edges, num_images, vg_layout(workspace_dev, num_edges, num_images, triplet_capacity)};
    if (num_edges > 0) {  // without an edge the stages touch the counts only
        GTSFM_CHECK_ARG(pair_images_dev && rotation_dev && workspace_dev && num_triplets_dev && aggregate_error_dev && keep_dev, "%s: null pointer", me);
        const int fits = gtsfm_check_workspace(me, workspace_dev, workspace_bytes >= g.w.bytes, workspace_bytes, g.w.bytes, "%lld edges, %d images and %lld triplets", num_edges, num_images, triplet_capacity);
        if (fits != GTSFM_OK) return fits;
    }
    DeviceRunner run{(hipStream_t)stream_, me};
    return vg_cycle_filter_stages(run, me, g, criterion, error_threshold, triplet_capacity, num_triplets_dev, aggregate_error_dev, keep_dev, counts_dev, triplets_dev,
                                  cycle_error_dev, num_triplets_host);
}

extern "C" int gtsfm_largest_component(const int32_t* pair_images_dev, const uint8_t* pair_enable_dev, long long num_edges, int num_images, void* workspace_dev,
                                       size_t workspace_bytes, uint8_t* node_mask_dev, uint8_t* pair_keep_dev, int32_t* counts_dev, void* stream_) {
    const char* me = "gtsfm_largest_component";
    GTSFM_CHECK_ARG(num_edges >= 0 && num_edges < VG_MAX_EDGES && num_images >= 0 && num_images < VG_MAX_IMAGES, "%s: sizes out of range (%lld edges, %d images)", me,
                    num_edges, num_images);
    GTSFM_CHECK_ARG(counts_dev && (num_images == 0 || node_mask_dev) && (num_edges == 0 || (pair_images_dev && pair_keep_dev)), "%s: null pointer", me);
    VgComponents g = vg_cc_layout(workspace_dev, num_images);
    g.pair_images = pair_images_dev, g.pair_enable = pair_enable_dev, g.num_edges = num_edges, g.num_images = num_images;
    const int fits = gtsfm_check_workspace(me, workspace_dev, workspace_bytes >= g.bytes, workspace_bytes, g.bytes, "%d images", num_images);
    if (fits != GTSFM_OK) return fits;
    DeviceRunner run{(hipStream_t)stream_, me};
    return vg_largest_component_stages(run, me, g, node_mask_dev, pair_keep_dev, counts_dev);
}
