// The scaffold of the one-workgroup-per-problem solvers (rotation averaging, translation recovery): the host/device lane model, the scan and
// the tree, the adjacency lists and the anchor's component, the trust region's scalar rules and the launch shell. Internal linkage, like
// graph_prims.h: each translation unit keeps its own instantiation.
//
// THE LANE MODEL. A solver is ONE function for the device and the host: a section between SOLVER_PAR_BEGIN and SOLVER_PAR_END is run by
// every lane and ends with a barrier; on the host (tools/*_host_main.cpp) it is a loop over the lanes, in either order and with any lane
// count (solver_host), and the atomics are plain updates. Scalars that steer the control flow are read from memory after a barrier, inside
// a section: they are uniform, so every branch around a barrier is on a uniform value and every barrier is matched. Every loop has a cap
// that is an argument or a size; no loop waits on a value another lane may never write.
#pragma once

#include <math.h>

#include "graph_prims.h"

#define SOLVER_THREADS 256
#define SOLVER_FLAG_WORDS 8  // 0 and 1: the stage's two refusals, raised by its validate kernel
#define SOLVER_RHO_REG (1e3 * 2.220446049250313e-16)
#define SOLVER_ACCEPT_RHO 0.1

enum SolverStatus { SOLVER_CONVERGED = 0, SOLVER_MAX_ITERATIONS = 1, SOLVER_NO_VALID_ROW = 2, SOLVER_NON_FINITE = 3 };

struct SolverHostLanes {  // the host builds' lane count and order (the device pass only parses the tools that set it)
    int lanes, descending;
};
__attribute__((unused)) static SolverHostLanes solver_host = {1, 0};

#if defined(__HIP_DEVICE_COMPILE__)
#define SOLVER_PAR_BEGIN                  \
    {                                     \
        const int lane = threadIdx.x;     \
        const int lanes = SOLVER_THREADS; \
        (void)lane, (void)lanes;
#define SOLVER_PAR_END \
    }                  \
    __syncthreads();
#else
#define SOLVER_PAR_BEGIN                                                           \
    for (int solver_l = 0; solver_l < solver_host.lanes; ++solver_l) {             \
        const int lanes = solver_host.lanes;                                       \
        const int lane = solver_host.descending ? lanes - 1 - solver_l : solver_l; \
        (void)lane, (void)lanes;
#define SOLVER_PAR_END }
#endif

namespace {

// The graph of one problem over `nodes` node ids and its rows; carved for every problem at once, then sliced.
struct SolverGraph {
    int *off, *cid;                                // [P][nodes + 2]: list offsets by node; compact ids (an exclusive scan of the reach flags)
    int *cursor, *reach, *cnode;                   // [P][nodes]
    long long* lanebuf;                            // [P][SOLVER_THREADS]
    int *raw_row, *raw_owner, *adj_nbr, *adj_row;  // [2 rows]; a problem's slice starts at twice its first row
    double* t;                                     // the tree: the caller's, p2 doubles
    int n, p2, anchor_c;                           // the component's nodes, padded to a power of two; the anchor's compact id
};

SolverGraph solver_carve(WorkspaceCarver& ws, size_t rows, size_t nodes, size_t problems) {
    SolverGraph g{};
    g.off = (int*)ws.take(problems * (nodes + 2) * 4);
    g.cid = (int*)ws.take(problems * (nodes + 2) * 4);
    g.cursor = (int*)ws.take(problems * nodes * 4);
    g.reach = (int*)ws.take(problems * nodes * 4);
    g.cnode = (int*)ws.take(problems * nodes * 4);
    g.lanebuf = (long long*)ws.take(problems * SOLVER_THREADS * 8);
    g.raw_row = (int*)ws.take(2 * rows * 4);
    g.raw_owner = (int*)ws.take(2 * rows * 4);
    g.adj_nbr = (int*)ws.take(2 * rows * 4);
    g.adj_row = (int*)ws.take(2 * rows * 4);
    return g;
}

// problem p's part of `all`; first_row: the rows of the problems before it
GTSFM_HD SolverGraph solver_slice(const SolverGraph& all, int p, int nodes, size_t first_row) {
    SolverGraph g = all;
    const size_t sp = (size_t)p, sn = (size_t)nodes;
    g.off += sp * (sn + 2), g.cid += sp * (sn + 2), g.cursor += sp * sn, g.reach += sp * sn, g.cnode += sp * sn, g.lanebuf += sp * SOLVER_THREADS;
    g.raw_row += 2 * first_row, g.raw_owner += 2 * first_row, g.adj_nbr += 2 * first_row, g.adj_row += 2 * first_row;
    return g;
}

// ---- the scan and the tree ----

// val[0 .. n) -> its exclusive prefix sum in place, val[n] = the total: every lane a contiguous chunk
GTSFM_HD void solver_scan(int* val, int n, long long* lanebuf) {
    SOLVER_PAR_BEGIN
    const int chunk = (n + lanes - 1) / lanes, from = lane * chunk < n ? lane * chunk : n, to = from + chunk < n ? from + chunk : n;
    long long s = 0;
    for (int i = from; i < to; ++i) s += val[i];
    lanebuf[lane] = s;
    SOLVER_PAR_END
    SOLVER_PAR_BEGIN
    const int chunk = (n + lanes - 1) / lanes, from = lane * chunk < n ? lane * chunk : n, to = from + chunk < n ? from + chunk : n;
    long long run = 0;
    for (int l = 0; l < lane; ++l) run += lanebuf[l];
    for (int i = from; i < to; ++i) {
        const int x = val[i];
        val[i] = (int)run;
        run += x;
    }
    if (lane == lanes - 1) {  // the last lane's chunk may be empty; the lanes before it hold everything
        val[n] = (int)run;
    }
    SOLVER_PAR_END
}

// the tree over t[0 .. p2): t[i] = t[i] (+ or max) t[i + s] level by level; the result is uniform
GTSFM_HD double solver_tree(double* t, int p2, bool take_max) {
    for (long long s = 1; s < p2; s <<= 1) {
        SOLVER_PAR_BEGIN
        for (long long i = (long long)lane * 2 * s; i < p2; i += (long long)lanes * 2 * s) {
            const double x = t[i], y = t[i + s];
            t[i] = take_max ? (x > y ? x : y) : x + y;
        }
        SOLVER_PAR_END
    }
    double out = 0.0;
    SOLVER_PAR_BEGIN
    out = t[0];
    SOLVER_PAR_END
    return out;
}
// inside the section that fills t[0 .. n): zeros up to the power of two
GTSFM_HD void solver_tree_pad(const SolverGraph& g, int lane, int lanes) {
    for (int c = g.n + lane; c < g.p2; c += lanes) g.t[c] = 0.0;
}

// a dot product as a left-to-right chain: ((a0 b0 + a1 b1) + a2 b2) + ...
GTSFM_HD double solver_dot(const double* a, const double* b, int k) {
    double s = a[0] * b[0];
    for (int i = 1; i < k; ++i) s = s + a[i] * b[i];
    return s;
}
// <x, y> over the component's nodes, k numbers per node
GTSFM_HD double solver_dot_nodes(const SolverGraph& g, const double* x, const double* y, int k) {
    SOLVER_PAR_BEGIN
    for (int c = lane; c < g.n; c += lanes) g.t[c] = solver_dot(x + k * (size_t)c, y + k * (size_t)c, k);
    solver_tree_pad(g, lane, lanes);
    SOLVER_PAR_END
    return solver_tree(g.t, g.p2, false);
}
// |x|_inf over the component's nodes, k numbers per node
GTSFM_HD double solver_inf_norm(const SolverGraph& g, const double* x, int k) {
    SOLVER_PAR_BEGIN
    for (int c = lane; c < g.n; c += lanes) {
        const double* v = x + k * (size_t)c;
        double m = fabs(v[0]);
        for (int i = 1; i < k; ++i) m = m > fabs(v[i]) ? m : fabs(v[i]);
        g.t[c] = m;
    }
    solver_tree_pad(g, lane, lanes);
    SOLVER_PAR_END
    return solver_tree(g.t, g.p2, true);
}

// ---- the lists and the component ----

// inside the caller's first section: the graph's counters to zero
GTSFM_HD void solver_clear(const SolverGraph& g, int nodes, int lane, int lanes) {
    for (int i = lane; i < nodes + 2; i += lanes) g.off[i] = 0, g.cid[i] = 0;
    for (int i = lane; i < nodes; i += lanes) g.cursor[i] = 0, g.reach[i] = 0;
}

// The adjacency lists of rows 0 .. rows - 1, after solver_clear and a barrier. ends(row, &a, &b) gives a row's two nodes, valid(row) says
// whether it counts. Degrees by integer atomics, the scan, an arbitrary slot per entry (atomic cursor), then every entry is ranked within
// its node's list by (neighbour, row) and moved to its place: adj_nbr is the neighbour, adj_row is 2 * row + (the list's node is the
// row's a). Returns the first valid row, `rows` when there is none (then no list is built); *entries: twice the valid rows.
template <class Ends, class Valid>
GTSFM_HD int solver_build_lists(const SolverGraph& g, int nodes, int rows, Ends ends, Valid valid, int* entries) {
    SOLVER_PAR_BEGIN
    long long first = rows;
    for (int l = lane; l < rows; l += lanes) {
        if (!valid(l)) continue;
        int na, nb;
        ends(l, &na, &nb);
        hd_atomic_add(&g.off[na], 1);
        hd_atomic_add(&g.off[nb], 1);
        if (l < first) first = l;
    }
    g.lanebuf[lane] = first;
    SOLVER_PAR_END
    long long first = rows;
    SOLVER_PAR_BEGIN
    first = rows;
    for (int l = 0; l < lanes; ++l) first = g.lanebuf[l] < first ? g.lanebuf[l] : first;
    SOLVER_PAR_END
    solver_scan(g.off, nodes, g.lanebuf);
    int total = 0;
    SOLVER_PAR_BEGIN
    total = g.off[nodes];
    SOLVER_PAR_END
    *entries = total;
    if (first >= rows) return rows;
    SOLVER_PAR_BEGIN
    for (int l = lane; l < rows; l += lanes) {
        if (!valid(l)) continue;
        int na, nb;
        ends(l, &na, &nb);
        const int s1 = g.off[na] + hd_atomic_add(&g.cursor[na], 1), s2 = g.off[nb] + hd_atomic_add(&g.cursor[nb], 1);
        if (s1 < g.off[na + 1]) g.raw_row[s1] = l, g.raw_owner[s1] = na;  // always true: exactly degree rows ask
        if (s2 < g.off[nb + 1]) g.raw_row[s2] = l, g.raw_owner[s2] = nb;
    }
    SOLVER_PAR_END
    SOLVER_PAR_BEGIN
    for (int s = lane; s < total; s += lanes) {
        const int row = g.raw_row[s], owner = g.raw_owner[s];
        int na, nb;
        ends(row, &na, &nb);
        const int nbr = owner == na ? nb : na;
        int rank = 0;
        for (int j = g.off[owner]; j < g.off[owner + 1]; ++j) {
            const int rj = g.raw_row[j];
            int ja, jb;
            ends(rj, &ja, &jb);
            const int nj = owner == ja ? jb : ja;
            if (nj < nbr || (nj == nbr && rj < row)) ++rank;
        }
        g.adj_nbr[g.off[owner] + rank] = nbr;
        g.adj_row[g.off[owner] + rank] = 2 * row + (owner == na ? 1 : 0);
    }
    SOLVER_PAR_END
    return (int)first;
}

// The anchor's component: n, p2, anchor_c, cnode (its nodes in ascending id), cid (a node's compact id), and adj_nbr renumbered to compact
// ids in the component's lists. The lanes read reach[] of their neighbours while other lanes set it in the same section: a race that is
// MEANT. reach[] only ever goes from 0 to 1 (a 4-byte store), a lane that misses a fresh 1 sees it in the next round, and the fixed point
// -- the component -- is unique; only the number of rounds depends on the timing, and no output holds it. The loop ends after a round
// without a change, at most `nodes` rounds.
GTSFM_HD void solver_component(SolverGraph& g, int anchor, int nodes) {
    SOLVER_PAR_BEGIN
    if (lane == 0) g.reach[anchor] = 1;
    SOLVER_PAR_END
    for (int round = 0; round < nodes; ++round) {
        SOLVER_PAR_BEGIN
        long long changed = 0;
        for (int node = lane; node < nodes; node += lanes) {
            if (g.reach[node]) continue;
            for (int j = g.off[node]; j < g.off[node + 1]; ++j) {
                if (g.reach[g.adj_nbr[j]]) {
                    g.reach[node] = 1, changed = 1;
                    break;
                }
            }
        }
        g.lanebuf[lane] = changed;
        SOLVER_PAR_END
        long long any = 0;
        SOLVER_PAR_BEGIN
        any = 0;
        for (int l = 0; l < lanes; ++l) any |= g.lanebuf[l];
        SOLVER_PAR_END
        if (!any) break;
    }
    SOLVER_PAR_BEGIN
    for (int i = lane; i < nodes; i += lanes) g.cid[i] = g.reach[i];
    SOLVER_PAR_END
    solver_scan(g.cid, nodes, g.lanebuf);
    SOLVER_PAR_BEGIN
    for (int i = lane; i < nodes; i += lanes)
        if (g.reach[i]) g.cnode[g.cid[i]] = i;
    SOLVER_PAR_END
    int n = 0, anchor_c = 0;
    SOLVER_PAR_BEGIN
    n = g.cid[nodes], anchor_c = g.cid[anchor];
    SOLVER_PAR_END
    g.n = n, g.anchor_c = anchor_c;
    g.p2 = 1;
    while (g.p2 < n) g.p2 *= 2;
    SOLVER_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        const int node = g.cnode[c];
        for (int j = g.off[node]; j < g.off[node + 1]; ++j) g.adj_nbr[j] = g.cid[g.adj_nbr[j]];
    }
    SOLVER_PAR_END
}

// ---- the trust region's scalar rules ----

// the ratio of the actual to the model's decrease, regularised (Manopt); -1 when the trial cost or the ratio is not finite
GTSFM_HD double solver_rho(double f, double f_new, double model) {
    const double reg = SOLVER_RHO_REG * (fabs(f) > 1.0 ? fabs(f) : 1.0);
    const double rho = ((f - f_new) + reg) / (-model + reg);
    return isfinite(f_new) && isfinite(rho) ? rho : -1.0;
}
GTSFM_HD double solver_radius(double delta, double rho, bool on_boundary) {
    return rho < 0.25 ? delta / 4.0 : rho > 0.75 && on_boundary ? delta * 2.0 : delta;
}
// the step along d from eta to the boundary |eta + tau d| = delta
GTSFM_HD double solver_boundary_tau(double e_pe, double e_pd, double d_pd, double delta) {
    return (-e_pd + sqrt(e_pd * e_pd + d_pd * (delta * delta - e_pe))) / d_pd;
}

// ---- the launch shell ----

__global__ __launch_bounds__(SOLVER_THREADS) void solver_clear_flags_kernel(int* flags) {
    if (threadIdx.x < SOLVER_FLAG_WORDS) flags[threadIdx.x] = 0;
}

// Clears the flag words, runs the stage's validate kernel over n indices and reads flags[0 .. 2) back: the call's one stream wait, before
// anything is written. The caller words its two refusals, then launches its solve kernel with one workgroup per problem.
template <class Args>
int solver_launch(const char* me, void (*validate_kernel)(Args, long long), const char* validate_name, const Args& a, int* flags_dev, long long n,
                  hipStream_t stream, int* flags) {
    hipLaunchKernelGGL(solver_clear_flags_kernel, dim3(1), dim3(SOLVER_THREADS), 0, stream, flags_dev);
    GTSFM_CHECK_LAUNCH("solver_clear_flags_kernel");
    hipLaunchKernelGGL(validate_kernel, dim3((unsigned)((n + SOLVER_THREADS - 1) / SOLVER_THREADS)), dim3(SOLVER_THREADS), 0, stream, a, n);
    GTSFM_CHECK_LAUNCH(validate_name);
    if (hipMemcpyAsync(flags, flags_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        gtsfm_set_error("%s: reading the input flags failed: %s", me, hipGetErrorString(hipGetLastError()));
        return GTSFM_ERR_HIP;
    }
    return GTSFM_OK;
}

}  // namespace
