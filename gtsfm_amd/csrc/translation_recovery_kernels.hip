// Translation recovery on the device: camera and landmark positions from the 1DSfM inlier directions, by the robust chordal cost
// f(x) = sum_e rho_k(|unit(x_b - x_a) - z_e| / sigma) plus one scale row, from a linear initialisation, by a Gauss-Newton trust region with
// Steihaug-Toint truncated CG and a scalar Jacobi preconditioner. See include/gtsfm_amd.h; the specification is
// tests/translation_recovery_reference.py, which this file follows operation for operation. The sibling of rotation_averaging_kernels.hip.
//
//   tr_validate_kernel : one lane per row: the validity byte, the refusal flags (a bad pair or measurement, bad track or problem offsets).
//            The host reads the flags here, before any output is written.
//   tr_solve_kernel    : ONE WORKGROUP PER PROBLEM runs everything else to the end.
//     rows       : a problem's rows are its pair rows, then its measurements in CSR order; each gets its two nodes (a, b): (i2, i1) for a
//            pair, (camera, N + track - first track) for a measurement (the track by a bisection of track_off).
//     adjacency  : degrees by integer atomics, a blocked scan, an arbitrary slot per entry (atomic cursor), then every entry is ranked
//            within its node's list by (neighbour, row) and moved to its place: the lists are in the order the specification sums in.
//     component  : labels spread from the anchor until a round changes nothing (at most N + T rounds); its nodes get compact ids in
//            ascending node id and the lists are renumbered. The scale row sits on the component's first valid row.
//     stage A, B : lane l owns the compact nodes l, l + 256, ...; a node's sums run over its list in order; every global scalar is the
//            pairwise tree over the compact index padded to a power of two, done in the workspace level by level. Hence no byte depends
//            on the lane count, the run, or the problem's place in a batch. There is no floating-point atomic, and nothing but + - * /
//            sqrt and comparisons (-ffp-contract=off). Nothing is assembled: a cost pass leaves, per list entry, the unit vector and the
//            two coefficients of the Gauss-Newton model (5 doubles), and a Hessian application is one pass over the lists.
//     Every loop has a cap that is an argument or a size; no loop waits on a value another lane may never write. All state lives in the
//     workspace (272 bytes per node, 105 per row).
// The solver is ONE function for the device and the host: a section between TR_PAR_BEGIN and TR_PAR_END is run by every lane and ends
// with a barrier; on the host (tools/translation_recovery_host_main.cpp) it is a loop over the lanes, in either order and with any lane
// count, and the atomics are plain updates. Scalars that steer the control flow are read from memory after a barrier: they are uniform.
// The adjacency, component, scan and tree code is a LOCAL COPY of the rotation kernel's: that file stays as it is.

#include <math.h>

#include "../../include/gtsfm_amd.h"
#include "graph_prims.h"

#define TR_HD __host__ __device__ __forceinline__
#define TR_THREADS 256
#define TR_MAX_ROWS (1ll << 28)   // pair rows + measurements
#define TR_MAX_NODES (1ll << 24)  // num_images + max_tracks
#define TR_MAX_STATE (1ll << 28)  // num_problems * nodes
#define TR_FLAG_WORDS 8           // 0: a bad pair row or measurement; 1: bad track or problem offsets
#define TR_NODE_DOUBLES 34        // the tree (2 per node, padded), ten 3-vectors (x, x', g, g', eta, H eta, r, M^-1 r, d, H d), m, m'
#define TR_ENTRY_DOUBLES 5        // u (3), w / (|d| sigma)^2, the scale row's w / sigma^2 (0 on every other row)
#define TR_RHO_REG (1e3 * 2.220446049250313e-16)
#define TR_CONVERGED 0
#define TR_MAX_ITERATIONS 1
#define TR_NO_VALID_ROW 2
#define TR_NON_FINITE 3

struct TrHostLanes {  // the host build's lane count and order (tools/translation_recovery_host_main.cpp)
    int lanes, descending;
};
static TrHostLanes tr_host = {1, 0};

#if defined(__HIP_DEVICE_COMPILE__)
#define TR_PAR_BEGIN                  \
    {                                 \
        const int lane = threadIdx.x; \
        const int lanes = TR_THREADS; \
        (void)lane, (void)lanes;
#define TR_PAR_END   \
    }                \
    __syncthreads();
#else
#define TR_PAR_BEGIN                                      \
    for (int tr_l = 0; tr_l < tr_host.lanes; ++tr_l) {    \
        const int lanes = tr_host.lanes;                  \
        const int lane = tr_host.descending ? lanes - 1 - tr_l : tr_l; \
        (void)lane, (void)lanes;
#define TR_PAR_END }
#endif

namespace {

struct TrWorkspace {
    int* flags;         // [TR_FLAG_WORDS]
    uint8_t* valid;     // [E + S]: the pair rows, then the measurements
    int *row_a, *row_b; // [E + S]: a row's nodes within its problem; a problem's slice starts at its first pair row + its first measurement
    int *off, *cid;     // [P][M + 2]: list offsets by node; compact ids (an exclusive scan of the reach flags)
    int *cursor, *reach, *cnode;  // [P][M]
    long long* lanebuf; // [P][TR_THREADS]
    int *raw_row, *raw_owner, *adj_nbr, *adj_row;  // [2 (E + S)]; a problem's slice starts at twice its first row
    double* entry;      // [2][2 (E + S)][TR_ENTRY_DOUBLES]: the model at the point held and at the trial point
    double* state;      // [P][TR_NODE_DOUBLES][M]
    size_t bytes;
};

TrWorkspace tr_layout(void* base, long long pairs, long long meas, long long nodes, long long problems) {
    TrWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t r = (size_t)(pairs + meas), m = (size_t)nodes, p = (size_t)problems;
    w.flags = (int*)ws.take(TR_FLAG_WORDS * 4);
    w.valid = (uint8_t*)ws.take(r);
    w.row_a = (int*)ws.take(r * 4);
    w.row_b = (int*)ws.take(r * 4);
    w.off = (int*)ws.take(p * (m + 2) * 4);
    w.cid = (int*)ws.take(p * (m + 2) * 4);
    w.cursor = (int*)ws.take(p * m * 4);
    w.reach = (int*)ws.take(p * m * 4);
    w.cnode = (int*)ws.take(p * m * 4);
    w.lanebuf = (long long*)ws.take(p * TR_THREADS * 8);
    w.raw_row = (int*)ws.take(2 * r * 4);
    w.raw_owner = (int*)ws.take(2 * r * 4);
    w.adj_nbr = (int*)ws.take(2 * r * 4);
    w.adj_row = (int*)ws.take(2 * r * 4);
    w.entry = (double*)ws.take(2 * 2 * r * TR_ENTRY_DOUBLES * 8);
    w.state = (double*)ws.take(p * TR_NODE_DOUBLES * (m ? m : 1) * 8);
    w.bytes = ws.used;
    return w;
}

struct TrArgs {
    const int* pair_images;      // [E][2]
    const double* world_pair;    // [E][3]
    const uint8_t* pair_enable;  // [E] or null
    const long long* track_off;  // [T + 1] (null when T == 0)
    const int* image;            // [S]
    const double* world_meas;    // [S][3]
    const uint8_t* meas_enable;  // [S] or null
    const long long* row_off;    // [P + 1][2] = (first pair row, first track) or null: one problem over everything
    long long num_pairs, num_tracks, num_meas;
    int num_images, max_tracks, num_problems, anchor;
    double scale, sigma, huber_k, init_tol, delta0, kappa_cg, gradient_tol, rel_tol, abs_tol;
    int init_cap, max_outer, max_inner;
    TrWorkspace w;
    double* translation;  // [P][M][3]
    uint8_t* node_valid;  // [P][M]
    int* counters;        // [P][8]
    double* costs;        // [P][4]
};

TR_HD double tr_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ---- the validity pass ----

TR_HD void tr_validate(const TrArgs& a, long long m) {
    const long long E = a.num_pairs, S = a.num_meas, T = a.num_tracks;
    if (m < a.num_problems) {
        const long long plo = a.row_off ? a.row_off[2 * m] : 0, phi = a.row_off ? a.row_off[2 * m + 2] : E;
        const long long tlo = a.row_off ? a.row_off[2 * m + 1] : 0, thi = a.row_off ? a.row_off[2 * m + 3] : T;
        if (!(plo >= 0 && plo <= phi && phi <= E && tlo >= 0 && tlo <= thi && thi <= T && thi - tlo <= a.max_tracks)) a.w.flags[1] = 1;
    }
    if (m < T && !(a.track_off[m] >= 0 && a.track_off[m] <= a.track_off[m + 1] && a.track_off[m + 1] <= S)) a.w.flags[1] = 1;
    if (m == 0 && (T > 0 ? (a.track_off[0] != 0 || a.track_off[T] != S) : S != 0)) a.w.flags[1] = 1;
    if (m < E) {
        uint8_t ok = 0;
        if (!a.pair_enable || a.pair_enable[m]) {
            const int i1 = a.pair_images[2 * m], i2 = a.pair_images[2 * m + 1];
            if (!(i1 >= 0 && i1 < i2 && i2 < a.num_images)) {
                a.w.flags[0] = 1;
            } else {
                const double* z = a.world_pair + 3 * m;
                ok = isfinite(z[0]) && isfinite(z[1]) && isfinite(z[2]) ? 1 : 0;
            }
        }
        a.w.valid[m] = ok;
    }
    if (m < S) {
        uint8_t ok = 0;
        if (!a.meas_enable || a.meas_enable[m]) {
            const int i = a.image[m];
            if (!(i >= 0 && i < a.num_images)) {
                a.w.flags[0] = 1;
            } else {
                const double* z = a.world_meas + 3 * m;
                ok = isfinite(z[0]) && isfinite(z[1]) && isfinite(z[2]) ? 1 : 0;
            }
        }
        a.w.valid[E + m] = ok;
    }
}

// ---- the per-problem state ----

struct TrProblem {
    long long plo, mlo;  // the problem's first pair row and first measurement
    int np, rows;        // its pair rows; its rows
    int n, p2, anchor_c, e0;
    int *row_a, *row_b, *off, *cid, *cursor, *reach, *cnode, *raw_row, *raw_owner, *adj_nbr, *adj_row;
    long long* lanebuf;
    double *x, *xn, *g, *gn, *m, *mn, *eta, *heta, *res, *zv, *d, *hd, *t, *entry, *entry_n;
};

TR_HD bool tr_row_valid(const TrArgs& a, const TrProblem& q, int l) {
    return (l < q.np ? a.w.valid[q.plo + l] : a.w.valid[a.num_pairs + q.mlo + (l - q.np)]) != 0;
}
TR_HD const double* tr_row_z(const TrArgs& a, const TrProblem& q, int l) {
    return l < q.np ? a.world_pair + 3 * (q.plo + l) : a.world_meas + 3 * (q.mlo + (l - q.np));
}

// val[0 .. n) -> its exclusive prefix sum in place, val[n] = the total: every lane a contiguous chunk
TR_HD void tr_scan(int* val, int n, long long* lanebuf) {
    TR_PAR_BEGIN
    const int chunk = (n + lanes - 1) / lanes, from = lane * chunk < n ? lane * chunk : n, to = from + chunk < n ? from + chunk : n;
    long long s = 0;
    for (int i = from; i < to; ++i) s += val[i];
    lanebuf[lane] = s;
    TR_PAR_END
    TR_PAR_BEGIN
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
    TR_PAR_END
}

// the tree over t[0 .. p2): t[i] = t[i] (+ or max) t[i + s] level by level; the result is uniform
TR_HD double tr_tree(double* t, int p2, bool take_max) {
    for (long long s = 1; s < p2; s <<= 1) {
        TR_PAR_BEGIN
        for (long long i = (long long)lane * 2 * s; i < p2; i += (long long)lanes * 2 * s) {
            const double x = t[i], y = t[i + s];
            t[i] = take_max ? (x > y ? x : y) : x + y;
        }
        TR_PAR_END
    }
    double out = 0.0;
    TR_PAR_BEGIN
    out = t[0];
    TR_PAR_END
    return out;
}
TR_HD void tr_tree_pad(const TrProblem& q, int lane, int lanes) {
    for (int c = q.n + lane; c < q.p2; c += lanes) q.t[c] = 0.0;
}

// <x, y> over the nodes
TR_HD double tr_dot_nodes(const TrProblem& q, const double* x, const double* y) {
    TR_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) q.t[c] = tr_dot3(x + 3 * (size_t)c, y + 3 * (size_t)c);
    tr_tree_pad(q, lane, lanes);
    TR_PAR_END
    return tr_tree(q.t, q.p2, false);
}

// |g|_inf
TR_HD double tr_inf_norm(const TrProblem& q, const double* g) {
    TR_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const double* v = g + 3 * (size_t)c;
        const double m01 = fabs(v[0]) > fabs(v[1]) ? fabs(v[0]) : fabs(v[1]);
        q.t[c] = m01 > fabs(v[2]) ? m01 : fabs(v[2]);
    }
    tr_tree_pad(q, lane, lanes);
    TR_PAR_END
    return tr_tree(q.t, q.p2, true);
}

// dst_k = sum over k's list of (src_k - src_j): the scalar graph Laplacian on three columns; the anchor's row is zero
TR_HD void tr_laplacian(const TrProblem& q, const double* src, double* dst) {
    TR_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        const double* sk = src + 3 * (size_t)c;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const double* sj = src + 3 * (size_t)q.adj_nbr[j];
            for (int i = 0; i < 3; ++i) acc[i] = acc[i] + (sk[i] - sj[i]);
        }
        for (int i = 0; i < 3; ++i) dst[3 * (size_t)c + i] = c == q.anchor_c ? 0.0 : acc[i];
    }
    TR_PAR_END
}

// Huber's rho and weight at s = |r| / sigma
TR_HD void tr_huber(double s, bool huber, double k, double* rho, double* w) {
    if (huber && s > k) {
        *rho = k * (s - 0.5 * k), *w = k / s;
    } else {
        *rho = 0.5 * (s * s), *w = 1.0;
    }
}

// the cost at x; its gradient into g (the anchor's zero), the Jacobi weights into mw and the model's entries into entry
TR_HD double tr_pass(const TrArgs& a, const TrProblem& q, const double* x, double* g, double* mw, double* entry) {
    TR_PAR_BEGIN
    const double sigma = a.sigma, sig2 = a.sigma * a.sigma, k = a.huber_k;
    const bool huber = k > 0 && isfinite(k);
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        const double* xk = x + 3 * (size_t)c;
        double acc[3] = {0.0, 0.0, 0.0}, cost = 0.0, macc = 0.0;
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int e2 = q.adj_row[j], l = e2 >> 1, is_a = e2 & 1;
            const double *xj = x + 3 * (size_t)q.adj_nbr[j], *z = tr_row_z(a, q, l);
            const double *xa = is_a ? xk : xj, *xb = is_a ? xj : xk;
            double d[3], u[3], r[3], term[3], rho, w;
            for (int i = 0; i < 3; ++i) d[i] = xb[i] - xa[i];
            const double nrm = sqrt(tr_dot3(d, d));
            for (int i = 0; i < 3; ++i) u[i] = d[i] / nrm, r[i] = u[i] - z[i];
            tr_huber(sqrt(tr_dot3(r, r)) / sigma, huber, k, &rho, &w);
            const double ur = tr_dot3(u, r), cg = w / (nrm * sig2), coef = w / ((nrm * sigma) * (nrm * sigma));
            for (int i = 0; i < 3; ++i) term[i] = cg * (r[i] - u[i] * ur);
            double coef_s = 0.0;
            if (l == q.e0) {  // the scale row
                double rs[3], rho_s, w_s;
                for (int i = 0; i < 3; ++i) rs[i] = d[i] - a.scale * z[i];
                tr_huber(sqrt(tr_dot3(rs, rs)) / sigma, huber, k, &rho_s, &w_s);
                coef_s = w_s / sig2;
                for (int i = 0; i < 3; ++i) term[i] = term[i] + coef_s * rs[i];
                rho = rho + rho_s;
            }
            for (int i = 0; i < 3; ++i) acc[i] = is_a ? acc[i] - term[i] : acc[i] + term[i];
            cost = cost + rho;
            macc = macc + (2.0 * coef + 3.0 * coef_s);
            double* en = entry + TR_ENTRY_DOUBLES * (size_t)j;
            en[0] = u[0], en[1] = u[1], en[2] = u[2], en[3] = coef, en[4] = coef_s;
        }
        for (int i = 0; i < 3; ++i) g[3 * (size_t)c + i] = c == q.anchor_c ? 0.0 : acc[i];
        mw[c] = macc / 3.0;
        q.t[c] = cost;
    }
    tr_tree_pad(q, lane, lanes);
    TR_PAR_END
    return 0.5 * tr_tree(q.t, q.p2, false);  // every row is in two lists
}

// hd = H[d] by the entries of the point held, the anchor's zero; returns <d, hd>
TR_HD double tr_hessian(const TrProblem& q) {
    TR_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        const double* vk = q.d + 3 * (size_t)c;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int is_a = q.adj_row[j] & 1;
            const double *vj = q.d + 3 * (size_t)q.adj_nbr[j], *en = q.entry + TR_ENTRY_DOUBLES * (size_t)j;
            double dv[3];
            for (int i = 0; i < 3; ++i) dv[i] = is_a ? vj[i] - vk[i] : vk[i] - vj[i];
            const double udv = tr_dot3(en, dv);
            for (int i = 0; i < 3; ++i) {
                const double term = en[3] * (dv[i] - en[i] * udv) + en[4] * dv[i];
                acc[i] = is_a ? acc[i] - term : acc[i] + term;
            }
        }
        double* hd = q.hd + 3 * (size_t)c;
        for (int i = 0; i < 3; ++i) hd[i] = c == q.anchor_c ? 0.0 : acc[i];
        q.t[c] = tr_dot3(vk, hd);
    }
    tr_tree_pad(q, lane, lanes);
    TR_PAR_END
    return tr_tree(q.t, q.p2, false);
}

// ---- one problem, start to end ----

TR_HD void tr_solve(const TrArgs& a, int p) {
    const int N = a.num_images, M = a.num_images + a.max_tracks;
    TrProblem q;
    q.plo = a.row_off ? a.row_off[2 * p] : 0;
    const long long phi = a.row_off ? a.row_off[2 * p + 2] : a.num_pairs;
    const long long tlo = a.row_off ? a.row_off[2 * p + 1] : 0, thi = a.row_off ? a.row_off[2 * p + 3] : a.num_tracks;
    q.mlo = a.num_tracks > 0 ? a.track_off[tlo] : 0;
    const long long mhi = a.num_tracks > 0 ? a.track_off[thi] : 0;
    q.np = (int)(phi - q.plo), q.rows = q.np + (int)(mhi - q.mlo);
    const size_t first = (size_t)(q.plo + q.mlo);
    q.row_a = a.w.row_a + first, q.row_b = a.w.row_b + first;
    q.off = a.w.off + (size_t)p * (M + 2), q.cid = a.w.cid + (size_t)p * (M + 2);
    q.cursor = a.w.cursor + (size_t)p * M, q.reach = a.w.reach + (size_t)p * M, q.cnode = a.w.cnode + (size_t)p * M;
    q.lanebuf = a.w.lanebuf + (size_t)p * TR_THREADS;
    q.raw_row = a.w.raw_row + 2 * first, q.raw_owner = a.w.raw_owner + 2 * first, q.adj_nbr = a.w.adj_nbr + 2 * first, q.adj_row = a.w.adj_row + 2 * first;
    q.entry = a.w.entry + TR_ENTRY_DOUBLES * 2 * first;
    q.entry_n = a.w.entry + TR_ENTRY_DOUBLES * 2 * ((size_t)(a.num_pairs + a.num_meas) + first);
    double* out = a.translation + 3 * (size_t)p * M;
    uint8_t* node_valid = a.node_valid + (size_t)p * M;
    int* counters = a.counters + 8 * (size_t)p;
    double* costs = a.costs + 4 * (size_t)p;
    const double nan = __builtin_nan("");

    // the outputs' defaults, every row's nodes, the degrees, the first valid row
    TR_PAR_BEGIN
    for (int i = lane; i < M + 2; i += lanes) q.off[i] = 0, q.cid[i] = 0;
    for (int i = lane; i < M; i += lanes) {
        q.cursor[i] = 0, q.reach[i] = 0, node_valid[i] = 0;
        for (int k = 0; k < 3; ++k) out[3 * (size_t)i + k] = nan;
    }
    for (int i = lane; i < 8; i += lanes) counters[i] = 0;
    for (int i = lane; i < 4; i += lanes) costs[i] = nan;
    TR_PAR_END
    TR_PAR_BEGIN
    long long first_row = q.rows;
    for (int l = lane; l < q.rows; l += lanes) {
        int na, nb;
        if (l < q.np) {
            na = a.pair_images[2 * (q.plo + l) + 1], nb = a.pair_images[2 * (q.plo + l)];
        } else {
            const long long s = q.mlo + (l - q.np);
            long long lo = tlo, hi = thi;  // the track: track_off[lo] <= s < track_off[hi]
            for (int it = 0; it < 64 && hi - lo > 1; ++it) {
                const long long mid = lo + (hi - lo) / 2;
                if (a.track_off[mid] <= s) {
                    lo = mid;
                } else {
                    hi = mid;
                }
            }
            na = a.image[s], nb = N + (int)(lo - tlo);
        }
        q.row_a[l] = na, q.row_b[l] = nb;
        if (!tr_row_valid(a, q, l)) continue;
        hd_atomic_add(&q.off[na], 1);
        hd_atomic_add(&q.off[nb], 1);
        if (l < first_row) first_row = l;
    }
    q.lanebuf[lane] = first_row;
    TR_PAR_END
    long long first_row = q.rows;
    TR_PAR_BEGIN
    first_row = q.rows;
    for (int l = 0; l < lanes; ++l) first_row = q.lanebuf[l] < first_row ? q.lanebuf[l] : first_row;
    TR_PAR_END
    tr_scan(q.off, M, q.lanebuf);
    int total = 0;
    TR_PAR_BEGIN
    total = q.off[M];
    TR_PAR_END
    if (first_row >= q.rows) {
        TR_PAR_BEGIN
        if (lane == 0) counters[0] = TR_NO_VALID_ROW, counters[6] = a.anchor;
        TR_PAR_END
        return;
    }
    int anchor = a.anchor;
    TR_PAR_BEGIN
    anchor = a.anchor >= 0 ? a.anchor : q.row_a[first_row];
    TR_PAR_END

    // the lists: a slot each, then every entry to its rank by (neighbour, row)
    TR_PAR_BEGIN
    for (int l = lane; l < q.rows; l += lanes) {
        if (!tr_row_valid(a, q, l)) continue;
        const int na = q.row_a[l], nb = q.row_b[l];
        const int s1 = q.off[na] + hd_atomic_add(&q.cursor[na], 1), s2 = q.off[nb] + hd_atomic_add(&q.cursor[nb], 1);
        if (s1 < q.off[na + 1]) q.raw_row[s1] = l, q.raw_owner[s1] = na;  // always true: exactly degree rows ask
        if (s2 < q.off[nb + 1]) q.raw_row[s2] = l, q.raw_owner[s2] = nb;
    }
    TR_PAR_END
    TR_PAR_BEGIN
    for (int s = lane; s < total; s += lanes) {
        const int row = q.raw_row[s], owner = q.raw_owner[s];
        const int na = q.row_a[row], nbr = owner == na ? q.row_b[row] : na;
        int rank = 0;
        for (int j = q.off[owner]; j < q.off[owner + 1]; ++j) {
            const int rj = q.raw_row[j], ja = q.row_a[rj], nj = owner == ja ? q.row_b[rj] : ja;
            if (nj < nbr || (nj == nbr && rj < row)) ++rank;
        }
        q.adj_nbr[q.off[owner] + rank] = nbr;
        q.adj_row[q.off[owner] + rank] = 2 * row + (owner == na ? 1 : 0);
    }
    TR_PAR_END

    // the anchor's component. The lanes read reach[] of their neighbours while other lanes set it in the same section: a race that is MEANT.
    // reach[] only ever goes from 0 to 1 (a 4-byte store), a lane that misses a fresh 1 sees it in the next round, and the fixed point -- the
    // component -- is unique; only the number of rounds depends on the timing, and no output holds it. The loop ends after a round without a
    // change, at most M rounds.
    TR_PAR_BEGIN
    if (lane == 0) q.reach[anchor] = 1;
    TR_PAR_END
    for (int round = 0; round < M; ++round) {
        TR_PAR_BEGIN
        long long changed = 0;
        for (int node = lane; node < M; node += lanes) {
            if (q.reach[node]) continue;
            for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
                if (q.reach[q.adj_nbr[j]]) {
                    q.reach[node] = 1, changed = 1;
                    break;
                }
            }
        }
        q.lanebuf[lane] = changed;
        TR_PAR_END
        long long any = 0;
        TR_PAR_BEGIN
        any = 0;
        for (int l = 0; l < lanes; ++l) any |= q.lanebuf[l];
        TR_PAR_END
        if (!any) break;
    }
    TR_PAR_BEGIN
    for (int i = lane; i < M; i += lanes) q.cid[i] = q.reach[i];
    TR_PAR_END
    tr_scan(q.cid, M, q.lanebuf);
    TR_PAR_BEGIN
    for (int i = lane; i < M; i += lanes)
        if (q.reach[i]) q.cnode[q.cid[i]] = i;
    // the scale row: the component's first valid row
    long long e0 = q.rows;
    for (int l = lane; l < q.rows; l += lanes)
        if (tr_row_valid(a, q, l) && q.reach[q.row_a[l]] && l < e0) e0 = l;
    q.lanebuf[lane] = e0;
    TR_PAR_END
    int n = 0, anchor_c = 0;
    long long e0 = q.rows;
    TR_PAR_BEGIN
    n = q.cid[M], anchor_c = q.cid[anchor];
    e0 = q.rows;
    for (int l = 0; l < lanes; ++l) e0 = q.lanebuf[l] < e0 ? q.lanebuf[l] : e0;
    TR_PAR_END
    q.n = n, q.anchor_c = anchor_c, q.e0 = (int)e0;
    q.p2 = 1;
    while (q.p2 < n) q.p2 *= 2;
    TR_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        const int node = q.cnode[c];
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) q.adj_nbr[j] = q.cid[q.adj_nbr[j]];
    }
    TR_PAR_END

    double* base = a.w.state + (size_t)p * TR_NODE_DOUBLES * (size_t)M;
    const size_t sm = (size_t)M;
    q.t = base;  // p2 < 2 n <= 2 M
    q.x = base + 2 * sm, q.xn = base + 5 * sm, q.g = base + 8 * sm, q.gn = base + 11 * sm, q.eta = base + 14 * sm, q.heta = base + 17 * sm;
    q.res = base + 20 * sm, q.zv = base + 23 * sm, q.d = base + 26 * sm, q.hd = base + 29 * sm, q.m = base + 32 * sm, q.mn = base + 33 * sm;

    // stage A: CG on the reduced graph Laplacian from x = 0, three right-hand sides and one step length; residual = res, direction = d, L d = hd
    double *x = q.x, *cr = q.res, *cp = q.d, *cap = q.hd;
    TR_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        const int node = q.cnode[c];
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int e2 = q.adj_row[j];
            const double* z = tr_row_z(a, q, e2 >> 1);
            for (int i = 0; i < 3; ++i) acc[i] = (e2 & 1) ? acc[i] - a.scale * z[i] : acc[i] + a.scale * z[i];
        }
        for (int i = 0; i < 3; ++i) {
            const size_t at = 3 * (size_t)c + i;
            cr[at] = c == anchor_c ? 0.0 : acc[i];
            cp[at] = cr[at], x[at] = 0.0;
        }
        q.t[c] = tr_dot3(cr + 3 * (size_t)c, cr + 3 * (size_t)c);
    }
    tr_tree_pad(q, lane, lanes);
    TR_PAR_END
    double rr = tr_tree(q.t, q.p2, false);
    const double rr0 = rr;
    int init_steps = 0;
    while (init_steps < a.init_cap && rr > (a.init_tol * a.init_tol) * rr0) {
        tr_laplacian(q, cp, cap);
        const double pap = tr_dot_nodes(q, cp, cap);
        if (!(pap > 0)) break;
        const double alpha = rr / pap;
        TR_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) {
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                x[at] = x[at] + alpha * cp[at];
                cr[at] = cr[at] - alpha * cap[at];
            }
            q.t[c] = tr_dot3(cr + 3 * (size_t)c, cr + 3 * (size_t)c);
        }
        tr_tree_pad(q, lane, lanes);
        TR_PAR_END
        const double rr_new = tr_tree(q.t, q.p2, false);
        const double beta = rr_new / rr;
        TR_PAR_BEGIN
        for (int c = lane; c < n; c += lanes)
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                cp[at] = cr[at] + beta * cp[at];
            }
        TR_PAR_END
        rr = rr_new;
        ++init_steps;
    }

    // stage B
    const double sig2 = a.sigma * a.sigma;
    double f = tr_pass(a, q, q.x, q.g, q.m, q.entry);
    const double init_cost = f;
    int status = isfinite(f) ? TR_MAX_ITERATIONS : TR_NON_FINITE;
    const int inner_cap = a.max_inner > 0 ? a.max_inner : 3 * n;
    double delta = a.delta0, gn = nan;
    int outer = 0, accepted = 0, happ = 0;
    while (status == TR_MAX_ITERATIONS) {
        gn = tr_inf_norm(q, q.g);
        TR_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) {
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                q.zv[at] = c == anchor_c ? 0.0 : q.g[at] / q.m[c];
                q.eta[at] = 0.0, q.heta[at] = 0.0, q.res[at] = q.g[at], q.d[at] = -q.zv[at];
            }
            q.t[c] = tr_dot3(q.zv + 3 * (size_t)c, q.res + 3 * (size_t)c);
        }
        tr_tree_pad(q, lane, lanes);
        TR_PAR_END
        double z_r = tr_tree(q.t, q.p2, false);
        if (!isfinite(z_r)) {
            status = TR_NON_FINITE;
            break;
        }
        if (gn <= a.gradient_tol / sig2) {
            status = TR_CONVERGED;
            break;
        }
        if (outer >= a.max_outer) break;
        ++outer;
        const double target = sqrt(z_r) * a.kappa_cg;
        double e_pe = 0.0, e_pd = 0.0, d_pd = z_r;
        bool on_boundary = false;
        for (int inner = 0; inner < inner_cap; ++inner) {
            const double d_hd = tr_hessian(q);
            ++happ;
            const double alpha = z_r / d_hd;
            const double e_pe_new = e_pe + 2.0 * alpha * e_pd + alpha * alpha * d_pd;
            if (!(d_hd > 0) || e_pe_new >= delta * delta) {
                const double tau = (-e_pd + sqrt(e_pd * e_pd + d_pd * (delta * delta - e_pe))) / d_pd;
                TR_PAR_BEGIN
                for (int c = lane; c < n; c += lanes)
                    for (int i = 0; i < 3; ++i) {
                        const size_t at = 3 * (size_t)c + i;
                        q.eta[at] = q.eta[at] + tau * q.d[at], q.heta[at] = q.heta[at] + tau * q.hd[at];
                    }
                TR_PAR_END
                on_boundary = true;
                break;
            }
            e_pe = e_pe_new;
            TR_PAR_BEGIN
            for (int c = lane; c < n; c += lanes) {
                for (int i = 0; i < 3; ++i) {
                    const size_t at = 3 * (size_t)c + i;
                    q.eta[at] = q.eta[at] + alpha * q.d[at], q.heta[at] = q.heta[at] + alpha * q.hd[at];
                    q.res[at] = q.res[at] + alpha * q.hd[at];
                    q.zv[at] = c == anchor_c ? 0.0 : q.res[at] / q.m[c];
                }
                q.t[c] = tr_dot3(q.zv + 3 * (size_t)c, q.res + 3 * (size_t)c);
            }
            tr_tree_pad(q, lane, lanes);
            TR_PAR_END
            const double zr_new = tr_tree(q.t, q.p2, false);
            if (sqrt(zr_new) <= target) break;
            const double beta = zr_new / z_r;
            TR_PAR_BEGIN
            for (int c = lane; c < n; c += lanes)
                for (int i = 0; i < 3; ++i) {
                    const size_t at = 3 * (size_t)c + i;
                    q.d[at] = -q.zv[at] + beta * q.d[at];
                }
            TR_PAR_END
            e_pd = beta * (e_pd + alpha * d_pd);
            d_pd = zr_new + beta * beta * d_pd;
            z_r = zr_new;
        }
        const double g_eta = tr_dot_nodes(q, q.g, q.eta);
        const double model = g_eta + 0.5 * tr_dot_nodes(q, q.eta, q.heta);
        TR_PAR_BEGIN
        for (int c = lane; c < n; c += lanes)
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                q.xn[at] = q.x[at] + q.eta[at];
            }
        TR_PAR_END
        const double f_new = tr_pass(a, q, q.xn, q.gn, q.mn, q.entry_n);
        const double reg = TR_RHO_REG * (fabs(f) > 1.0 ? fabs(f) : 1.0);
        double rho = ((f - f_new) + reg) / (-model + reg);
        if (!(isfinite(f_new) && isfinite(rho))) rho = -1.0;
        bool small = false;
        if (rho > 0.1) {
            double* s = q.x;
            q.x = q.xn, q.xn = s;
            s = q.g, q.g = q.gn, q.gn = s;
            s = q.m, q.m = q.mn, q.mn = s;
            s = q.entry, q.entry = q.entry_n, q.entry_n = s;
            const double drop = f - f_new;
            small = drop <= a.rel_tol * f || drop <= a.abs_tol;
            f = f_new;
            ++accepted;
        }
        if (rho < 0.25) {
            delta = delta / 4.0;
        } else if (rho > 0.75 && on_boundary) {
            delta = delta * 2.0;
        }
        if (small) {
            status = TR_CONVERGED;
            gn = tr_inf_norm(q, q.g);
        }
    }

    TR_PAR_BEGIN
    if (status != TR_NON_FINITE) {
        for (int c = lane; c < n; c += lanes) {
            double* o = out + 3 * (size_t)q.cnode[c];
            for (int i = 0; i < 3; ++i) o[i] = c == anchor_c ? 0.0 : q.x[3 * (size_t)c + i];
            node_valid[q.cnode[c]] = 1;
        }
    }
    if (lane == 0) {
        const int valid_rows = total / 2;  // the lists hold every valid row twice
        counters[0] = status, counters[1] = outer, counters[2] = accepted, counters[3] = happ, counters[4] = init_steps, counters[5] = n;
        counters[6] = anchor, counters[7] = valid_rows;
        costs[0] = init_cost, costs[1] = f, costs[2] = gn, costs[3] = delta;
    }
    TR_PAR_END
}

// ---- kernels ----

__global__ __launch_bounds__(TR_THREADS) void tr_init_kernel(TrArgs a) {
    if (threadIdx.x < TR_FLAG_WORDS) a.w.flags[threadIdx.x] = 0;
}
__global__ __launch_bounds__(TR_THREADS) void tr_validate_kernel(TrArgs a, long long n) {
    const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    if (i < n) tr_validate(a, i);
}
// one workgroup per problem; every branch around a barrier is on a uniform value
__global__ __launch_bounds__(TR_THREADS) void tr_solve_kernel(TrArgs a) { tr_solve(a, (int)blockIdx.x); }

bool tr_sizes_ok(long long num_pairs, long long num_meas, long long num_images, long long num_tracks, long long max_tracks, long long num_problems) {
    return num_pairs >= 0 && num_meas >= 0 && num_images >= 0 && num_tracks >= 0 && max_tracks >= 0 && max_tracks <= num_tracks && num_problems >= 1 &&
           num_pairs + num_meas < TR_MAX_ROWS && num_tracks < TR_MAX_ROWS && num_images + max_tracks < TR_MAX_NODES && num_problems < TR_MAX_STATE &&
           num_problems * (num_images + max_tracks > 0 ? num_images + max_tracks : 1) < TR_MAX_STATE;
}
bool tr_options_ok(double scale, double sigma, double huber_k, double init_tol, int init_cap, double delta0, double kappa_cg, double gradient_tol, double rel_tol,
                   double abs_tol, int max_outer, int max_inner) {
    return isfinite(scale) && scale > 0 && isfinite(sigma) && sigma > 0 && !(huber_k != huber_k) && init_tol >= 0 && init_cap >= 0 && delta0 > 0 && kappa_cg >= 0 &&
           gradient_tol >= 0 && rel_tol >= 0 && abs_tol >= 0 && max_outer >= 0 && max_inner >= 0;
}
// the longest run of measurements a validate lane index must cover
long long tr_validate_lanes(long long num_pairs, long long num_meas, long long num_tracks, long long num_problems) {
    long long n = num_pairs > num_meas ? num_pairs : num_meas;
    n = n > num_tracks ? n : num_tracks;
    n = n > num_problems ? n : num_problems;
    return n > 1 ? n : 1;
}

}  // namespace

extern "C" size_t gtsfm_translation_recovery_workspace_bytes(long long num_pairs, long long num_meas, long long num_images, long long num_tracks,
                                                             long long max_problem_tracks, long long num_problems) {
    if (!tr_sizes_ok(num_pairs, num_meas, num_images, num_tracks, max_problem_tracks, num_problems)) return 0;
    return tr_layout(nullptr, num_pairs, num_meas, num_images + max_problem_tracks, num_problems).bytes;
}

extern "C" int gtsfm_translation_recovery_f64(const int32_t* pair_images_dev, const double* world_pair_dev, const uint8_t* pair_enable_dev, long long num_pairs,
                                              const long long* track_off_dev, const int32_t* image_dev, const double* world_meas_dev, const uint8_t* meas_enable_dev,
                                              long long num_tracks, long long num_meas, int num_images, const long long* problem_row_off_dev, int num_problems,
                                              long long max_problem_tracks, int anchor, double scale_factor, double sigma, double huber_k, double init_tol,
                                              int init_max_iterations, double delta0, double kappa_cg, double gradient_tol, double rel_tol, double abs_tol, int max_outer,
                                              int max_inner, void* workspace_dev, size_t workspace_bytes, double* translation_out_dev, uint8_t* node_valid_dev,
                                              int32_t* counters_dev, double* costs_dev, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* me = "gtsfm_translation_recovery_f64";
    GTSFM_CHECK_ARG(tr_sizes_ok(num_pairs, num_meas, num_images, num_tracks, max_problem_tracks, num_problems),
                    "%s: sizes out of range (%lld pairs, %lld measurements, %d images, %lld tracks, %lld per problem, %d problems)", me, num_pairs, num_meas, num_images,
                    num_tracks, max_problem_tracks, num_problems);
    const long long nodes = num_images + max_problem_tracks;
    GTSFM_CHECK_ARG(anchor >= -1 && (anchor < nodes || anchor == -1), "%s: the anchor %d is outside -1 .. %lld", me, anchor, nodes - 1);
    GTSFM_CHECK_ARG(tr_options_ok(scale_factor, sigma, huber_k, init_tol, init_max_iterations, delta0, kappa_cg, gradient_tol, rel_tol, abs_tol, max_outer, max_inner),
                    "%s: scale_factor, sigma and delta0 must be positive and finite, huber_k not NaN, no tolerance or cap negative", me);
    GTSFM_CHECK_ARG(workspace_dev && counters_dev && costs_dev && (nodes == 0 || (translation_out_dev && node_valid_dev)), "%s: null pointer", me);
    GTSFM_CHECK_ARG(num_pairs == 0 || (pair_images_dev && world_pair_dev), "%s: null pair pointer", me);
    GTSFM_CHECK_ARG(num_tracks == 0 || track_off_dev, "%s: %lld tracks without track_off_dev", me, num_tracks);
    GTSFM_CHECK_ARG(num_meas == 0 || (num_tracks > 0 && image_dev && world_meas_dev), "%s: %lld measurements without tracks, image_dev or world_meas_dev", me, num_meas);
    GTSFM_CHECK_ARG(problem_row_off_dev || (num_problems == 1 && max_problem_tracks == num_tracks),
                    "%s: without problem_row_off_dev there is one problem and max_problem_tracks is num_tracks", me);
    GTSFM_CHECK_ARG(((uintptr_t)workspace_dev & 255) == 0, "%s: the workspace must be aligned to 256 bytes", me);
    TrArgs a{pair_images_dev, world_pair_dev, pair_enable_dev, track_off_dev, image_dev, world_meas_dev, meas_enable_dev, problem_row_off_dev, num_pairs, num_tracks, num_meas,
             num_images, (int)max_problem_tracks, num_problems, anchor, scale_factor, sigma, huber_k, init_tol, delta0, kappa_cg, gradient_tol, rel_tol, abs_tol,
             init_max_iterations, max_outer, max_inner, tr_layout(workspace_dev, num_pairs, num_meas, nodes, num_problems), translation_out_dev, node_valid_dev, counters_dev,
             costs_dev};
    if (workspace_bytes < a.w.bytes) {
        gtsfm_set_error("%s: workspace of %zu bytes, %zu needed for %lld rows, %lld nodes and %d problems", me, workspace_bytes, a.w.bytes, num_pairs + num_meas, nodes,
                        num_problems);
        return GTSFM_ERR_WORKSPACE;
    }
    const long long n = tr_validate_lanes(num_pairs, num_meas, num_tracks, num_problems);
    hipLaunchKernelGGL(tr_init_kernel, dim3(1), dim3(TR_THREADS), 0, stream, a);
    GTSFM_CHECK_LAUNCH("tr_init_kernel");
    hipLaunchKernelGGL(tr_validate_kernel, dim3((unsigned)((n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, stream, a, n);
    GTSFM_CHECK_LAUNCH("tr_validate_kernel");
    int flags[2] = {0, 0};
    if (hipMemcpyAsync(flags, a.w.flags, sizeof(flags), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        gtsfm_set_error("%s: reading the input flags failed: %s", me, hipGetErrorString(hipGetLastError()));
        return GTSFM_ERR_HIP;
    }
    GTSFM_CHECK_ARG(!flags[0], "%s: an enabled pair row has i1 >= i2, or a row names an image outside 0 .. %d; nothing was written", me, num_images - 1);
    GTSFM_CHECK_ARG(!flags[1], "%s: track_off_dev or problem_row_off_dev is not ascending within its range, or a problem has more than %lld tracks; nothing was written", me,
                    max_problem_tracks);
    hipLaunchKernelGGL(tr_solve_kernel, dim3((unsigned)num_problems), dim3(TR_THREADS), 0, stream, a);
    GTSFM_CHECK_LAUNCH("tr_solve_kernel");
    return GTSFM_OK;
}
