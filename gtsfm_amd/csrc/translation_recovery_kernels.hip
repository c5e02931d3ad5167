// Translation recovery on the device: camera and landmark positions from the 1DSfM inlier directions, by the robust chordal cost
// f(x) = sum_e rho_k(|unit(x_b - x_a) - z_e| / sigma) plus one scale row, from a linear initialisation, by a Gauss-Newton trust region with
// Steihaug-Toint truncated CG and a scalar Jacobi preconditioner. See include/gtsfm_amd.h; the specification is
// tests/translation_recovery_reference.py, which this file follows operation for operation.
//
//   trec_validate_kernel : one lane per row: the validity byte, the refusal flags (a bad pair or measurement, bad track or problem offsets).
//            The host reads the flags here, before any output is written.
//   trec_solve_kernel    : ONE WORKGROUP PER PROBLEM runs everything else to the end, on the scaffold of problem_solver.h (the lane model,
//            the adjacency lists in the order the specification sums in, the anchor's component with compact ids, the scan and the tree).
//     rows       : a problem's rows are its pair rows, then its measurements in CSR order; each gets its two nodes (a, b): (i2, i1) for a
//            pair, (camera, N + track - first track) for a measurement (the track by a bisection of track_off). The scale row sits on
//            the component's first valid row.
//     stage A, B : lane l owns the compact nodes l, l + 256, ...; a node's sums run over its list in order; every global scalar is the
//            pairwise tree over the compact index padded to a power of two, done in the workspace level by level. Hence no byte depends
//            on the lane count, the run, or the problem's place in a batch. There is no floating-point atomic, and nothing but + - * /
//            sqrt and comparisons (-ffp-contract=off). Nothing is assembled: a cost pass leaves, per list entry, the unit vector and the
//            two coefficients of the Gauss-Newton model (5 doubles), and a Hessian application is one pass over the lists.
//     All state lives in the workspace (272 bytes per node, 105 per row).
// The host build of trec_validate and trec_solve is tools/translation_recovery_host_main.cpp.

#include "../../include/gtsfm_amd.h"
#include "problem_solver.h"

#define TREC_MAX_ROWS (1ll << 28)   // pair rows + measurements
#define TREC_MAX_NODES (1ll << 24)  // num_images + max_tracks
#define TREC_MAX_STATE (1ll << 28)  // num_problems * nodes
#define TREC_NODE_DOUBLES 34        // the tree (2 per node, padded), ten 3-vectors (x, x', g, g', eta, H eta, r, M^-1 r, d, H d), m, m'
#define TREC_ENTRY_DOUBLES 5        // u (3), w / (|d| sigma)^2, the scale row's w / sigma^2 (0 on every other row)

namespace {

struct TrecWorkspace {
    int* flags;          // [SOLVER_FLAG_WORDS]; 0: a bad pair row or measurement; 1: bad track or problem offsets
    uint8_t* valid;      // [E + S]: the pair rows, then the measurements
    int *row_a, *row_b;  // [E + S]: a row's nodes within its problem; a problem's slice starts at its first pair row + its first measurement
    SolverGraph g;       // over the M = N + max_tracks nodes and the E + S rows
    double* entry;       // [2][2 (E + S)][TREC_ENTRY_DOUBLES]: the model at the point held and at the trial point
    double* state;       // [P][TREC_NODE_DOUBLES][M]
    size_t bytes;
};

TrecWorkspace trec_layout(void* base, long long pairs, long long meas, long long nodes, long long problems) {
    TrecWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t r = (size_t)(pairs + meas), m = (size_t)nodes, p = (size_t)problems;
    w.flags = (int*)ws.take(SOLVER_FLAG_WORDS * 4);
    w.valid = (uint8_t*)ws.take(r);
    w.row_a = (int*)ws.take(r * 4);
    w.row_b = (int*)ws.take(r * 4);
    w.g = solver_carve(ws, r, m, p);
    w.entry = (double*)ws.take(2 * 2 * r * TREC_ENTRY_DOUBLES * 8);
    w.state = (double*)ws.take(p * TREC_NODE_DOUBLES * (m ? m : 1) * 8);
    w.bytes = ws.used;
    return w;
}

struct TrecArgs {
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
    TrecWorkspace w;
    double* translation;  // [P][M][3]
    uint8_t* node_valid;  // [P][M]
    int* counters;        // [P][8]
    double* costs;        // [P][4]
};

// ---- the validity pass ----

GTSFM_HD void trec_validate(const TrecArgs& a, long long m) {
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

struct TrecProblem : SolverGraph {
    long long plo, mlo;  // the problem's first pair row and first measurement
    int np, rows;        // its pair rows; its rows
    int e0;              // the scale row
    int *row_a, *row_b;
    double *x, *xn, *g, *gn, *m, *mn, *eta, *heta, *res, *zv, *d, *hd, *entry, *entry_n;
};

GTSFM_HD bool trec_row_valid(const TrecArgs& a, const TrecProblem& q, int l) {
    return (l < q.np ? a.w.valid[q.plo + l] : a.w.valid[a.num_pairs + q.mlo + (l - q.np)]) != 0;
}
GTSFM_HD const double* trec_row_z(const TrecArgs& a, const TrecProblem& q, int l) {
    return l < q.np ? a.world_pair + 3 * (q.plo + l) : a.world_meas + 3 * (q.mlo + (l - q.np));
}

// dst_k = sum over k's list of (src_k - src_j): the scalar graph Laplacian on three columns; the anchor's row is zero
GTSFM_HD void trec_laplacian(const TrecProblem& q, const double* src, double* dst) {
    SOLVER_PAR_BEGIN
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
    SOLVER_PAR_END
}

// Huber's rho and weight at s = |r| / sigma
GTSFM_HD void trec_huber(double s, bool huber, double k, double* rho, double* w) {
    if (huber && s > k) {
        *rho = k * (s - 0.5 * k), *w = k / s;
    } else {
        *rho = 0.5 * (s * s), *w = 1.0;
    }
}

// the cost at x; its gradient into g (the anchor's zero), the Jacobi weights into mw and the model's entries into entry
GTSFM_HD double trec_pass(const TrecArgs& a, const TrecProblem& q, const double* x, double* g, double* mw, double* entry) {
    SOLVER_PAR_BEGIN
    const double sigma = a.sigma, sig2 = a.sigma * a.sigma, k = a.huber_k;
    const bool huber = k > 0 && isfinite(k);
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        const double* xk = x + 3 * (size_t)c;
        double acc[3] = {0.0, 0.0, 0.0}, cost = 0.0, macc = 0.0;
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int e2 = q.adj_row[j], l = e2 >> 1, is_a = e2 & 1;
            const double *xj = x + 3 * (size_t)q.adj_nbr[j], *z = trec_row_z(a, q, l);
            const double *xa = is_a ? xk : xj, *xb = is_a ? xj : xk;
            double d[3], u[3], r[3], term[3], rho, w;
            for (int i = 0; i < 3; ++i) d[i] = xb[i] - xa[i];
            const double nrm = sqrt(solver_dot(d, d, 3));
            for (int i = 0; i < 3; ++i) u[i] = d[i] / nrm, r[i] = u[i] - z[i];
            trec_huber(sqrt(solver_dot(r, r, 3)) / sigma, huber, k, &rho, &w);
            const double ur = solver_dot(u, r, 3), cg = w / (nrm * sig2), coef = w / ((nrm * sigma) * (nrm * sigma));
            for (int i = 0; i < 3; ++i) term[i] = cg * (r[i] - u[i] * ur);
            double coef_s = 0.0;
            if (l == q.e0) {  // the scale row
                double rs[3], rho_s, w_s;
                for (int i = 0; i < 3; ++i) rs[i] = d[i] - a.scale * z[i];
                trec_huber(sqrt(solver_dot(rs, rs, 3)) / sigma, huber, k, &rho_s, &w_s);
                coef_s = w_s / sig2;
                for (int i = 0; i < 3; ++i) term[i] = term[i] + coef_s * rs[i];
                rho = rho + rho_s;
            }
            for (int i = 0; i < 3; ++i) acc[i] = is_a ? acc[i] - term[i] : acc[i] + term[i];
            cost = cost + rho;
            macc = macc + (2.0 * coef + 3.0 * coef_s);
            double* en = entry + TREC_ENTRY_DOUBLES * (size_t)j;
            en[0] = u[0], en[1] = u[1], en[2] = u[2], en[3] = coef, en[4] = coef_s;
        }
        for (int i = 0; i < 3; ++i) g[3 * (size_t)c + i] = c == q.anchor_c ? 0.0 : acc[i];
        mw[c] = macc / 3.0;
        q.t[c] = cost;
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    return 0.5 * solver_tree(q.t, q.p2, false);  // every row is in two lists
}

// hd = H[d] by the entries of the point held, the anchor's zero; returns <d, hd>
GTSFM_HD double trec_hessian(const TrecProblem& q) {
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        const double* vk = q.d + 3 * (size_t)c;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int is_a = q.adj_row[j] & 1;
            const double *vj = q.d + 3 * (size_t)q.adj_nbr[j], *en = q.entry + TREC_ENTRY_DOUBLES * (size_t)j;
            double dv[3];
            for (int i = 0; i < 3; ++i) dv[i] = is_a ? vj[i] - vk[i] : vk[i] - vj[i];
            const double udv = solver_dot(en, dv, 3);
            for (int i = 0; i < 3; ++i) {
                const double term = en[3] * (dv[i] - en[i] * udv) + en[4] * dv[i];
                acc[i] = is_a ? acc[i] - term : acc[i] + term;
            }
        }
        double* hd = q.hd + 3 * (size_t)c;
        for (int i = 0; i < 3; ++i) hd[i] = c == q.anchor_c ? 0.0 : acc[i];
        q.t[c] = solver_dot(vk, hd, 3);
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    return solver_tree(q.t, q.p2, false);
}

// ---- one problem, start to end ----

GTSFM_HD void trec_solve(const TrecArgs& a, int p) {
    const int N = a.num_images, M = a.num_images + a.max_tracks;
    TrecProblem q;
    q.plo = a.row_off ? a.row_off[2 * p] : 0;
    const long long phi = a.row_off ? a.row_off[2 * p + 2] : a.num_pairs;
    const long long tlo = a.row_off ? a.row_off[2 * p + 1] : 0, thi = a.row_off ? a.row_off[2 * p + 3] : a.num_tracks;
    q.mlo = a.num_tracks > 0 ? a.track_off[tlo] : 0;
    const long long mhi = a.num_tracks > 0 ? a.track_off[thi] : 0;
    q.np = (int)(phi - q.plo), q.rows = q.np + (int)(mhi - q.mlo);
    const size_t first = (size_t)(q.plo + q.mlo);
    static_cast<SolverGraph&>(q) = solver_slice(a.w.g, p, M, first);
    q.row_a = a.w.row_a + first, q.row_b = a.w.row_b + first;
    q.entry = a.w.entry + TREC_ENTRY_DOUBLES * 2 * first;
    q.entry_n = a.w.entry + TREC_ENTRY_DOUBLES * 2 * ((size_t)(a.num_pairs + a.num_meas) + first);
    double* out = a.translation + 3 * (size_t)p * M;
    uint8_t* node_valid = a.node_valid + (size_t)p * M;
    int* counters = a.counters + 8 * (size_t)p;
    double* costs = a.costs + 4 * (size_t)p;
    const double nan = __builtin_nan("");

    // the outputs' defaults, every row's nodes
    SOLVER_PAR_BEGIN
    solver_clear(q, M, lane, lanes);
    for (int i = lane; i < M; i += lanes) {
        node_valid[i] = 0;
        for (int k = 0; k < 3; ++k) out[3 * (size_t)i + k] = nan;
    }
    for (int i = lane; i < 8; i += lanes) counters[i] = 0;
    for (int i = lane; i < 4; i += lanes) costs[i] = nan;
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
    }
    SOLVER_PAR_END
    int total = 0;
    const int first_row = solver_build_lists(
        q, M, q.rows, [&](int l, int* na, int* nb) { *na = q.row_a[l], *nb = q.row_b[l]; }, [&](int l) { return trec_row_valid(a, q, l); }, &total);
    if (first_row >= q.rows) {
        SOLVER_PAR_BEGIN
        if (lane == 0) counters[0] = SOLVER_NO_VALID_ROW, counters[6] = a.anchor;
        SOLVER_PAR_END
        return;
    }
    int anchor = a.anchor;
    SOLVER_PAR_BEGIN
    anchor = a.anchor >= 0 ? a.anchor : q.row_a[first_row];
    SOLVER_PAR_END
    solver_component(q, anchor, M);
    const int n = q.n, anchor_c = q.anchor_c;

    // the scale row: the component's first valid row
    SOLVER_PAR_BEGIN
    long long e0 = q.rows;
    for (int l = lane; l < q.rows; l += lanes)
        if (trec_row_valid(a, q, l) && q.reach[q.row_a[l]] && l < e0) e0 = l;
    q.lanebuf[lane] = e0;
    SOLVER_PAR_END
    long long e0 = q.rows;
    SOLVER_PAR_BEGIN
    e0 = q.rows;
    for (int l = 0; l < lanes; ++l) e0 = q.lanebuf[l] < e0 ? q.lanebuf[l] : e0;
    SOLVER_PAR_END
    q.e0 = (int)e0;

    double* base = a.w.state + (size_t)p * TREC_NODE_DOUBLES * (size_t)M;
    const size_t sm = (size_t)M;
    q.t = base;  // p2 < 2 n <= 2 M
    q.x = base + 2 * sm, q.xn = base + 5 * sm, q.g = base + 8 * sm, q.gn = base + 11 * sm, q.eta = base + 14 * sm, q.heta = base + 17 * sm;
    q.res = base + 20 * sm, q.zv = base + 23 * sm, q.d = base + 26 * sm, q.hd = base + 29 * sm, q.m = base + 32 * sm, q.mn = base + 33 * sm;

    // stage A: CG on the reduced graph Laplacian from x = 0, three right-hand sides and one step length; residual = res, direction = d, L d = hd
    double *x = q.x, *cr = q.res, *cp = q.d, *cap = q.hd;
    SOLVER_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        const int node = q.cnode[c];
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int e2 = q.adj_row[j];
            const double* z = trec_row_z(a, q, e2 >> 1);
            for (int i = 0; i < 3; ++i) acc[i] = (e2 & 1) ? acc[i] - a.scale * z[i] : acc[i] + a.scale * z[i];
        }
        for (int i = 0; i < 3; ++i) {
            const size_t at = 3 * (size_t)c + i;
            cr[at] = c == anchor_c ? 0.0 : acc[i];
            cp[at] = cr[at], x[at] = 0.0;
        }
        q.t[c] = solver_dot(cr + 3 * (size_t)c, cr + 3 * (size_t)c, 3);
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    double rr = solver_tree(q.t, q.p2, false);
    const double rr0 = rr;
    int init_steps = 0;
    while (init_steps < a.init_cap && rr > (a.init_tol * a.init_tol) * rr0) {
        trec_laplacian(q, cp, cap);
        const double pap = solver_dot_nodes(q, cp, cap, 3);
        if (!(pap > 0)) break;
        const double alpha = rr / pap;
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) {
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                x[at] = x[at] + alpha * cp[at];
                cr[at] = cr[at] - alpha * cap[at];
            }
            q.t[c] = solver_dot(cr + 3 * (size_t)c, cr + 3 * (size_t)c, 3);
        }
        solver_tree_pad(q, lane, lanes);
        SOLVER_PAR_END
        const double rr_new = solver_tree(q.t, q.p2, false);
        const double beta = rr_new / rr;
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes)
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                cp[at] = cr[at] + beta * cp[at];
            }
        SOLVER_PAR_END
        rr = rr_new;
        ++init_steps;
    }

    // stage B
    const double sig2 = a.sigma * a.sigma;
    double f = trec_pass(a, q, q.x, q.g, q.m, q.entry);
    const double init_cost = f;
    int status = isfinite(f) ? SOLVER_MAX_ITERATIONS : SOLVER_NON_FINITE;
    const int inner_cap = a.max_inner > 0 ? a.max_inner : 3 * n;
    double delta = a.delta0, gn = nan;
    int outer = 0, accepted = 0, happ = 0;
    while (status == SOLVER_MAX_ITERATIONS) {
        gn = solver_inf_norm(q, q.g, 3);
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) {
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                q.zv[at] = c == anchor_c ? 0.0 : q.g[at] / q.m[c];
                q.eta[at] = 0.0, q.heta[at] = 0.0, q.res[at] = q.g[at], q.d[at] = -q.zv[at];
            }
            q.t[c] = solver_dot(q.zv + 3 * (size_t)c, q.res + 3 * (size_t)c, 3);
        }
        solver_tree_pad(q, lane, lanes);
        SOLVER_PAR_END
        double z_r = solver_tree(q.t, q.p2, false);
        if (!isfinite(z_r)) {
            status = SOLVER_NON_FINITE;
            break;
        }
        if (gn <= a.gradient_tol / sig2) {
            status = SOLVER_CONVERGED;
            break;
        }
        if (outer >= a.max_outer) break;
        ++outer;
        const double target = sqrt(z_r) * a.kappa_cg;
        double e_pe = 0.0, e_pd = 0.0, d_pd = z_r;
        bool on_boundary = false;
        for (int inner = 0; inner < inner_cap; ++inner) {
            const double d_hd = trec_hessian(q);
            ++happ;
            const double alpha = z_r / d_hd;
            const double e_pe_new = e_pe + 2.0 * alpha * e_pd + alpha * alpha * d_pd;
            if (!(d_hd > 0) || e_pe_new >= delta * delta) {
                const double tau = solver_boundary_tau(e_pe, e_pd, d_pd, delta);
                SOLVER_PAR_BEGIN
                for (int c = lane; c < n; c += lanes)
                    for (int i = 0; i < 3; ++i) {
                        const size_t at = 3 * (size_t)c + i;
                        q.eta[at] = q.eta[at] + tau * q.d[at], q.heta[at] = q.heta[at] + tau * q.hd[at];
                    }
                SOLVER_PAR_END
                on_boundary = true;
                break;
            }
            e_pe = e_pe_new;
            SOLVER_PAR_BEGIN
            for (int c = lane; c < n; c += lanes) {
                for (int i = 0; i < 3; ++i) {
                    const size_t at = 3 * (size_t)c + i;
                    q.eta[at] = q.eta[at] + alpha * q.d[at], q.heta[at] = q.heta[at] + alpha * q.hd[at];
                    q.res[at] = q.res[at] + alpha * q.hd[at];
                    q.zv[at] = c == anchor_c ? 0.0 : q.res[at] / q.m[c];
                }
                q.t[c] = solver_dot(q.zv + 3 * (size_t)c, q.res + 3 * (size_t)c, 3);
            }
            solver_tree_pad(q, lane, lanes);
            SOLVER_PAR_END
            const double zr_new = solver_tree(q.t, q.p2, false);
            if (sqrt(zr_new) <= target) break;
            const double beta = zr_new / z_r;
            SOLVER_PAR_BEGIN
            for (int c = lane; c < n; c += lanes)
                for (int i = 0; i < 3; ++i) {
                    const size_t at = 3 * (size_t)c + i;
                    q.d[at] = -q.zv[at] + beta * q.d[at];
                }
            SOLVER_PAR_END
            e_pd = beta * (e_pd + alpha * d_pd);
            d_pd = zr_new + beta * beta * d_pd;
            z_r = zr_new;
        }
        const double g_eta = solver_dot_nodes(q, q.g, q.eta, 3);
        const double model = g_eta + 0.5 * solver_dot_nodes(q, q.eta, q.heta, 3);
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes)
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                q.xn[at] = q.x[at] + q.eta[at];
            }
        SOLVER_PAR_END
        const double f_new = trec_pass(a, q, q.xn, q.gn, q.mn, q.entry_n);
        const double rho = solver_rho(f, f_new, model);
        bool small = false;
        if (rho > SOLVER_ACCEPT_RHO) {
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
        delta = solver_radius(delta, rho, on_boundary);
        if (small) {
            status = SOLVER_CONVERGED;
            gn = solver_inf_norm(q, q.g, 3);
        }
    }

    SOLVER_PAR_BEGIN
    if (status != SOLVER_NON_FINITE) {
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
    SOLVER_PAR_END
}

// ---- kernels ----

__global__ __launch_bounds__(SOLVER_THREADS) void trec_validate_kernel(TrecArgs a, long long n) {
    const long long i = (long long)blockIdx.x * SOLVER_THREADS + threadIdx.x;
    if (i < n) trec_validate(a, i);
}
// one workgroup per problem; every branch around a barrier is on a uniform value
__global__ __launch_bounds__(SOLVER_THREADS) void trec_solve_kernel(TrecArgs a) { trec_solve(a, (int)blockIdx.x); }

bool trec_sizes_ok(long long num_pairs, long long num_meas, long long num_images, long long num_tracks, long long max_tracks, long long num_problems) {
    return num_pairs >= 0 && num_meas >= 0 && num_images >= 0 && num_tracks >= 0 && max_tracks >= 0 && max_tracks <= num_tracks && num_problems >= 1 &&
           num_pairs + num_meas < TREC_MAX_ROWS && num_tracks < TREC_MAX_ROWS && num_images + max_tracks < TREC_MAX_NODES && num_problems < TREC_MAX_STATE &&
           num_problems * (num_images + max_tracks > 0 ? num_images + max_tracks : 1) < TREC_MAX_STATE;
}
bool trec_options_ok(double scale, double sigma, double huber_k, double init_tol, int init_cap, double delta0, double kappa_cg, double gradient_tol, double rel_tol,
                   double abs_tol, int max_outer, int max_inner) {
    return isfinite(scale) && scale > 0 && isfinite(sigma) && sigma > 0 && !(huber_k != huber_k) && init_tol >= 0 && init_cap >= 0 && delta0 > 0 && kappa_cg >= 0 &&
           gradient_tol >= 0 && rel_tol >= 0 && abs_tol >= 0 && max_outer >= 0 && max_inner >= 0;
}
// the longest run of measurements a validate lane index must cover
long long trec_validate_lanes(long long num_pairs, long long num_meas, long long num_tracks, long long num_problems) {
    long long n = num_pairs > num_meas ? num_pairs : num_meas;
    n = n > num_tracks ? n : num_tracks;
    n = n > num_problems ? n : num_problems;
    return n > 1 ? n : 1;
}

}  // namespace

extern "C" size_t gtsfm_translation_recovery_workspace_bytes(long long num_pairs, long long num_meas, long long num_images, long long num_tracks,
                                                             long long max_problem_tracks, long long num_problems) {
    if (!trec_sizes_ok(num_pairs, num_meas, num_images, num_tracks, max_problem_tracks, num_problems)) return 0;
    return trec_layout(nullptr, num_pairs, num_meas, num_images + max_problem_tracks, num_problems).bytes;
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
    GTSFM_CHECK_ARG(trec_sizes_ok(num_pairs, num_meas, num_images, num_tracks, max_problem_tracks, num_problems),
                    "%s: sizes out of range (%lld pairs, %lld measurements, %d images, %lld tracks, %lld per problem, %d problems)", me, num_pairs, num_meas, num_images,
                    num_tracks, max_problem_tracks, num_problems);
    const long long nodes = num_images + max_problem_tracks;
    GTSFM_CHECK_ARG(anchor >= -1 && (anchor < nodes || anchor == -1), "%s: the anchor %d is outside -1 .. %lld", me, anchor, nodes - 1);
    GTSFM_CHECK_ARG(trec_options_ok(scale_factor, sigma, huber_k, init_tol, init_max_iterations, delta0, kappa_cg, gradient_tol, rel_tol, abs_tol, max_outer, max_inner),
                    "%s: scale_factor, sigma and delta0 must be positive and finite, huber_k not NaN, no tolerance or cap negative", me);
    GTSFM_CHECK_ARG(workspace_dev && counters_dev && costs_dev && (nodes == 0 || (translation_out_dev && node_valid_dev)), "%s: null pointer", me);
    GTSFM_CHECK_ARG(num_pairs == 0 || (pair_images_dev && world_pair_dev), "%s: null pair pointer", me);
    GTSFM_CHECK_ARG(num_tracks == 0 || track_off_dev, "%s: %lld tracks without track_off_dev", me, num_tracks);
    GTSFM_CHECK_ARG(num_meas == 0 || (num_tracks > 0 && image_dev && world_meas_dev), "%s: %lld measurements without tracks, image_dev or world_meas_dev", me, num_meas);
    GTSFM_CHECK_ARG(problem_row_off_dev || (num_problems == 1 && max_problem_tracks == num_tracks),
                    "%s: without problem_row_off_dev there is one problem and max_problem_tracks is num_tracks", me);
    GTSFM_CHECK_ARG(((uintptr_t)workspace_dev & 255) == 0, "%s: the workspace must be aligned to 256 bytes", me);
    TrecArgs a{pair_images_dev, world_pair_dev, pair_enable_dev, track_off_dev, image_dev, world_meas_dev, meas_enable_dev, problem_row_off_dev, num_pairs, num_tracks, num_meas,
               num_images, (int)max_problem_tracks, num_problems, anchor, scale_factor, sigma, huber_k, init_tol, delta0, kappa_cg, gradient_tol, rel_tol, abs_tol,
               init_max_iterations, max_outer, max_inner, trec_layout(workspace_dev, num_pairs, num_meas, nodes, num_problems), translation_out_dev, node_valid_dev, counters_dev,
               costs_dev};
    if (workspace_bytes < a.w.bytes) {
        gtsfm_set_error("%s: workspace of %zu bytes, %zu needed for %lld rows, %lld nodes and %d problems", me, workspace_bytes, a.w.bytes, num_pairs + num_meas, nodes,
                        num_problems);
        return GTSFM_ERR_WORKSPACE;
    }
    const long long n = trec_validate_lanes(num_pairs, num_meas, num_tracks, num_problems);
    int flags[2] = {0, 0};
    const int rc = solver_launch(me, trec_validate_kernel, "trec_validate_kernel", a, a.w.flags, n, stream, flags);
    if (rc != GTSFM_OK) return rc;
    GTSFM_CHECK_ARG(!flags[0], "%s: an enabled pair row has i1 >= i2, or a row names an image outside 0 .. %d; nothing was written", me, num_images - 1);
    GTSFM_CHECK_ARG(!flags[1], "%s: track_off_dev or problem_row_off_dev is not ascending within its range, or a problem has more than %lld tracks; nothing was written", me,
                    max_problem_tracks);
    hipLaunchKernelGGL(trec_solve_kernel, dim3((unsigned)num_problems), dim3(SOLVER_THREADS), 0, stream, a);
    GTSFM_CHECK_LAUNCH("trec_solve_kernel");
    return GTSFM_OK;
}
