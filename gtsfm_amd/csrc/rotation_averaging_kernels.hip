// Rotation averaging on the device: the chordal cost sum_e kappa_e |R_i2 M_e - R_i1|_F^2 over SO(3)^n (Shonan's cost at p = 3), from a chordal
// initialisation, by a Riemannian trust region with Steihaug-Toint truncated CG and the exact Hessian. See include/gtsfm_amd.h; the
// specification is tests/rotation_averaging_reference.py, which this file follows operation for operation.
//
//   ra_validate_kernel : one lane per row: the validity byte, the refusal flags (a bad pair, bad problem offsets). The host reads the flags
//            here, before any output is written.
//   ra_solve_kernel    : ONE WORKGROUP PER PROBLEM runs everything else to the end, on the scaffold of problem_solver.h (the lane model,
//            the adjacency lists in the order the specification sums in, the anchor's component with compact ids, the scan and the tree).
//     stage A, B : lane l owns the compact nodes l, l + 256, ...; a node's sums run over its list in order; every global scalar (dot
//            products, norms, costs, the infinity norm) is the pairwise tree over the compact index padded to a power of two, done in
//            the workspace level by level. Hence no byte depends on the lane count, the run, or the problem's place in a batch. There is
//            no floating-point atomic, and nothing but + - * / sqrt (-ffp-contract=off): the Cayley retraction needs no libm.
//     All state lives in the workspace (528 bytes per node, L2-resident at these sizes).
// The host build of ra_validate and ra_solve is tools/rotation_averaging_host_main.cpp.

#include "../../include/gtsfm_amd.h"
#include "problem_solver.h"

#define RA_MAX_ROWS (1ll << 28)
#define RA_MAX_NODES (1ll << 24)
#define RA_MAX_STATE (1ll << 28)  // num_problems * num_images
#define RA_NODE_DOUBLES 66        // R, R', W, W', Lambda (9 each), six tangent vectors (3 each), the tree (2 per node, padded), one spare
#define RA_SVD_SWEEPS 30
#define RA_SVD_EPS 1e-15

namespace {

struct RaWorkspace {
    int* flags;      // [SOLVER_FLAG_WORDS]; 0: a bad pair row; 1: bad problem offsets
    uint8_t* valid;  // [E]
    SolverGraph g;   // over the images and the rows
    double* state;   // [P][RA_NODE_DOUBLES][N]
    size_t bytes;
};

RaWorkspace ra_layout(void* base, long long rows, long long images, long long problems) {
    RaWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t e = (size_t)rows, n = (size_t)images, p = (size_t)problems;
    w.flags = (int*)ws.take(SOLVER_FLAG_WORDS * 4);
    w.valid = (uint8_t*)ws.take(e);
    w.g = solver_carve(ws, e, n, p);
    w.state = (double*)ws.take(p * RA_NODE_DOUBLES * (n ? n : 1) * 8);
    w.bytes = ws.used;
    return w;
}

struct RaArgs {
    const int* pair_images;
    const double* rotation;
    const double* weight;
    const uint8_t* pair_enable;
    const long long* row_off;  // [P + 1] or null: one problem over every row
    long long num_rows;
    int num_images, num_problems, anchor;
    double chordal_tol, delta0, kappa_cg, theta, gradient_tol;
    int chordal_cap, max_outer, max_inner;
    RaWorkspace w;
    double* wri;          // [P][N][9]
    uint8_t* node_valid;  // [P][N]
    int* counters;        // [P][8]
    double* costs;        // [P][4]
};

GTSFM_HD bool ra_theta_ok(double theta) { return theta == 0.0 || theta == 0.5 || theta == 1.0 || theta == 2.0; }
GTSFM_HD double ra_theta_power(double x, double theta) { return theta == 1.0 ? x : theta == 0.5 ? sqrt(x) : theta == 2.0 ? x * x : 1.0; }

// ---- 3 x 3 arithmetic: every entry of a product is (a0 b0 + a1 b1) + a2 b2 ----

GTSFM_HD void ra_mm(const double* a, const double* b, double* c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
GTSFM_HD void ra_mmT(const double* a, const double* b, double* c) {  // a b^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1]) + a[3 * i + 2] * b[3 * j + 2];
}
GTSFM_HD void ra_mTm(const double* a, const double* b, double* c) {  // a^T b
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[i] * b[j] + a[3 + i] * b[3 + j]) + a[6 + i] * b[6 + j];
}
// R hat(xi)
GTSFM_HD void ra_hat_right(const double* r, const double* xi, double* v) {
    const double x = xi[0], y = xi[1], z = xi[2];
    for (int i = 0; i < 3; ++i) {
        v[3 * i] = r[3 * i + 1] * z - r[3 * i + 2] * y;
        v[3 * i + 1] = r[3 * i + 2] * x - r[3 * i] * z;
        v[3 * i + 2] = r[3 * i] * y - r[3 * i + 1] * x;
    }
}
// 4 vee(a)
GTSFM_HD void ra_vee4(const double* a, double* g) {
    g[0] = 2.0 * (a[7] - a[5]), g[1] = 2.0 * (a[2] - a[6]), g[2] = 2.0 * (a[3] - a[1]);
}
// the term of node k in (A L)_k for one list entry: A_k - A_j M where k is the row's i1, (A_k M - A_j) M^T where it is the i2
GTSFM_HD void ra_contrib(const double* ak, const double* aj, const double* m, int is_i1, double* c) {
    double t[9];
    if (is_i1) {
        ra_mm(aj, m, t);
        for (int i = 0; i < 9; ++i) c[i] = ak[i] - t[i];
    } else {
        ra_mm(ak, m, t);
        for (int i = 0; i < 9; ++i) t[i] = t[i] - aj[i];
        ra_mmT(t, m, c);
    }
}
GTSFM_HD void ra_cayley(const double* r, const double* xi, double* out) {
    const double h[3] = {0.5 * xi[0], 0.5 * xi[1], 0.5 * xi[2]};
    const double s = 2.0 / (1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]));
    const double hh[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
    double h2[9], q[9];
    ra_mm(hh, hh, h2);
    for (int i = 0; i < 9; ++i) q[i] = (i % 4 == 0 ? 1.0 : 0.0) + s * (hh[i] + h2[i]);
    ra_mm(r, q, out);
}
GTSFM_HD double ra_det3(const double* m) {
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// the closest rotation by a one-sided Jacobi SVD: U diag(s) V^T, s = 1 except sign(det U det V) at the smallest singular value
GTSFM_HD void ra_project_so3(const double* x, double* out) {
    double a[9], v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) a[i] = x[i];
    for (int sweep = 0; sweep < RA_SVD_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double al = (a[p] * a[p] + a[3 + p] * a[3 + p]) + a[6 + p] * a[6 + p];
            const double be = (a[q] * a[q] + a[3 + q] * a[3 + q]) + a[6 + q] * a[6 + q];
            const double ga = (a[p] * a[q] + a[3 + p] * a[3 + q]) + a[6 + p] * a[6 + q];
            if (fabs(ga) > RA_SVD_EPS * sqrt(al * be)) {
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t);
                const double s = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double ap = a[3 * i + p], aq = a[3 * i + q];
                    a[3 * i + p] = c * ap - s * aq, a[3 * i + q] = s * ap + c * aq;
                }
                for (int i = 0; i < 3; ++i) {
                    const double vp = v[3 * i + p], vq = v[3 * i + q];
                    v[3 * i + p] = c * vp - s * vq, v[3 * i + q] = s * vp + c * vq;
                }
                rotated = true;
            }
        }
        if (!rotated) break;
    }
    double sig[3], u[9];
    for (int j = 0; j < 3; ++j) sig[j] = sqrt((a[j] * a[j] + a[3 + j] * a[3 + j]) + a[6 + j] * a[6 + j]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) u[3 * i + j] = a[3 * i + j] / sig[j];
    const double d = ra_det3(u) * ra_det3(v);
    int jmin = 0;
    if (sig[1] < sig[jmin]) jmin = 1;
    if (sig[2] < sig[jmin]) jmin = 2;
    double sg[3] = {1.0, 1.0, 1.0};
    sg[jmin] = d < 0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (sg[0] * u[3 * i] * v[3 * j] + sg[1] * u[3 * i + 1] * v[3 * j + 1]) + sg[2] * u[3 * i + 2] * v[3 * j + 2];
}

// ---- the validity pass ----

GTSFM_HD void ra_validate(const RaArgs& a, long long m) {
    if (m < a.num_problems) {
        const long long lo = a.row_off ? a.row_off[m] : 0, hi = a.row_off ? a.row_off[m + 1] : a.num_rows;
        if (!(lo >= 0 && lo <= hi && hi <= a.num_rows)) a.w.flags[1] = 1;
    }
    if (m >= a.num_rows) return;
    uint8_t ok = 0;
    if (!a.pair_enable || a.pair_enable[m]) {
        const int i1 = a.pair_images[2 * m], i2 = a.pair_images[2 * m + 1];
        if (!(i1 >= 0 && i2 >= 0 && i1 < a.num_images && i2 < a.num_images && i1 != i2)) {
            a.w.flags[0] = 1;
        } else {
            const double kappa = a.weight[m];
            bool fin = isfinite(kappa) && kappa > 0;
            for (int i = 0; i < 9; ++i) fin = fin && isfinite(a.rotation[9 * m + i]);
            ok = fin ? 1 : 0;
        }
    }
    a.w.valid[m] = ok;
}

// ---- the per-problem state ----

struct RaProblem : SolverGraph {
    long long lo, hi;  // the problem's rows
    double *r, *rn, *w, *wn, *lam, *g, *eta, *heta, *res, *d, *hd;
};

// dst_k = (src L)_k over k's list, kappa = 1 when not weighted; the anchor's block is zero when zero_anchor
GTSFM_HD void ra_apply(const RaArgs& a, const RaProblem& q, const double* src, double* dst, bool weighted, bool zero_anchor) {
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, term[9];
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int e2 = q.adj_row[j];
            const long long row = e2 >> 1;
            const double kappa = weighted ? a.weight[row] : 1.0;
            ra_contrib(src + 9 * (size_t)c, src + 9 * (size_t)q.adj_nbr[j], a.rotation + 9 * row, e2 & 1, term);
            for (int i = 0; i < 9; ++i) acc[i] = acc[i] + kappa * term[i];
        }
        for (int i = 0; i < 9; ++i) dst[9 * (size_t)c + i] = zero_anchor && c == q.anchor_c ? 0.0 : acc[i];
    }
    SOLVER_PAR_END
}

// W = Y L at `r` into `w`, and the cost 0.5 * tree(per-node sums of kappa |residual|^2)
GTSFM_HD double ra_pass(const RaArgs& a, const RaProblem& q, const double* r, double* w) {
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, cost = 0.0, res[9], term[9], t[9];
        const double* rk = r + 9 * (size_t)c;
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int e2 = q.adj_row[j];
            const long long row = e2 >> 1;
            const double kappa = a.weight[row], *m = a.rotation + 9 * row, *rj = r + 9 * (size_t)q.adj_nbr[j];
            if (e2 & 1) {
                ra_mm(rj, m, t);
                for (int i = 0; i < 9; ++i) res[i] = rk[i] - t[i];
                for (int i = 0; i < 9; ++i) term[i] = res[i];
            } else {
                ra_mm(rk, m, t);
                for (int i = 0; i < 9; ++i) res[i] = t[i] - rj[i];
                ra_mmT(res, m, term);
            }
            for (int i = 0; i < 9; ++i) acc[i] = acc[i] + kappa * term[i];
            cost = cost + kappa * solver_dot(res, res, 9);
        }
        for (int i = 0; i < 9; ++i) w[9 * (size_t)c + i] = acc[i];
        q.t[c] = cost;
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    return 0.5 * solver_tree(q.t, q.p2, false);
}

// hd = H[d] at (r, lam), the anchor's block zero; returns <d, hd>
GTSFM_HD double ra_hessian(const RaArgs& a, const RaProblem& q) {
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, vk[9], vj[9], term[9], b[9], a2[9];
        const double* rk = q.r + 9 * (size_t)c;
        ra_hat_right(rk, q.d + 3 * (size_t)c, vk);
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const int e2 = q.adj_row[j], nb = q.adj_nbr[j];
            const long long row = e2 >> 1;
            const double kappa = a.weight[row];
            ra_hat_right(q.r + 9 * (size_t)nb, q.d + 3 * (size_t)nb, vj);
            ra_contrib(vk, vj, a.rotation + 9 * row, e2 & 1, term);
            for (int i = 0; i < 9; ++i) acc[i] = acc[i] + kappa * term[i];
        }
        ra_mm(vk, q.lam + 9 * (size_t)c, term);
        for (int i = 0; i < 9; ++i) b[i] = acc[i] - term[i];
        ra_mTm(rk, b, a2);
        double* hd = q.hd + 3 * (size_t)c;
        ra_vee4(a2, hd);
        if (c == q.anchor_c) hd[0] = hd[1] = hd[2] = 0.0;
        q.t[c] = solver_dot(q.d + 3 * (size_t)c, hd, 3);
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    return solver_tree(q.t, q.p2, false);
}

// ---- one problem, start to end ----

GTSFM_HD void ra_solve(const RaArgs& a, int p) {
    const int N = a.num_images;
    RaProblem q;
    q.lo = a.row_off ? a.row_off[p] : 0, q.hi = a.row_off ? a.row_off[p + 1] : a.num_rows;
    static_cast<SolverGraph&>(q) = solver_slice(a.w.g, p, N, (size_t)q.lo);
    double* wri = a.wri + 9 * (size_t)p * N;
    uint8_t* node_valid = a.node_valid + (size_t)p * N;
    int* counters = a.counters + 8 * (size_t)p;
    double* costs = a.costs + 4 * (size_t)p;
    const double nan = __builtin_nan("");

    // the outputs' defaults
    SOLVER_PAR_BEGIN
    solver_clear(q, N, lane, lanes);
    for (int i = lane; i < N; i += lanes) {
        node_valid[i] = 0;
        for (int k = 0; k < 9; ++k) wri[9 * (size_t)i + k] = nan;
    }
    for (int i = lane; i < 8; i += lanes) counters[i] = 0;
    for (int i = lane; i < 4; i += lanes) costs[i] = nan;
    SOLVER_PAR_END

    // the lists over the problem's rows: a row's a is its i1, its b the i2
    const int rows = (int)(q.hi - q.lo);
    int total = 0;
    const int first = solver_build_lists(
        q, N, rows, [&](int l, int* i1, int* i2) { *i1 = a.pair_images[2 * (q.lo + l)], *i2 = a.pair_images[2 * (q.lo + l) + 1]; },
        [&](int l) { return a.w.valid[q.lo + l] != 0; }, &total);
    if (first >= rows) {
        SOLVER_PAR_BEGIN
        if (lane == 0) counters[0] = SOLVER_NO_VALID_ROW, counters[6] = a.anchor;
        SOLVER_PAR_END
        return;
    }
    const int anchor = a.anchor >= 0 ? a.anchor : a.pair_images[2 * (q.lo + first) + 1];
    solver_component(q, anchor, N);
    const int n = q.n, anchor_c = q.anchor_c;
    SOLVER_PAR_BEGIN  // adj_row holds the row within the problem: rebase it to the row of the call
    for (int c = lane; c < n; c += lanes) {
        const int node = q.cnode[c];
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) q.adj_row[j] = q.adj_row[j] + 2 * (int)q.lo;
    }
    SOLVER_PAR_END

    double* base = a.w.state + (size_t)p * RA_NODE_DOUBLES * (size_t)N;
    const size_t sn = (size_t)N;
    q.r = base, q.rn = base + 9 * sn, q.w = base + 18 * sn, q.wn = base + 27 * sn, q.lam = base + 36 * sn;
    q.g = base + 45 * sn, q.eta = base + 48 * sn, q.heta = base + 51 * sn, q.res = base + 54 * sn, q.d = base + 57 * sn, q.hd = base + 60 * sn;
    q.t = base + 63 * sn;  // p2 < 2 n <= 2 N, and one spare N

    // the largest weight, and the cost with every rotation the identity
    SOLVER_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        const int node = q.cnode[c];
        double best = 0.0;
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const double kappa = a.weight[q.adj_row[j] >> 1];
            best = kappa > best ? kappa : best;
        }
        q.t[c] = best;
        for (int i = 0; i < 9; ++i) q.r[9 * (size_t)c + i] = i % 4 == 0 ? 1.0 : 0.0;
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    const double max_kappa = solver_tree(q.t, q.p2, true);
    const double initial_cost = ra_pass(a, q, q.r, q.w);

    // stage A: CG on the reduced connection Laplacian from X = 0; x = rn, residual = w, direction = wn, L p = lam
    double *x = q.rn, *cr = q.w, *cp = q.wn, *cap = q.lam;
    SOLVER_PAR_BEGIN
    for (int c = lane; c < n; c += lanes)
        for (int i = 0; i < 9; ++i) q.r[9 * (size_t)c + i] = c == anchor_c && i % 4 == 0 ? 1.0 : 0.0;
    SOLVER_PAR_END
    ra_apply(a, q, q.r, cap, false, false);
    SOLVER_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        for (int i = 0; i < 9; ++i) {
            const size_t at = 9 * (size_t)c + i;
            cr[at] = c == anchor_c ? 0.0 : -cap[at];
            cp[at] = cr[at], x[at] = 0.0;
        }
        q.t[c] = solver_dot(cr + 9 * (size_t)c, cr + 9 * (size_t)c, 9);
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    double rr = solver_tree(q.t, q.p2, false);
    const double rr0 = rr;
    int chordal_steps = 0;
    while (chordal_steps < a.chordal_cap && rr > (a.chordal_tol * a.chordal_tol) * rr0) {
        ra_apply(a, q, cp, cap, false, true);
        const double pap = solver_dot_nodes(q, cp, cap, 9);
        if (!(pap > 0)) break;
        const double alpha = rr / pap;
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) {
            for (int i = 0; i < 9; ++i) {
                const size_t at = 9 * (size_t)c + i;
                x[at] = x[at] + alpha * cp[at];
                cr[at] = cr[at] - alpha * cap[at];
            }
            q.t[c] = solver_dot(cr + 9 * (size_t)c, cr + 9 * (size_t)c, 9);
        }
        solver_tree_pad(q, lane, lanes);
        SOLVER_PAR_END
        const double rr_new = solver_tree(q.t, q.p2, false);
        const double beta = rr_new / rr;
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes)
            for (int i = 0; i < 9; ++i) {
                const size_t at = 9 * (size_t)c + i;
                cp[at] = cr[at] + beta * cp[at];
            }
        SOLVER_PAR_END
        rr = rr_new;
        ++chordal_steps;
    }
    SOLVER_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        if (c == anchor_c)
            for (int i = 0; i < 9; ++i) x[9 * (size_t)c + i] = i % 4 == 0 ? 1.0 : 0.0;
        ra_project_so3(x + 9 * (size_t)c, q.r + 9 * (size_t)c);
    }
    SOLVER_PAR_END

    // stage B
    double f = ra_pass(a, q, q.r, q.w);
    const double chordal_cost = f;
    int status = isfinite(f) ? SOLVER_MAX_ITERATIONS : SOLVER_NON_FINITE;
    const int inner_cap = a.max_inner > 0 ? a.max_inner : 3 * n;
    double delta = a.delta0, gn = nan;
    int outer = 0, accepted = 0, happ = 0;
    while (status == SOLVER_MAX_ITERATIONS) {
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) {
            double aa[9];
            ra_mTm(q.r + 9 * (size_t)c, q.w + 9 * (size_t)c, aa);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) q.lam[9 * (size_t)c + 3 * i + j] = 0.5 * (aa[3 * i + j] + aa[3 * j + i]);
            double* g = q.g + 3 * (size_t)c;
            ra_vee4(aa, g);
            if (c == anchor_c) g[0] = g[1] = g[2] = 0.0;
            const double m01 = fabs(g[0]) > fabs(g[1]) ? fabs(g[0]) : fabs(g[1]);
            q.t[c] = m01 > fabs(g[2]) ? m01 : fabs(g[2]);
        }
        solver_tree_pad(q, lane, lanes);
        SOLVER_PAR_END
        gn = solver_tree(q.t, q.p2, true);
        double r_r = solver_dot_nodes(q, q.g, q.g, 3);
        if (!isfinite(r_r)) {
            status = SOLVER_NON_FINITE;
            break;
        }
        if (gn <= a.gradient_tol * max_kappa) {
            status = SOLVER_CONVERGED;
            break;
        }
        if (outer >= a.max_outer) break;
        ++outer;
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes)
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                q.eta[at] = 0.0, q.heta[at] = 0.0, q.res[at] = q.g[at], q.d[at] = -q.g[at];
            }
        SOLVER_PAR_END
        const double norm_r0 = sqrt(r_r);
        const double power = ra_theta_power(norm_r0, a.theta);
        const double target = norm_r0 * (a.kappa_cg < power ? a.kappa_cg : power);
        double e_pe = 0.0, e_pd = 0.0, d_pd = r_r;
        bool on_boundary = false;
        for (int inner = 0; inner < inner_cap; ++inner) {
            const double d_hd = ra_hessian(a, q);
            ++happ;
            const double alpha = r_r / d_hd;
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
                }
                q.t[c] = solver_dot(q.res + 3 * (size_t)c, q.res + 3 * (size_t)c, 3);
            }
            solver_tree_pad(q, lane, lanes);
            SOLVER_PAR_END
            const double rr_new = solver_tree(q.t, q.p2, false);
            if (sqrt(rr_new) <= target) break;
            const double beta = rr_new / r_r;
            SOLVER_PAR_BEGIN
            for (int c = lane; c < n; c += lanes)
                for (int i = 0; i < 3; ++i) {
                    const size_t at = 3 * (size_t)c + i;
                    q.d[at] = -q.res[at] + beta * q.d[at];
                }
            SOLVER_PAR_END
            e_pd = beta * (e_pd + alpha * d_pd);
            d_pd = rr_new + beta * beta * d_pd;
            r_r = rr_new;
        }
        const double g_eta = solver_dot_nodes(q, q.g, q.eta, 3);
        const double model = g_eta + 0.5 * solver_dot_nodes(q, q.eta, q.heta, 3);
        SOLVER_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) ra_cayley(q.r + 9 * (size_t)c, q.eta + 3 * (size_t)c, q.rn + 9 * (size_t)c);
        SOLVER_PAR_END
        const double f_new = ra_pass(a, q, q.rn, q.wn);
        const double rho = solver_rho(f, f_new, model);
        if (rho > SOLVER_ACCEPT_RHO) {
            double* s = q.r;
            q.r = q.rn, q.rn = s;
            s = q.w, q.w = q.wn, q.wn = s;
            f = f_new;
            ++accepted;
        }
        delta = solver_radius(delta, rho, on_boundary);
    }

    SOLVER_PAR_BEGIN
    if (status != SOLVER_NON_FINITE) {
        for (int c = lane; c < n; c += lanes) {
            double* out = wri + 9 * (size_t)q.cnode[c];
            ra_mTm(q.r + 9 * (size_t)anchor_c, q.r + 9 * (size_t)c, out);
            if (c == anchor_c)
                for (int i = 0; i < 9; ++i) out[i] = i % 4 == 0 ? 1.0 : 0.0;
            node_valid[q.cnode[c]] = 1;
        }
    }
    if (lane == 0) {
        const int valid_rows = total / 2;  // the lists hold every valid row twice
        counters[0] = status, counters[1] = outer, counters[2] = accepted, counters[3] = happ, counters[4] = chordal_steps, counters[5] = n;
        counters[6] = anchor, counters[7] = valid_rows;
        costs[0] = initial_cost, costs[1] = chordal_cost, costs[2] = f, costs[3] = gn;
    }
    SOLVER_PAR_END
}

// ---- kernels ----

__global__ __launch_bounds__(SOLVER_THREADS) void ra_validate_kernel(RaArgs a, long long n) {
    const long long i = (long long)blockIdx.x * SOLVER_THREADS + threadIdx.x;
    if (i < n) ra_validate(a, i);
}
// one workgroup per problem; every branch around a barrier is on a uniform value
__global__ __launch_bounds__(SOLVER_THREADS) void ra_solve_kernel(RaArgs a) { ra_solve(a, (int)blockIdx.x); }

bool ra_sizes_ok(long long num_rows, long long num_images, long long num_problems) {
    return num_rows >= 0 && num_images >= 0 && num_problems >= 1 && num_rows < RA_MAX_ROWS && num_images < RA_MAX_NODES && num_problems < RA_MAX_STATE &&
           num_problems * (num_images > 0 ? num_images : 1) < RA_MAX_STATE;
}

}  // namespace

extern "C" size_t gtsfm_rotation_averaging_workspace_bytes(long long num_rows, long long num_images, long long num_problems) {
    if (!ra_sizes_ok(num_rows, num_images, num_problems)) return 0;
    return ra_layout(nullptr, num_rows, num_images, num_problems).bytes;
}

extern "C" int gtsfm_rotation_averaging_f64(const int32_t* pair_images_dev, const double* rotation_dev, const double* weight_dev, const uint8_t* pair_enable_dev,
                                            long long num_rows, int num_images, const long long* problem_row_off_dev, int num_problems, int anchor,
                                            double chordal_tol, int chordal_max_iterations, double delta0, double kappa_cg, double theta, double gradient_tol,
                                            int max_outer, int max_inner, void* workspace_dev, size_t workspace_bytes, double* rotation_out_dev,
                                            uint8_t* node_valid_dev, int32_t* counters_dev, double* costs_dev, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* me = "gtsfm_rotation_averaging_f64";
    GTSFM_CHECK_ARG(ra_sizes_ok(num_rows, num_images, num_problems), "%s: sizes out of range (%lld rows, %d images, %d problems)", me, num_rows, num_images, num_problems);
    GTSFM_CHECK_ARG(anchor >= -1 && (anchor < num_images || anchor == -1), "%s: the anchor %d is outside -1 .. %d", me, anchor, num_images - 1);
    GTSFM_CHECK_ARG(ra_theta_ok(theta), "%s: theta must be one of 0, 0.5, 1, 2 (no libm on the device), got %g", me, theta);
    GTSFM_CHECK_ARG(chordal_tol >= 0 && chordal_max_iterations >= 0 && delta0 > 0 && kappa_cg >= 0 && gradient_tol >= 0 && max_outer >= 0 && max_inner >= 0,
                    "%s: a negative tolerance or cap, or delta0 <= 0", me);
    GTSFM_CHECK_ARG(workspace_dev && counters_dev && costs_dev && (num_images == 0 || (rotation_out_dev && node_valid_dev)), "%s: null pointer", me);
    GTSFM_CHECK_ARG(num_rows == 0 || (pair_images_dev && rotation_dev && weight_dev), "%s: null row pointer", me);
    GTSFM_CHECK_ARG(num_problems == 1 || problem_row_off_dev, "%s: %d problems without problem_row_off_dev", me, num_problems);
    GTSFM_CHECK_ARG(((uintptr_t)workspace_dev & 255) == 0, "%s: the workspace must be aligned to 256 bytes", me);
    RaArgs a{pair_images_dev, rotation_dev, weight_dev, pair_enable_dev, problem_row_off_dev, num_rows, num_images, num_problems, anchor, chordal_tol, delta0, kappa_cg, theta,
             gradient_tol, chordal_max_iterations, max_outer, max_inner, ra_layout(workspace_dev, num_rows, num_images, num_problems), rotation_out_dev, node_valid_dev,
             counters_dev, costs_dev};
    if (workspace_bytes < a.w.bytes) {
        gtsfm_set_error("%s: workspace of %zu bytes, %zu needed for %lld rows, %d images and %d problems", me, workspace_bytes, a.w.bytes, num_rows, num_images, num_problems);
        return GTSFM_ERR_WORKSPACE;
    }
    const long long n = num_rows > num_problems ? num_rows : num_problems;
    int flags[2] = {0, 0};
    const int rc = solver_launch(me, ra_validate_kernel, "ra_validate_kernel", a, a.w.flags, n, stream, flags);
    if (rc != GTSFM_OK) return rc;
    GTSFM_CHECK_ARG(!flags[0], "%s: an enabled row has i1 == i2 or names an image outside 0 .. %d; nothing was written", me, num_images - 1);
    GTSFM_CHECK_ARG(!flags[1], "%s: problem_row_off_dev is not ascending within 0 .. %lld; nothing was written", me, num_rows);
    hipLaunchKernelGGL(ra_solve_kernel, dim3((unsigned)num_problems), dim3(SOLVER_THREADS), 0, stream, a);
    GTSFM_CHECK_LAUNCH("ra_solve_kernel");
    return GTSFM_OK;
}
