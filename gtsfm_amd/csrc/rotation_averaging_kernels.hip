// Rotation averaging on the device: the chordal cost sum_e kappa_e |R_i2 M_e - R_i1|_F^2 over SO(3)^n (Shonan's cost at p = 3), from a chordal
// initialisation, by a Riemannian trust region with Steihaug-Toint truncated CG and the exact Hessian. See include/gtsfm_amd.h; the
// specification is tests/rotation_averaging_reference.py, which this file follows operation for operation.
//
//   ra_validate_kernel : one lane per row: the validity byte, the refusal flags (a bad pair, bad problem offsets). The host reads the flags
//            here, before any output is written.
//   ra_solve_kernel    : ONE WORKGROUP PER PROBLEM runs everything else to the end.
//     adjacency  : degrees by integer atomics, a blocked scan, an arbitrary slot per entry (atomic cursor), then every entry is ranked
//            within its node's list by (neighbour, row) and moved to its place: the lists are in the order the specification sums in.
//     component  : labels spread from the anchor until a round changes nothing (at most num_images rounds); its nodes get compact ids in
//            ascending image id and the lists are renumbered.
//     stage A, B : lane l owns the compact nodes l, l + 256, ...; a node's sums run over its list in order; every global scalar (dot
//            products, norms, costs, the infinity norm) is the pairwise tree over the compact index padded to a power of two, done in
//            the workspace level by level. Hence no byte depends on the lane count, the run, or the problem's place in a batch. There is
//            no floating-point atomic, and nothing but + - * / sqrt (-ffp-contract=off): the Cayley retraction needs no libm.
//     Every loop has a cap that is an argument or a size; no loop waits on a value another lane may never write. All state lives in the
//     workspace (528 bytes per node, L2-resident at these sizes).
// The solver is ONE function for the device and the host: a section between RA_PAR_BEGIN and RA_PAR_END is run by every lane and ends
// with a barrier; on the host (tools/rotation_averaging_host_main.cpp) it is a loop over the lanes, in either order and with any lane
// count, and the atomics are plain updates. Scalars that steer the control flow are read from memory after a barrier: they are uniform.

#include <math.h>

#include "../../include/gtsfm_amd.h"
#include "graph_prims.h"

#define RA_HD __host__ __device__ __forceinline__
#define RA_THREADS 256
#define RA_MAX_ROWS (1ll << 28)
#define RA_MAX_NODES (1ll << 24)
#define RA_MAX_STATE (1ll << 28)  // num_problems * num_images
#define RA_FLAG_WORDS 8           // 0: a bad pair row; 1: bad problem offsets
#define RA_NODE_DOUBLES 66        // R, R', W, W', Lambda (9 each), six tangent vectors (3 each), the tree (2 per node, padded), one spare
#define RA_SVD_SWEEPS 30
#define RA_SVD_EPS 1e-15
#define RA_RHO_REG (1e3 * 2.220446049250313e-16)
#define RA_CONVERGED 0
#define RA_MAX_ITERATIONS 1
#define RA_NO_VALID_ROW 2
#define RA_NON_FINITE 3

struct RaHostLanes {  // the host build's lane count and order (tools/rotation_averaging_host_main.cpp)
    int lanes, descending;
};
static RaHostLanes ra_host = {1, 0};

#if defined(__HIP_DEVICE_COMPILE__)
#define RA_PAR_BEGIN                  \
    {                                 \
        const int lane = threadIdx.x; \
        const int lanes = RA_THREADS; \
        (void)lane, (void)lanes;
#define RA_PAR_END   \
    }                \
    __syncthreads();
#else
#define RA_PAR_BEGIN                                      \
    for (int ra_l = 0; ra_l < ra_host.lanes; ++ra_l) {    \
        const int lanes = ra_host.lanes;                  \
        const int lane = ra_host.descending ? lanes - 1 - ra_l : ra_l; \
        (void)lane, (void)lanes;
#define RA_PAR_END }
#endif

namespace {

struct RaWorkspace {
    int* flags;         // [RA_FLAG_WORDS]
    uint8_t* valid;     // [E]
    int *off, *cid;     // [P][N + 2]: list offsets by image; compact ids (an exclusive scan of the reach flags)
    int *cursor, *reach, *cnode;  // [P][N]
    long long* lanebuf; // [P][RA_THREADS]
    int *raw_row, *raw_owner, *adj_nbr, *adj_row;  // [2 E]; a problem's slice starts at twice its first row
    double* state;      // [P][RA_NODE_DOUBLES][N]
    size_t bytes;
};

RaWorkspace ra_layout(void* base, long long rows, long long images, long long problems) {
    RaWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t e = (size_t)rows, n = (size_t)images, p = (size_t)problems;
    w.flags = (int*)ws.take(RA_FLAG_WORDS * 4);
    w.valid = (uint8_t*)ws.take(e);
    w.off = (int*)ws.take(p * (n + 2) * 4);
    w.cid = (int*)ws.take(p * (n + 2) * 4);
    w.cursor = (int*)ws.take(p * n * 4);
    w.reach = (int*)ws.take(p * n * 4);
    w.cnode = (int*)ws.take(p * n * 4);
    w.lanebuf = (long long*)ws.take(p * RA_THREADS * 8);
    w.raw_row = (int*)ws.take(2 * e * 4);
    w.raw_owner = (int*)ws.take(2 * e * 4);
    w.adj_nbr = (int*)ws.take(2 * e * 4);
    w.adj_row = (int*)ws.take(2 * e * 4);
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

RA_HD bool ra_theta_ok(double theta) { return theta == 0.0 || theta == 0.5 || theta == 1.0 || theta == 2.0; }
RA_HD double ra_theta_power(double x, double theta) { return theta == 1.0 ? x : theta == 0.5 ? sqrt(x) : theta == 2.0 ? x * x : 1.0; }

// ---- 3 x 3 arithmetic: every entry of a product is (a0 b0 + a1 b1) + a2 b2 ----

RA_HD void ra_mm(const double* a, const double* b, double* c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
RA_HD void ra_mmT(const double* a, const double* b, double* c) {  // a b^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1]) + a[3 * i + 2] * b[3 * j + 2];
}
RA_HD void ra_mTm(const double* a, const double* b, double* c) {  // a^T b
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[i] * b[j] + a[3 + i] * b[3 + j]) + a[6 + i] * b[6 + j];
}
RA_HD double ra_dot(const double* a, const double* b, int k) {
    double s = a[0] * b[0];
    for (int i = 1; i < k; ++i) s = s + a[i] * b[i];
    return s;
}
// R hat(xi)
RA_HD void ra_hat_right(const double* r, const double* xi, double* v) {
    const double x = xi[0], y = xi[1], z = xi[2];
    for (int i = 0; i < 3; ++i) {
        v[3 * i] = r[3 * i + 1] * z - r[3 * i + 2] * y;
        v[3 * i + 1] = r[3 * i + 2] * x - r[3 * i] * z;
        v[3 * i + 2] = r[3 * i] * y - r[3 * i + 1] * x;
    }
}
// 4 vee(a)
RA_HD void ra_vee4(const double* a, double* g) {
    g[0] = 2.0 * (a[7] - a[5]), g[1] = 2.0 * (a[2] - a[6]), g[2] = 2.0 * (a[3] - a[1]);
}
// the term of node k in (A L)_k for one list entry: A_k - A_j M where k is the row's i1, (A_k M - A_j) M^T where it is the i2
RA_HD void ra_contrib(const double* ak, const double* aj, const double* m, int is_i1, double* c) {
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
RA_HD void ra_cayley(const double* r, const double* xi, double* out) {
    const double h[3] = {0.5 * xi[0], 0.5 * xi[1], 0.5 * xi[2]};
    const double s = 2.0 / (1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]));
    const double hh[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
    double h2[9], q[9];
    ra_mm(hh, hh, h2);
    for (int i = 0; i < 9; ++i) q[i] = (i % 4 == 0 ? 1.0 : 0.0) + s * (hh[i] + h2[i]);
    ra_mm(r, q, out);
}
RA_HD double ra_det3(const double* m) {
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// the closest rotation by a one-sided Jacobi SVD: U diag(s) V^T, s = 1 except sign(det U det V) at the smallest singular value
RA_HD void ra_project_so3(const double* x, double* out) {
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

RA_HD void ra_validate(const RaArgs& a, long long m) {
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

struct RaProblem {
    long long lo, hi;  // the problem's rows
    int n, p2, anchor_c;
    int *off, *cid, *cursor, *reach, *cnode, *raw_row, *raw_owner, *adj_nbr, *adj_row;
    long long* lanebuf;
    double *r, *rn, *w, *wn, *lam, *g, *eta, *heta, *res, *d, *hd, *t;
};

// val[0 .. n) -> its exclusive prefix sum in place, val[n] = the total: every lane a contiguous chunk
RA_HD void ra_scan(int* val, int n, long long* lanebuf) {
    RA_PAR_BEGIN
    const int chunk = (n + lanes - 1) / lanes, from = lane * chunk < n ? lane * chunk : n, to = from + chunk < n ? from + chunk : n;
    long long s = 0;
    for (int i = from; i < to; ++i) s += val[i];
    lanebuf[lane] = s;
    RA_PAR_END
    RA_PAR_BEGIN
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
    RA_PAR_END
}

// the tree over t[0 .. p2): t[i] = t[i] (+ or max) t[i + s] level by level; the result is uniform
RA_HD double ra_tree(double* t, int p2, bool take_max) {
    for (long long s = 1; s < p2; s <<= 1) {
        RA_PAR_BEGIN
        for (long long i = (long long)lane * 2 * s; i < p2; i += (long long)lanes * 2 * s) {
            const double x = t[i], y = t[i + s];
            t[i] = take_max ? (x > y ? x : y) : x + y;
        }
        RA_PAR_END
    }
    double out = 0.0;
    RA_PAR_BEGIN
    out = t[0];
    RA_PAR_END
    return out;
}
RA_HD void ra_tree_pad(const RaProblem& q, int lane, int lanes) {
    for (int c = q.n + lane; c < q.p2; c += lanes) q.t[c] = 0.0;
}

// dst_k = (src L)_k over k's list, kappa = 1 when not weighted; the anchor's block is zero when zero_anchor
RA_HD void ra_apply(const RaArgs& a, const RaProblem& q, const double* src, double* dst, bool weighted, bool zero_anchor) {
    RA_PAR_BEGIN
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
    RA_PAR_END
}

// W = Y L at `r` into `w`, and the cost 0.5 * tree(per-node sums of kappa |residual|^2)
RA_HD double ra_pass(const RaArgs& a, const RaProblem& q, const double* r, double* w) {
    RA_PAR_BEGIN
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
            cost = cost + kappa * ra_dot(res, res, 9);
        }
        for (int i = 0; i < 9; ++i) w[9 * (size_t)c + i] = acc[i];
        q.t[c] = cost;
    }
    ra_tree_pad(q, lane, lanes);
    RA_PAR_END
    return 0.5 * ra_tree(q.t, q.p2, false);
}

// <x, y> over the nodes, k numbers per node
RA_HD double ra_dot_nodes(const RaProblem& q, const double* x, const double* y, int k) {
    RA_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) q.t[c] = ra_dot(x + k * (size_t)c, y + k * (size_t)c, k);
    ra_tree_pad(q, lane, lanes);
    RA_PAR_END
    return ra_tree(q.t, q.p2, false);
}

// hd = H[d] at (r, lam), the anchor's block zero; returns <d, hd>
RA_HD double ra_hessian(const RaArgs& a, const RaProblem& q) {
    RA_PAR_BEGIN
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
        q.t[c] = ra_dot(q.d + 3 * (size_t)c, hd, 3);
    }
    ra_tree_pad(q, lane, lanes);
    RA_PAR_END
    return ra_tree(q.t, q.p2, false);
}

// ---- one problem, start to end ----

RA_HD void ra_solve(const RaArgs& a, int p) {
    const int N = a.num_images;
    RaProblem q;
    q.lo = a.row_off ? a.row_off[p] : 0, q.hi = a.row_off ? a.row_off[p + 1] : a.num_rows;
    q.off = a.w.off + (size_t)p * (N + 2), q.cid = a.w.cid + (size_t)p * (N + 2);
    q.cursor = a.w.cursor + (size_t)p * N, q.reach = a.w.reach + (size_t)p * N, q.cnode = a.w.cnode + (size_t)p * N;
    q.lanebuf = a.w.lanebuf + (size_t)p * RA_THREADS;
    q.raw_row = a.w.raw_row + 2 * q.lo, q.raw_owner = a.w.raw_owner + 2 * q.lo, q.adj_nbr = a.w.adj_nbr + 2 * q.lo, q.adj_row = a.w.adj_row + 2 * q.lo;
    double* wri = a.wri + 9 * (size_t)p * N;
    uint8_t* node_valid = a.node_valid + (size_t)p * N;
    int* counters = a.counters + 8 * (size_t)p;
    double* costs = a.costs + 4 * (size_t)p;
    const double nan = __builtin_nan("");

    // the outputs' defaults, the degrees, the first valid row
    RA_PAR_BEGIN
    for (int i = lane; i < N + 2; i += lanes) q.off[i] = 0, q.cid[i] = 0;
    for (int i = lane; i < N; i += lanes) {
        q.cursor[i] = 0, q.reach[i] = 0, node_valid[i] = 0;
        for (int k = 0; k < 9; ++k) wri[9 * (size_t)i + k] = nan;
    }
    for (int i = lane; i < 8; i += lanes) counters[i] = 0;
    for (int i = lane; i < 4; i += lanes) costs[i] = nan;
    RA_PAR_END
    RA_PAR_BEGIN
    long long first = q.hi;
    for (long long m = q.lo + lane; m < q.hi; m += lanes) {
        if (!a.w.valid[m]) continue;
        hd_atomic_add(&q.off[a.pair_images[2 * m]], 1);
        hd_atomic_add(&q.off[a.pair_images[2 * m + 1]], 1);
        if (m < first) first = m;
    }
    q.lanebuf[lane] = first;
    RA_PAR_END
    long long first = q.hi;
    RA_PAR_BEGIN
    first = q.hi;
    for (int l = 0; l < lanes; ++l) first = q.lanebuf[l] < first ? q.lanebuf[l] : first;
    RA_PAR_END
    ra_scan(q.off, N, q.lanebuf);
    int total = 0;
    RA_PAR_BEGIN
    total = q.off[N];
    RA_PAR_END
    if (first >= q.hi) {
        RA_PAR_BEGIN
        if (lane == 0) counters[0] = RA_NO_VALID_ROW, counters[6] = a.anchor;
        RA_PAR_END
        return;
    }
    const int anchor = a.anchor >= 0 ? a.anchor : a.pair_images[2 * first + 1];

    // the lists: a slot each, then every entry to its rank by (neighbour, row)
    RA_PAR_BEGIN
    for (long long m = q.lo + lane; m < q.hi; m += lanes) {
        if (!a.w.valid[m]) continue;
        const int i1 = a.pair_images[2 * m], i2 = a.pair_images[2 * m + 1];
        const int s1 = q.off[i1] + hd_atomic_add(&q.cursor[i1], 1), s2 = q.off[i2] + hd_atomic_add(&q.cursor[i2], 1);
        if (s1 < q.off[i1 + 1]) q.raw_row[s1] = (int)(m - q.lo), q.raw_owner[s1] = i1;  // always true: exactly degree rows ask
        if (s2 < q.off[i2 + 1]) q.raw_row[s2] = (int)(m - q.lo), q.raw_owner[s2] = i2;
    }
    RA_PAR_END
    RA_PAR_BEGIN
    for (int s = lane; s < total; s += lanes) {
        const int row = q.raw_row[s], owner = q.raw_owner[s];
        const int i1 = a.pair_images[2 * (q.lo + row)], i2 = a.pair_images[2 * (q.lo + row) + 1], nbr = owner == i1 ? i2 : i1;
        int rank = 0;
        for (int j = q.off[owner]; j < q.off[owner + 1]; ++j) {
            const int rj = q.raw_row[j], j1 = a.pair_images[2 * (q.lo + rj)], j2 = a.pair_images[2 * (q.lo + rj) + 1], nj = owner == j1 ? j2 : j1;
            if (nj < nbr || (nj == nbr && rj < row)) ++rank;
        }
        q.adj_nbr[q.off[owner] + rank] = nbr;
        q.adj_row[q.off[owner] + rank] = 2 * row + (owner == i1 ? 1 : 0);  // the row within the problem; rebased below
    }
    RA_PAR_END

    // the anchor's component. The lanes read reach[] of their neighbours while other lanes set it in the same section: a race that is MEANT.
    // reach[] only ever goes from 0 to 1 (a 4-byte store), a lane that misses a fresh 1 sees it in the next round, and the fixed point -- the
    // component -- is unique; only the number of rounds depends on the timing, and no output holds it. The loop ends after a round without a
    // change, at most N rounds.
    RA_PAR_BEGIN
    if (lane == 0) q.reach[anchor] = 1;
    RA_PAR_END
    for (int round = 0; round < N; ++round) {
        RA_PAR_BEGIN
        long long changed = 0;
        for (int node = lane; node < N; node += lanes) {
            if (q.reach[node]) continue;
            for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
                if (q.reach[q.adj_nbr[j]]) {
                    q.reach[node] = 1, changed = 1;
                    break;
                }
            }
        }
        q.lanebuf[lane] = changed;
        RA_PAR_END
        long long any = 0;
        RA_PAR_BEGIN
        any = 0;
        for (int l = 0; l < lanes; ++l) any |= q.lanebuf[l];
        RA_PAR_END
        if (!any) break;
    }
    RA_PAR_BEGIN
    for (int i = lane; i < N; i += lanes) q.cid[i] = q.reach[i];
    RA_PAR_END
    ra_scan(q.cid, N, q.lanebuf);
    RA_PAR_BEGIN
    for (int i = lane; i < N; i += lanes)
        if (q.reach[i]) q.cnode[q.cid[i]] = i;
    RA_PAR_END
    int n = 0, anchor_c = 0;
    RA_PAR_BEGIN
    n = q.cid[N], anchor_c = q.cid[anchor];
    RA_PAR_END
    q.n = n, q.anchor_c = anchor_c;
    q.p2 = 1;
    while (q.p2 < n) q.p2 *= 2;
    RA_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        const int node = q.cnode[c];
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) q.adj_nbr[j] = q.cid[q.adj_nbr[j]], q.adj_row[j] = q.adj_row[j] + 2 * (int)q.lo;
    }
    RA_PAR_END

    double* base = a.w.state + (size_t)p * RA_NODE_DOUBLES * (size_t)N;
    const size_t sn = (size_t)N;
    q.r = base, q.rn = base + 9 * sn, q.w = base + 18 * sn, q.wn = base + 27 * sn, q.lam = base + 36 * sn;
    q.g = base + 45 * sn, q.eta = base + 48 * sn, q.heta = base + 51 * sn, q.res = base + 54 * sn, q.d = base + 57 * sn, q.hd = base + 60 * sn;
    q.t = base + 63 * sn;  // p2 < 2 n <= 2 N, and one spare N

    // the largest weight, and the cost with every rotation the identity
    RA_PAR_BEGIN
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
    ra_tree_pad(q, lane, lanes);
    RA_PAR_END
    const double max_kappa = ra_tree(q.t, q.p2, true);
    const double initial_cost = ra_pass(a, q, q.r, q.w);

    // stage A: CG on the reduced connection Laplacian from X = 0; x = rn, residual = w, direction = wn, L p = lam
    double *x = q.rn, *cr = q.w, *cp = q.wn, *cap = q.lam;
    RA_PAR_BEGIN
    for (int c = lane; c < n; c += lanes)
        for (int i = 0; i < 9; ++i) q.r[9 * (size_t)c + i] = c == anchor_c && i % 4 == 0 ? 1.0 : 0.0;
    RA_PAR_END
    ra_apply(a, q, q.r, cap, false, false);
    RA_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        for (int i = 0; i < 9; ++i) {
            const size_t at = 9 * (size_t)c + i;
            cr[at] = c == anchor_c ? 0.0 : -cap[at];
            cp[at] = cr[at], x[at] = 0.0;
        }
        q.t[c] = ra_dot(cr + 9 * (size_t)c, cr + 9 * (size_t)c, 9);
    }
    ra_tree_pad(q, lane, lanes);
    RA_PAR_END
    double rr = ra_tree(q.t, q.p2, false);
    const double rr0 = rr;
    int chordal_steps = 0;
    while (chordal_steps < a.chordal_cap && rr > (a.chordal_tol * a.chordal_tol) * rr0) {
        ra_apply(a, q, cp, cap, false, true);
        const double pap = ra_dot_nodes(q, cp, cap, 9);
        if (!(pap > 0)) break;
        const double alpha = rr / pap;
        RA_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) {
            for (int i = 0; i < 9; ++i) {
                const size_t at = 9 * (size_t)c + i;
                x[at] = x[at] + alpha * cp[at];
                cr[at] = cr[at] - alpha * cap[at];
            }
            q.t[c] = ra_dot(cr + 9 * (size_t)c, cr + 9 * (size_t)c, 9);
        }
        ra_tree_pad(q, lane, lanes);
        RA_PAR_END
        const double rr_new = ra_tree(q.t, q.p2, false);
        const double beta = rr_new / rr;
        RA_PAR_BEGIN
        for (int c = lane; c < n; c += lanes)
            for (int i = 0; i < 9; ++i) {
                const size_t at = 9 * (size_t)c + i;
                cp[at] = cr[at] + beta * cp[at];
            }
        RA_PAR_END
        rr = rr_new;
        ++chordal_steps;
    }
    RA_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        if (c == anchor_c)
            for (int i = 0; i < 9; ++i) x[9 * (size_t)c + i] = i % 4 == 0 ? 1.0 : 0.0;
        ra_project_so3(x + 9 * (size_t)c, q.r + 9 * (size_t)c);
    }
    RA_PAR_END

    // stage B
    double f = ra_pass(a, q, q.r, q.w);
    const double chordal_cost = f;
    int status = isfinite(f) ? RA_MAX_ITERATIONS : RA_NON_FINITE;
    const int inner_cap = a.max_inner > 0 ? a.max_inner : 3 * n;
    double delta = a.delta0, gn = nan;
    int outer = 0, accepted = 0, happ = 0;
    while (status == RA_MAX_ITERATIONS) {
        RA_PAR_BEGIN
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
        ra_tree_pad(q, lane, lanes);
        RA_PAR_END
        gn = ra_tree(q.t, q.p2, true);
        double r_r = ra_dot_nodes(q, q.g, q.g, 3);
        if (!isfinite(r_r)) {
            status = RA_NON_FINITE;
            break;
        }
        if (gn <= a.gradient_tol * max_kappa) {
            status = RA_CONVERGED;
            break;
        }
        if (outer >= a.max_outer) break;
        ++outer;
        RA_PAR_BEGIN
        for (int c = lane; c < n; c += lanes)
            for (int i = 0; i < 3; ++i) {
                const size_t at = 3 * (size_t)c + i;
                q.eta[at] = 0.0, q.heta[at] = 0.0, q.res[at] = q.g[at], q.d[at] = -q.g[at];
            }
        RA_PAR_END
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
                const double tau = (-e_pd + sqrt(e_pd * e_pd + d_pd * (delta * delta - e_pe))) / d_pd;
                RA_PAR_BEGIN
                for (int c = lane; c < n; c += lanes)
                    for (int i = 0; i < 3; ++i) {
                        const size_t at = 3 * (size_t)c + i;
                        q.eta[at] = q.eta[at] + tau * q.d[at], q.heta[at] = q.heta[at] + tau * q.hd[at];
                    }
                RA_PAR_END
                on_boundary = true;
                break;
            }
            e_pe = e_pe_new;
            RA_PAR_BEGIN
            for (int c = lane; c < n; c += lanes) {
                for (int i = 0; i < 3; ++i) {
                    const size_t at = 3 * (size_t)c + i;
                    q.eta[at] = q.eta[at] + alpha * q.d[at], q.heta[at] = q.heta[at] + alpha * q.hd[at];
                    q.res[at] = q.res[at] + alpha * q.hd[at];
                }
                q.t[c] = ra_dot(q.res + 3 * (size_t)c, q.res + 3 * (size_t)c, 3);
            }
            ra_tree_pad(q, lane, lanes);
            RA_PAR_END
            const double rr_new = ra_tree(q.t, q.p2, false);
            if (sqrt(rr_new) <= target) break;
            const double beta = rr_new / r_r;
            RA_PAR_BEGIN
            for (int c = lane; c < n; c += lanes)
                for (int i = 0; i < 3; ++i) {
                    const size_t at = 3 * (size_t)c + i;
                    q.d[at] = -q.res[at] + beta * q.d[at];
                }
            RA_PAR_END
            e_pd = beta * (e_pd + alpha * d_pd);
            d_pd = rr_new + beta * beta * d_pd;
            r_r = rr_new;
        }
        const double g_eta = ra_dot_nodes(q, q.g, q.eta, 3);
        const double model = g_eta + 0.5 * ra_dot_nodes(q, q.eta, q.heta, 3);
        RA_PAR_BEGIN
        for (int c = lane; c < n; c += lanes) ra_cayley(q.r + 9 * (size_t)c, q.eta + 3 * (size_t)c, q.rn + 9 * (size_t)c);
        RA_PAR_END
        const double f_new = ra_pass(a, q, q.rn, q.wn);
        const double reg = RA_RHO_REG * (fabs(f) > 1.0 ? fabs(f) : 1.0);
        double rho = ((f - f_new) + reg) / (-model + reg);
        if (!(isfinite(f_new) && isfinite(rho))) rho = -1.0;
        if (rho > 0.1) {
            double* s = q.r;
            q.r = q.rn, q.rn = s;
            s = q.w, q.w = q.wn, q.wn = s;
            f = f_new;
            ++accepted;
        }
        if (rho < 0.25) {
            delta = delta / 4.0;
        } else if (rho > 0.75 && on_boundary) {
            delta = delta * 2.0;
        }
    }

    RA_PAR_BEGIN
    if (status != RA_NON_FINITE) {
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
    RA_PAR_END
}

// ---- kernels ----

__global__ __launch_bounds__(RA_THREADS) void ra_init_kernel(RaArgs a) {
    if (threadIdx.x < RA_FLAG_WORDS) a.w.flags[threadIdx.x] = 0;
}
__global__ __launch_bounds__(RA_THREADS) void ra_validate_kernel(RaArgs a, long long n) {
    const long long i = (long long)blockIdx.x * RA_THREADS + threadIdx.x;
    if (i < n) ra_validate(a, i);
}
// one workgroup per problem; every branch around a barrier is on a uniform value
__global__ __launch_bounds__(RA_THREADS) void ra_solve_kernel(RaArgs a) { ra_solve(a, (int)blockIdx.x); }

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
    hipLaunchKernelGGL(ra_init_kernel, dim3(1), dim3(RA_THREADS), 0, stream, a);
    GTSFM_CHECK_LAUNCH("ra_init_kernel");
    hipLaunchKernelGGL(ra_validate_kernel, dim3((unsigned)((n + RA_THREADS - 1) / RA_THREADS)), dim3(RA_THREADS), 0, stream, a, n);
    GTSFM_CHECK_LAUNCH("ra_validate_kernel");
    int flags[2] = {0, 0};
    if (hipMemcpyAsync(flags, a.w.flags, sizeof(flags), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        gtsfm_set_error("%s: reading the input flags failed: %s", me, hipGetErrorString(hipGetLastError()));
        return GTSFM_ERR_HIP;
    }
    GTSFM_CHECK_ARG(!flags[0], "%s: an enabled row has i1 == i2 or names an image outside 0 .. %d; nothing was written", me, num_images - 1);
    GTSFM_CHECK_ARG(!flags[1], "%s: problem_row_off_dev is not ascending within 0 .. %lld; nothing was written", me, num_rows);
    hipLaunchKernelGGL(ra_solve_kernel, dim3((unsigned)num_problems), dim3(RA_THREADS), 0, stream, a);
    GTSFM_CHECK_LAUNCH("ra_solve_kernel");
    return GTSFM_OK;
}
