// Global bundle adjustment on the device: every camera pose and every track's point refined by a robust Levenberg-Marquardt on the
// reprojection errors, f = sum_m rho_k(|proj(cam_i, p_j) - uv_m| / sigma), then the tracks filtered by reprojection error. Calibrations are
// held fixed, one camera (the anchor) is held fixed exactly, the scale is left to the damping. See include/gtsfm_amd.h; the specification is
// tests/global_ba_reference.py, which this file follows operation for operation.
//
//   gba_validate_kernel : one lane per track: its offsets, the validity bytes of its measurements; one lane per problem: its offsets. The
//            two refusal flags (bad track offsets, bad problem offsets). The host reads the flags here, before any output is written.
//   gba_solve_kernel    : ONE WORKGROUP PER PROBLEM runs everything else to the end, on the scaffold of problem_solver.h (the lane model,
//            the nodes' lists in the order the specification sums in, the anchor's component with compact ids, the scan and the tree).
//     nodes      : the N cameras, then the problem's tracks. A row is a measurement: a = its camera, b = N + its track - the first track.
//     lists      : a camera's in ascending (track, measurement) order, a track's in ascending (camera, measurement) order.
//     linearise  : per list entry the scaled residual, the Huber weight and the two Jacobian blocks (21 doubles), per camera the gradient
//            and the lower triangle of its 6 x 6 block, per point the gradient and its 3 x 3 block. W = (w Jc)^T Jp is never formed.
//     step       : the points' damped blocks eliminated, the reduced camera system applied matrix-free (one pass over the tracks, one over
//            the cameras) inside conjugate gradients preconditioned by the cameras' damped blocks (Cholesky), the points by
//            back-substitution, the model decrease of the step actually taken by one more pass.
//     Lane l owns the compact nodes l, l + 256, ...; a node's sums run over its list in order; every global scalar is the pairwise tree
//     over the compact index padded to a power of two. Hence no byte depends on the lane count, the run, or the problem's place in a
//     batch. There is no floating-point atomic, and nothing but + - * / sqrt and comparisons (-ffp-contract=off).
//     All state lives in the workspace (880 bytes per node and problem, 336 per measurement plus the graph's 41).
// The host build of gba_validate and gba_solve is tools/global_ba_host_main.cpp.

#include "../../include/gtsfm_amd.h"
#include "problem_solver.h"

#define GBA_MAX_ROWS (1ll << 28)   // measurements
#define GBA_MAX_NODES (1ll << 24)  // num_images + max_tracks
#define GBA_MAX_STATE (1ll << 28)  // num_problems * nodes
#define GBA_NODE_DOUBLES 110       // the tree (2 per node, padded), x and x' (12 each), g (6), the block (21), its factor (21), rhs, dx, r, z, d, S d (6 each)
#define GBA_ENTRY_DOUBLES 21       // r (2), w, Jc (2 x 6), Jp (2 x 3)
#define GBA_LAMBDA_INITIAL 1e-5
#define GBA_LAMBDA_FACTOR 10.0
#define GBA_LAMBDA_UPPER 1e5
#define GBA_MIN_FIDELITY 1e-3
#define GBA_LAMBDA_BOUND 4  // after SolverStatus

namespace {

struct GbaWorkspace {
    int* flags;          // [SOLVER_FLAG_WORDS]; 0: bad track offsets; 1: bad problem offsets
    uint8_t* valid;      // [S]
    int *row_a, *row_b;  // [S]: a measurement's nodes within its problem
    SolverGraph g;       // over the M = N + max_tracks nodes and the S rows
    double* entry;       // [2 S][GBA_ENTRY_DOUBLES]: the linearisation at the values held, per list entry
    double* state;       // [P][GBA_NODE_DOUBLES][M]
    size_t bytes;
};

GbaWorkspace gba_layout(void* base, long long meas, long long nodes, long long problems) {
    GbaWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t r = (size_t)meas, m = (size_t)nodes, p = (size_t)problems;
    w.flags = (int*)ws.take(SOLVER_FLAG_WORDS * 4);
    w.valid = (uint8_t*)ws.take(r);
    w.row_a = (int*)ws.take(r * 4);
    w.row_b = (int*)ws.take(r * 4);
    w.g = solver_carve(ws, r, m, p);
    w.entry = (double*)ws.take(2 * r * GBA_ENTRY_DOUBLES * 8);
    w.state = (double*)ws.take(p * GBA_NODE_DOUBLES * (m ? m : 1) * 8);
    w.bytes = ws.used;
    return w;
}

struct GbaArgs {
    const double* cameras;        // [N][17]
    const long long* track_off;   // [T + 1] (null when T == 0)
    const int* image;             // [S]
    const float* uv;              // [S][2]
    const double* point;          // [T][3]
    const uint8_t* track_enable;  // [T] or null
    const uint8_t* meas_enable;   // [S] or null
    const long long* problem_off;  // [P + 1] over the tracks, or null: one problem over everything
    long long num_tracks, num_meas;
    int num_images, max_tracks, num_problems, anchor, min_track_length;
    double sigma, huber_k, threshold, rel_tol, abs_tol, cg_forcing;
    int max_iterations, max_inner;
    GbaWorkspace w;
    double* cameras_out;    // [P][N][17]
    double* point_out;      // [T][3]
    double* reproj_error;   // [S]
    uint8_t* track_valid;   // [T]
    uint8_t* camera_kept;   // [P][N]
    uint8_t* node_valid;    // [P][M]
    int* counters;          // [P][8]
    double* costs;          // [P][4]
};

// ---- the validity pass ----

GTSFM_HD bool gba_meas_ok(const GbaArgs& a, long long s) {
    if (a.meas_enable && !a.meas_enable[s]) return false;
    const int i = a.image[s];
    if (!(i >= 0 && i < a.num_images) || a.cameras[17 * (size_t)i] == 0.0) return false;
    return isfinite(a.uv[2 * s]) && isfinite(a.uv[2 * s + 1]);
}

GTSFM_HD void gba_validate(const GbaArgs& a, long long m) {
    const long long S = a.num_meas, T = a.num_tracks;
    if (a.problem_off && m < a.num_problems) {
        const long long lo = a.problem_off[m], hi = a.problem_off[m + 1];
        if (!(lo >= 0 && lo <= hi && hi <= T && hi - lo <= a.max_tracks)) a.w.flags[1] = 1;
        if (m == 0 && (a.problem_off[0] != 0 || a.problem_off[a.num_problems] != T)) a.w.flags[1] = 1;
    }
    if (m == 0 && (T > 0 ? (a.track_off[0] != 0 || a.track_off[T] != S) : S != 0)) a.w.flags[0] = 1;
    if (m < T) {
        const long long lo = a.track_off[m], hi = a.track_off[m + 1];
        if (!(lo >= 0 && lo <= hi && hi <= S)) {
            a.w.flags[0] = 1;
            return;
        }
        long long count = 0;
        for (long long s = lo; s < hi; ++s) count += gba_meas_ok(a, s) ? 1 : 0;
        const double* p = a.point + 3 * m;
        const bool ok = (!a.track_enable || a.track_enable[m]) && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && count >= a.min_track_length;
        for (long long s = lo; s < hi; ++s) a.w.valid[s] = ok && gba_meas_ok(a, s) ? 1 : 0;
    }
}

// ---- the per-problem state ----

struct GbaProblem : SolverGraph {
    long long tlo, mlo;  // the problem's first track and first measurement
    int rows, nc;        // its measurements; the cameras of the component (compact ids 0 .. nc - 1)
    int *row_a, *row_b;
    double *x, *xn, *g, *blk, *fac, *rhs, *dx, *r, *z, *d, *sd, *entry;
};

struct GbaObs {
    double q[3], res[2];  // the point in the camera's frame, the residual in pixels (zero behind the camera)
    bool ok;
    const double *pose, *cam;  // the camera's 12 state numbers, its row of the table
};

// list entry j of compact node c at the values x
GTSFM_HD void gba_observe(const GbaArgs& a, const GbaProblem& q, const double* x, int c, int j, GbaObs* o) {
    const int is_cam = q.adj_row[j] & 1, nb = q.adj_nbr[j];
    const long long s = q.mlo + (q.adj_row[j] >> 1);
    const double *pose = x + 12 * (size_t)(is_cam ? c : nb), *p = x + 12 * (size_t)(is_cam ? nb : c);
    const double* cam = a.cameras + 17 * (size_t)a.image[s];
    const double dv[3] = {p[0] - pose[9], p[1] - pose[10], p[2] - pose[11]};
    for (int k = 0; k < 3; ++k) o->q[k] = (pose[k] * dv[0] + pose[3 + k] * dv[1]) + pose[6 + k] * dv[2];
    o->ok = o->q[2] > 0;
    const double z = o->ok ? o->q[2] : 1.0;
    o->res[0] = o->ok ? (cam[1] * (o->q[0] / z) + cam[3]) - (double)a.uv[2 * s] : 0.0;
    o->res[1] = o->ok ? (cam[2] * (o->q[1] / z) + cam[4]) - (double)a.uv[2 * s + 1] : 0.0;
    o->pose = pose, o->cam = cam;
}

// Huber's rho and weight at the scaled residual
GTSFM_HD void gba_huber(const double* r, bool huber, double k, double* rho, double* w) {
    const double e = sqrt(r[0] * r[0] + r[1] * r[1]);
    if (huber && e > k) {
        *rho = k * (e - 0.5 * k), *w = k / e;
    } else {
        *rho = 0.5 * (e * e), *w = 1.0;
    }
}

GTSFM_HD double gba_chain6(const double* a, const double* b) {
    double s = a[0] * b[0];
    for (int i = 1; i < 6; ++i) s = s + a[i] * b[i];
    return s;
}
GTSFM_HD double gba_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the cost at x
GTSFM_HD double gba_cost(const GbaArgs& a, const GbaProblem& q, const double* x) {
    SOLVER_PAR_BEGIN
    const bool huber = a.huber_k > 0 && isfinite(a.huber_k);
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        double cost = 0.0;
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            GbaObs o;
            gba_observe(a, q, x, c, j, &o);
            const double r[2] = {o.res[0] / a.sigma, o.res[1] / a.sigma};
            double rho, w;
            gba_huber(r, huber, a.huber_k, &rho, &w);
            cost = cost + rho;
        }
        q.t[c] = cost;
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    return 0.5 * solver_tree(q.t, q.p2, false);  // every measurement is in two lists
}

// the cost at q.x; the entries, the gradient (the anchor's zero) and the blocks
GTSFM_HD double gba_linearise(const GbaArgs& a, const GbaProblem& q) {
    SOLVER_PAR_BEGIN
    const bool huber = a.huber_k > 0 && isfinite(a.huber_k);
    const double sigma = a.sigma;
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        const bool is_cam = c < q.nc;
        double cost = 0.0, g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, blk[21];
        for (int i = 0; i < 21; ++i) blk[i] = 0.0;
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            GbaObs o;
            gba_observe(a, q, q.x, c, j, &o);
            double* en = q.entry + GBA_ENTRY_DOUBLES * (size_t)j;
            double *jc = en + 3, *jp = en + 15;
            if (o.ok) {
                const double fx = o.cam[1], fy = o.cam[2], q0 = o.q[0], q1 = o.q[1], z = o.q[2];
                const double d00 = fx / z, d02 = -((fx * q0) / (z * z)), d11 = fy / z, d12 = -((fy * q1) / (z * z));
                jc[0] = -(d02 * q1), jc[1] = d02 * q0 - d00 * z, jc[2] = d00 * q1, jc[3] = -d00, jc[4] = 0.0, jc[5] = -d02;
                jc[6] = d11 * z - d12 * q1, jc[7] = d12 * q0, jc[8] = -(d11 * q0), jc[9] = 0.0, jc[10] = -d11, jc[11] = -d12;
                for (int k = 0; k < 3; ++k) jp[k] = d00 * o.pose[3 * k] + d02 * o.pose[3 * k + 2], jp[3 + k] = d11 * o.pose[3 * k + 1] + d12 * o.pose[3 * k + 2];
                for (int i = 0; i < 18; ++i) jc[i] = jc[i] / sigma;  // Jc, then Jp
            } else {
                for (int i = 0; i < 18; ++i) jc[i] = 0.0;
            }
            en[0] = o.res[0] / sigma, en[1] = o.res[1] / sigma;
            double rho;
            gba_huber(en, huber, a.huber_k, &rho, &en[2]);
            cost = cost + rho;
            const double w = en[2];
            if (is_cam) {
                double jw[12];
                for (int i = 0; i < 12; ++i) jw[i] = w * jc[i];
                for (int i = 0; i < 6; ++i) g[i] = g[i] + (jw[i] * en[0] + jw[6 + i] * en[1]);
                for (int i = 0, at = 0; i < 6; ++i)
                    for (int k = 0; k <= i; ++k, ++at) blk[at] = blk[at] + (jw[i] * jc[k] + jw[6 + i] * jc[6 + k]);
            } else {
                double jw[6];
                for (int i = 0; i < 6; ++i) jw[i] = w * jp[i];
                for (int i = 0; i < 3; ++i) g[i] = g[i] + (jw[i] * en[0] + jw[3 + i] * en[1]);
                for (int i = 0, at = 0; i < 3; ++i)
                    for (int k = 0; k <= i; ++k, ++at) blk[at] = blk[at] + (jw[i] * jp[k] + jw[3 + i] * jp[3 + k]);
            }
        }
        for (int i = 0; i < 6; ++i) q.g[6 * (size_t)c + i] = c == q.anchor_c ? 0.0 : g[i];
        for (int i = 0; i < 21; ++i) q.blk[21 * (size_t)c + i] = blk[i];
        q.t[c] = cost;
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    return 0.5 * solver_tree(q.t, q.p2, false);
}

// (V + lam I)^-1 b by elimination without pivoting; v = (v00, v10, v11, v20, v21, v22)
GTSFM_HD void gba_point_solve(const double* v, double lam, const double* b, double* x) {
    const double a00 = v[0] + lam, a01 = v[1], a02 = v[3];
    double a11 = v[2] + lam, a12 = v[4], a22 = v[5] + lam;
    const double l10 = a01 / a00, l20 = a02 / a00;
    a11 = a11 - l10 * a01;
    a12 = a12 - l10 * a02;
    a22 = a22 - l20 * a02;
    const double l21 = a12 / a11;
    a22 = a22 - l21 * a12;
    const double b0 = b[0], b1 = b[1] - l10 * b0, b2 = (b[2] - l20 * b0) - l21 * b1;
    x[2] = b2 / a22;
    x[1] = (b1 - a12 * x[2]) / a11;
    x[0] = ((b0 - a01 * x[1]) - a02 * x[2]) / a00;
}

// the Cholesky factor of U + lam I, both as lower triangles row by row; a pivot that is not positive gives NaN: a rejected trial
GTSFM_HD void gba_camera_factor(const double* u, double lam, double* low) {
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double acc = i == j ? u[i * (i + 1) / 2 + j] + lam : u[i * (i + 1) / 2 + j];
            for (int k = 0; k < j; ++k) acc = acc - low[i * (i + 1) / 2 + k] * low[j * (j + 1) / 2 + k];
            low[i * (i + 1) / 2 + j] = i == j ? sqrt(acc) : acc / low[j * (j + 1) / 2 + j];
        }
}
GTSFM_HD void gba_camera_solve(const double* low, const double* b, double* x) {
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double acc = b[i];
        for (int k = 0; k < i; ++k) acc = acc - low[i * (i + 1) / 2 + k] * y[k];
        y[i] = acc / low[i * (i + 1) / 2 + i];
    }
    for (int i = 5; i >= 0; --i) {
        double acc = y[i];
        for (int k = i + 1; k < 6; ++k) acc = acc - low[k * (k + 1) / 2 + i] * x[k];
        x[i] = acc / low[i * (i + 1) / 2 + i];
    }
}

// over camera c's list: sum of W y_point = (w Jc)^T (Jp y); y: 6 doubles per compact node, the first three used
GTSFM_HD void gba_w_times(const GbaProblem& q, int c, const double* y, double* acc) {
    const int node = q.cnode[c];
    for (int i = 0; i < 6; ++i) acc[i] = 0.0;
    for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
        const double *en = q.entry + GBA_ENTRY_DOUBLES * (size_t)j, *jc = en + 3, *jp = en + 15, *yy = y + 6 * (size_t)q.adj_nbr[j];
        const double t0 = gba_dot3(jp, yy), t1 = gba_dot3(jp + 3, yy);
        for (int i = 0; i < 6; ++i) acc[i] = acc[i] + ((en[2] * jc[i]) * t0 + (en[2] * jc[6 + i]) * t1);
    }
}
// over point c's list: sum of W^T d_camera = (w Jp)^T (Jc d); d: 6 doubles per compact node
GTSFM_HD void gba_wt_times(const GbaProblem& q, int c, const double* d, double* acc) {
    const int node = q.cnode[c];
    for (int i = 0; i < 3; ++i) acc[i] = 0.0;
    for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
        const double *en = q.entry + GBA_ENTRY_DOUBLES * (size_t)j, *jc = en + 3, *jp = en + 15, *dd = d + 6 * (size_t)q.adj_nbr[j];
        const double t0 = gba_chain6(jc, dd), t1 = gba_chain6(jc + 6, dd);
        for (int i = 0; i < 3; ++i) acc[i] = acc[i] + ((en[2] * jp[i]) * t0 + (en[2] * jp[3 + i]) * t1);
    }
}

// <x, y> over the component's cameras, 6 numbers per node (the points count zero)
GTSFM_HD double gba_dot_cameras(const GbaProblem& q, const double* x, const double* y) {
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) q.t[c] = c < q.nc ? gba_chain6(x + 6 * (size_t)c, y + 6 * (size_t)c) : 0.0;
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    return solver_tree(q.t, q.p2, false);
}

// sd = S d with S = U + lam I - W (V + lam I)^-1 W^T, the anchor's row zero; returns <d, sd>
GTSFM_HD double gba_schur_apply(const GbaProblem& q, double lam) {
    SOLVER_PAR_BEGIN
    for (int c = q.nc + lane; c < q.n; c += lanes) {
        double acc[3];
        gba_wt_times(q, c, q.d, acc);
        gba_point_solve(q.blk + 21 * (size_t)c, lam, acc, q.sd + 6 * (size_t)c);
    }
    SOLVER_PAR_END
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.nc; c += lanes) {
        const double *u = q.blk + 21 * (size_t)c, *d = q.d + 6 * (size_t)c;
        double acc[6], *sd = q.sd + 6 * (size_t)c;
        gba_w_times(q, c, q.sd, acc);
        for (int i = 0; i < 6; ++i) {
            double ud = 0.0;
            for (int k = 0; k < 6; ++k) {
                const double uik = i >= k ? u[i * (i + 1) / 2 + k] : u[k * (k + 1) / 2 + i];
                const double term = (i == k ? uik + lam : uik) * d[k];
                ud = k == 0 ? term : ud + term;
            }
            sd[i] = c == q.anchor_c ? 0.0 : ud - acc[i];
        }
    }
    SOLVER_PAR_END
    return gba_dot_cameras(q, q.d, q.sd);
}

// The inexact damped step into q.dx; returns the model decrease of that very step. *its: the CG iterations.
GTSFM_HD double gba_step(const GbaArgs& a, const GbaProblem& q, double lam, int inner_cap, int* its) {
    SOLVER_PAR_BEGIN
    for (int c = q.nc + lane; c < q.n; c += lanes) gba_point_solve(q.blk + 21 * (size_t)c, lam, q.g + 6 * (size_t)c, q.sd + 6 * (size_t)c);
    SOLVER_PAR_END
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.nc; c += lanes) {
        const size_t at = 6 * (size_t)c;
        double acc[6];
        gba_w_times(q, c, q.sd, acc);
        gba_camera_factor(q.blk + 21 * (size_t)c, lam, q.fac + 21 * (size_t)c);
        for (int i = 0; i < 6; ++i) q.rhs[at + i] = c == q.anchor_c ? 0.0 : acc[i] - q.g[at + i], q.r[at + i] = q.rhs[at + i], q.dx[at + i] = 0.0;
        gba_camera_solve(q.fac + 21 * (size_t)c, q.r + at, q.z + at);
        for (int i = 0; i < 6; ++i) {
            if (c == q.anchor_c) q.z[at + i] = 0.0;
            q.d[at + i] = q.z[at + i];
        }
    }
    SOLVER_PAR_END
    double rz = gba_dot_cameras(q, q.r, q.z), rr = gba_dot_cameras(q, q.r, q.r);
    const double target = a.cg_forcing * sqrt(rr);
    int n_its = 0;
    while (n_its < inner_cap && !(sqrt(rr) <= target) && rz > 0) {
        const double alpha = rz / gba_schur_apply(q, lam);
        SOLVER_PAR_BEGIN
        for (int c = lane; c < q.nc; c += lanes) {
            const size_t at = 6 * (size_t)c;
            for (int i = 0; i < 6; ++i) q.dx[at + i] = q.dx[at + i] + alpha * q.d[at + i], q.r[at + i] = q.r[at + i] - alpha * q.sd[at + i];
            gba_camera_solve(q.fac + 21 * (size_t)c, q.r + at, q.z + at);
            if (c == q.anchor_c)
                for (int i = 0; i < 6; ++i) q.z[at + i] = 0.0;
        }
        SOLVER_PAR_END
        rr = gba_dot_cameras(q, q.r, q.r);
        const double rz_new = gba_dot_cameras(q, q.r, q.z);
        const double beta = rz_new / rz;
        SOLVER_PAR_BEGIN
        for (int c = lane; c < q.nc; c += lanes)
            for (int i = 0; i < 6; ++i) q.d[6 * (size_t)c + i] = q.z[6 * (size_t)c + i] + beta * q.d[6 * (size_t)c + i];
        SOLVER_PAR_END
        rz = rz_new;
        ++n_its;
    }
    *its = n_its;
    // the points by back-substitution
    SOLVER_PAR_BEGIN
    for (int c = q.nc + lane; c < q.n; c += lanes) {
        const size_t at = 6 * (size_t)c;
        double acc[3], y[3];
        gba_wt_times(q, c, q.dx, acc);
        for (int i = 0; i < 3; ++i) acc[i] = q.g[at + i] + acc[i];
        gba_point_solve(q.blk + 21 * (size_t)c, lam, acc, y);
        for (int i = 0; i < 3; ++i) q.dx[at + i] = -y[i], q.dx[at + 3 + i] = 0.0;
    }
    SOLVER_PAR_END
    // the model decrease: -(g.dx + sum_m w |Jc dc + Jp dp|^2 / 2), every measurement in two lists
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const int node = q.cnode[c];
        const bool is_cam = c < q.nc;
        double hs = 0.0;
        for (int j = q.off[node]; j < q.off[node + 1]; ++j) {
            const double *en = q.entry + GBA_ENTRY_DOUBLES * (size_t)j, *jc = en + 3, *jp = en + 15;
            const double *dc = q.dx + 6 * (size_t)(is_cam ? c : q.adj_nbr[j]), *dp = q.dx + 6 * (size_t)(is_cam ? q.adj_nbr[j] : c);
            const double j0 = gba_chain6(jc, dc) + gba_dot3(jp, dp), j1 = gba_chain6(jc + 6, dc) + gba_dot3(jp + 3, dp);
            hs = hs + en[2] * (j0 * j0 + j1 * j1);
        }
        const double gd = is_cam ? gba_chain6(q.g + 6 * (size_t)c, q.dx + 6 * (size_t)c) : gba_dot3(q.g + 6 * (size_t)c, q.dx + 6 * (size_t)c);
        q.t[c] = gd + 0.25 * hs;
    }
    solver_tree_pad(q, lane, lanes);
    SOLVER_PAR_END
    return -solver_tree(q.t, q.p2, false);
}

GTSFM_HD void gba_mm(const double* a, const double* b, double* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// xn = x moved by dx: a pose to (R Cay(omega), t + R v), a point by its 3-vector; the anchor stays
GTSFM_HD void gba_retract(const GbaProblem& q) {
    SOLVER_PAR_BEGIN
    for (int c = lane; c < q.n; c += lanes) {
        const double *x = q.x + 12 * (size_t)c, *dx = q.dx + 6 * (size_t)c;
        double* xn = q.xn + 12 * (size_t)c;
        if (c == q.anchor_c) {
            for (int i = 0; i < 12; ++i) xn[i] = x[i];
        } else if (c < q.nc) {
            const double h[3] = {0.5 * dx[0], 0.5 * dx[1], 0.5 * dx[2]};
            const double s = 2.0 / (1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]));
            const double hh[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
            double h2[9], cay[9];
            gba_mm(hh, hh, h2);
            for (int i = 0; i < 9; ++i) cay[i] = (i % 4 == 0 ? 1.0 : 0.0) + s * (hh[i] + h2[i]);
            gba_mm(x, cay, xn);
            for (int i = 0; i < 3; ++i) xn[9 + i] = x[9 + i] + gba_dot3(x + 3 * i, dx + 3);
        } else {
            for (int i = 0; i < 3; ++i) xn[i] = x[i] + dx[i];
            for (int i = 3; i < 12; ++i) xn[i] = 0.0;
        }
    }
    SOLVER_PAR_END
}

// ---- one problem, start to end ----

GTSFM_HD void gba_solve(const GbaArgs& a, int p) {
    const int N = a.num_images, M = a.num_images + a.max_tracks;
    GbaProblem q;
    q.tlo = a.problem_off ? a.problem_off[p] : 0;
    const long long thi = a.problem_off ? a.problem_off[p + 1] : a.num_tracks;
    q.mlo = a.num_tracks > 0 ? a.track_off[q.tlo] : 0;
    const long long mhi = a.num_tracks > 0 ? a.track_off[thi] : 0;
    q.rows = (int)(mhi - q.mlo);
    const size_t first = (size_t)q.mlo;
    static_cast<SolverGraph&>(q) = solver_slice(a.w.g, p, M, first);
    q.row_a = a.w.row_a + first, q.row_b = a.w.row_b + first;
    q.entry = a.w.entry + GBA_ENTRY_DOUBLES * 2 * first;
    double* cameras_out = a.cameras_out + 17 * (size_t)p * N;
    uint8_t *node_valid = a.node_valid + (size_t)p * M, *camera_kept = a.camera_kept + (size_t)p * N;
    int* counters = a.counters + 8 * (size_t)p;
    double* costs = a.costs + 4 * (size_t)p;
    const double nan = __builtin_nan("");
    const long long tlo = q.tlo;

    // the outputs' defaults (the inputs, copied through), every row's nodes
    SOLVER_PAR_BEGIN
    solver_clear(q, M, lane, lanes);
    for (int i = lane; i < M; i += lanes) node_valid[i] = 0;
    for (int i = lane; i < N; i += lanes) camera_kept[i] = 0;
    for (long long i = lane; i < 17ll * N; i += lanes) cameras_out[i] = a.cameras[i];
    for (long long j = tlo + lane; j < thi; j += lanes) {
        a.track_valid[j] = 0;
        for (int k = 0; k < 3; ++k) a.point_out[3 * j + k] = a.point[3 * j + k];
    }
    for (int i = lane; i < 8; i += lanes) counters[i] = 0;
    for (int i = lane; i < 4; i += lanes) costs[i] = nan;
    for (int l = lane; l < q.rows; l += lanes) {
        const long long s = q.mlo + l;
        long long lo = tlo, hi = thi;  // the track: track_off[lo] <= s < track_off[hi]
        for (int it = 0; it < 64 && hi - lo > 1; ++it) {
            const long long mid = lo + (hi - lo) / 2;
            if (a.track_off[mid] <= s) {
                lo = mid;
            } else {
                hi = mid;
            }
        }
        q.row_a[l] = a.image[s], q.row_b[l] = N + (int)(lo - tlo);
        a.reproj_error[s] = nan;
    }
    SOLVER_PAR_END
    int total = 0;
    const int first_row = solver_build_lists(
        q, M, q.rows, [&](int l, int* na, int* nb) { *na = q.row_a[l], *nb = q.row_b[l]; }, [&](int l) { return a.w.valid[q.mlo + l] != 0; }, &total);
    // the anchor: the smallest camera with a valid measurement, or the one given when it has one
    SOLVER_PAR_BEGIN
    long long low = N;
    for (int l = lane; l < q.rows; l += lanes)
        if (a.w.valid[q.mlo + l] && q.row_a[l] < low) low = q.row_a[l];
    q.lanebuf[lane] = low;
    SOLVER_PAR_END
    long long low = N;
    SOLVER_PAR_BEGIN
    low = N;
    for (int l = 0; l < lanes; ++l) low = q.lanebuf[l] < low ? q.lanebuf[l] : low;
    if (a.anchor >= 0) low = q.off[a.anchor + 1] > q.off[a.anchor] ? a.anchor : N;
    SOLVER_PAR_END
    if (first_row >= q.rows || low >= N) {
        SOLVER_PAR_BEGIN
        if (lane == 0) counters[0] = SOLVER_NO_VALID_ROW, counters[1] = a.anchor, counters[4] = total / 2;
        SOLVER_PAR_END
        return;
    }
    const int anchor = (int)low;
    solver_component(q, anchor, M);
    const int n = q.n;
    int nc = 0;
    SOLVER_PAR_BEGIN
    nc = q.cid[N];
    SOLVER_PAR_END
    q.nc = nc;

    double* base = a.w.state + (size_t)p * GBA_NODE_DOUBLES * (size_t)M;
    const size_t sm = (size_t)M;
    q.t = base;  // p2 < 2 n <= 2 M
    q.x = base + 2 * sm, q.xn = base + 14 * sm, q.g = base + 26 * sm, q.blk = base + 32 * sm, q.fac = base + 53 * sm, q.rhs = base + 74 * sm, q.dx = base + 80 * sm;
    q.r = base + 86 * sm, q.z = base + 92 * sm, q.d = base + 98 * sm, q.sd = base + 104 * sm;

    SOLVER_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        const int node = q.cnode[c];
        double* x = q.x + 12 * (size_t)c;
        if (c < nc) {
            for (int i = 0; i < 12; ++i) x[i] = a.cameras[17 * (size_t)node + 5 + i];
        } else {
            for (int i = 0; i < 12; ++i) x[i] = i < 3 ? a.point[3 * (tlo + (node - N)) + i] : 0.0;
        }
    }
    SOLVER_PAR_END

    double f = gba_linearise(a, q);
    const double init_cost = f;
    int status = f != f ? SOLVER_NON_FINITE : SOLVER_MAX_ITERATIONS;
    const int inner_cap = a.max_inner > 0 ? a.max_inner : 6 * nc;
    const long long solve_cap = 2ll * a.max_iterations + 16;
    double lam = GBA_LAMBDA_INITIAL;
    int accepted = 0, solves = 0, cg_total = 0;
    bool fresh = true;
    while (status == SOLVER_MAX_ITERATIONS && accepted < a.max_iterations && solves < solve_cap) {
        if (!fresh) {
            gba_linearise(a, q);
            fresh = true;
        }
        ++solves;
        int its = 0;
        const double model = gba_step(a, q, lam, inner_cap, &its);
        cg_total += its;
        gba_retract(q);
        const double f_new = gba_cost(a, q, q.xn);
        if (isfinite(f_new) && model > 0 && (f - f_new) / model > GBA_MIN_FIDELITY) {
            const double dec = f - f_new, rel = dec / f;
            double* s = q.x;
            q.x = q.xn, q.xn = s;
            f = f_new, fresh = false;
            ++accepted;
            lam = lam / GBA_LAMBDA_FACTOR;
            if (dec < a.abs_tol || rel < a.rel_tol) status = SOLVER_CONVERGED;
        } else {
            lam = lam * GBA_LAMBDA_FACTOR;
            if (lam > GBA_LAMBDA_UPPER) status = GBA_LAMBDA_BOUND;
        }
    }
    if (status == SOLVER_NON_FINITE) {
        SOLVER_PAR_BEGIN
        if (lane == 0) counters[0] = status, counters[1] = anchor, counters[2] = nc, counters[3] = n - nc, counters[4] = total / 2;  // the costs stay NaN
        SOLVER_PAR_END
        return;
    }
    if (!fresh) gba_linearise(a, q);
    const double gn = solver_inf_norm(q, q.g, 6);

    // the results: poses and points, the reprojection errors and the filter
    SOLVER_PAR_BEGIN
    for (int c = lane; c < n; c += lanes) {
        const int node = q.cnode[c];
        const double* x = q.x + 12 * (size_t)c;
        node_valid[node] = 1;
        if (c < nc) {
            for (int i = 0; i < 12; ++i) cameras_out[17 * (size_t)node + 5 + i] = x[i];
        } else {
            const long long j = tlo + (node - N);
            for (int i = 0; i < 3; ++i) a.point_out[3 * j + i] = x[i];
            bool good = true;
            for (int e = q.off[node]; e < q.off[node + 1]; ++e) {
                GbaObs o;
                gba_observe(a, q, q.x, c, e, &o);
                const double err = o.ok ? sqrt(o.res[0] * o.res[0] + o.res[1] * o.res[1]) : nan;
                a.reproj_error[q.mlo + (q.adj_row[e] >> 1)] = err;
                good = good && err < a.threshold;
            }
            a.track_valid[j] = good ? 1 : 0;
            q.cursor[c] = good ? 1 : 0;
        }
    }
    SOLVER_PAR_END
    SOLVER_PAR_BEGIN
    for (int c = lane; c < nc; c += lanes) {
        const int node = q.cnode[c];
        int kept = 0;
        for (int e = q.off[node]; e < q.off[node + 1]; ++e) kept |= q.cursor[q.adj_nbr[e]];
        camera_kept[node] = kept ? 1 : 0;
    }
    if (lane == 0) {
        counters[0] = status, counters[1] = anchor, counters[2] = nc, counters[3] = n - nc, counters[4] = total / 2, counters[5] = accepted, counters[6] = solves;
        counters[7] = cg_total;
        costs[0] = init_cost, costs[1] = f, costs[2] = gn, costs[3] = lam;
    }
    SOLVER_PAR_END
}

// ---- kernels ----

__global__ __launch_bounds__(SOLVER_THREADS) void gba_validate_kernel(GbaArgs a, long long n) {
    const long long i = (long long)blockIdx.x * SOLVER_THREADS + threadIdx.x;
    if (i < n) gba_validate(a, i);
}
// one workgroup per problem; every branch around a barrier is on a uniform value
__global__ __launch_bounds__(SOLVER_THREADS) void gba_solve_kernel(GbaArgs a) { gba_solve(a, (int)blockIdx.x); }

bool gba_sizes_ok(long long num_meas, long long num_images, long long num_tracks, long long max_tracks, long long num_problems) {
    return num_meas >= 0 && num_images >= 0 && num_tracks >= 0 && max_tracks >= 0 && max_tracks <= num_tracks && num_problems >= 1 && num_meas < GBA_MAX_ROWS &&
           num_tracks < GBA_MAX_ROWS && num_images + max_tracks < GBA_MAX_NODES && num_problems < GBA_MAX_STATE &&
           num_problems * (num_images + max_tracks > 0 ? num_images + max_tracks : 1) < GBA_MAX_STATE;
}
bool gba_options_ok(int min_track_length, double sigma, double huber_k, double threshold, double rel_tol, double abs_tol, double cg_forcing, int max_iterations,
                    int max_inner) {
    return min_track_length >= 1 && isfinite(sigma) && sigma > 0 && !(huber_k != huber_k) && threshold > 0 && rel_tol >= 0 && abs_tol >= 0 && cg_forcing >= 0 &&
           max_iterations >= 0 && max_iterations < (1 << 29) && max_inner >= 0;
}
long long gba_validate_lanes(long long num_tracks, long long num_problems) {
    const long long n = num_tracks > num_problems ? num_tracks : num_problems;
    return n > 1 ? n : 1;
}

}  // namespace

extern "C" size_t gtsfm_global_ba_workspace_bytes(long long num_meas, long long num_images, long long num_tracks, long long max_problem_tracks, long long num_problems) {
    if (!gba_sizes_ok(num_meas, num_images, num_tracks, max_problem_tracks, num_problems)) return 0;
    return gba_layout(nullptr, num_meas, num_images + max_problem_tracks, num_problems).bytes;
}

extern "C" int gtsfm_global_ba_f64(const double* cameras_dev, int num_images, const long long* track_off_dev, const int32_t* image_dev, const float* uv_dev,
                                   const double* point_dev, const uint8_t* track_enable_dev, const uint8_t* meas_enable_dev, long long num_tracks, long long num_meas,
                                   const long long* problem_off_dev, int num_problems, long long max_problem_tracks, int anchor, int min_track_length,
                                   double measurement_sigma, double huber_k, double reproj_error_threshold, double rel_tol, double abs_tol, double cg_forcing,
                                   int max_iterations, int max_inner, void* workspace_dev, size_t workspace_bytes, double* cameras_out_dev, double* point_out_dev,
                                   double* reproj_error_dev, uint8_t* track_valid_dev, uint8_t* camera_kept_dev, uint8_t* node_valid_dev, int32_t* counters_dev,
                                   double* costs_dev, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* me = "gtsfm_global_ba_f64";
    GTSFM_CHECK_ARG(gba_sizes_ok(num_meas, num_images, num_tracks, max_problem_tracks, num_problems),
                    "%s: sizes out of range (%lld measurements, %d images, %lld tracks, %lld per problem, %d problems)", me, num_meas, num_images, num_tracks,
                    max_problem_tracks, num_problems);
    GTSFM_CHECK_ARG(anchor >= -1 && (anchor < num_images || anchor == -1), "%s: the anchor %d is outside -1 .. %d", me, anchor, num_images - 1);
    GTSFM_CHECK_ARG(gba_options_ok(min_track_length, measurement_sigma, huber_k, reproj_error_threshold, rel_tol, abs_tol, cg_forcing, max_iterations, max_inner),
                    "%s: measurement_sigma must be positive and finite, huber_k not NaN, the threshold and min_track_length positive, no tolerance or cap negative", me);
    GTSFM_CHECK_ARG(workspace_dev && counters_dev && costs_dev, "%s: null pointer", me);
    GTSFM_CHECK_ARG(num_images == 0 || (cameras_dev && cameras_out_dev && camera_kept_dev && node_valid_dev), "%s: null camera pointer", me);
    GTSFM_CHECK_ARG(num_tracks == 0 || (track_off_dev && point_dev && point_out_dev && track_valid_dev && node_valid_dev), "%s: %lld tracks with a null track pointer", me,
                    num_tracks);
    GTSFM_CHECK_ARG(num_meas == 0 || (num_tracks > 0 && image_dev && uv_dev && reproj_error_dev), "%s: %lld measurements without tracks or with a null pointer", me, num_meas);
    GTSFM_CHECK_ARG(problem_off_dev || (num_problems == 1 && max_problem_tracks == num_tracks),
                    "%s: without problem_off_dev there is one problem and max_problem_tracks is num_tracks", me);
    GTSFM_CHECK_ARG(((uintptr_t)workspace_dev & 255) == 0, "%s: the workspace must be aligned to 256 bytes", me);
    const long long nodes = num_images + max_problem_tracks;
    GbaArgs a{cameras_dev, track_off_dev, image_dev, uv_dev, point_dev, track_enable_dev, meas_enable_dev, problem_off_dev, num_tracks, num_meas, num_images,
              (int)max_problem_tracks, num_problems, anchor, min_track_length, measurement_sigma, huber_k, reproj_error_threshold, rel_tol, abs_tol, cg_forcing, max_iterations,
              max_inner, gba_layout(workspace_dev, num_meas, nodes, num_problems), cameras_out_dev, point_out_dev, reproj_error_dev, track_valid_dev, camera_kept_dev,
              node_valid_dev, counters_dev, costs_dev};
    if (workspace_bytes < a.w.bytes) {
        gtsfm_set_error("%s: workspace of %zu bytes, %zu needed for %lld measurements, %lld nodes and %d problems", me, workspace_bytes, a.w.bytes, num_meas, nodes, num_problems);
        return GTSFM_ERR_WORKSPACE;
    }
    int flags[2] = {0, 0};
    const int rc = solver_launch(me, gba_validate_kernel, "gba_validate_kernel", a, a.w.flags, gba_validate_lanes(num_tracks, num_problems), stream, flags);
    if (rc != GTSFM_OK) return rc;
    GTSFM_CHECK_ARG(!flags[0], "%s: track_off_dev is not ascending from 0 to %lld; nothing was written", me, num_meas);
    GTSFM_CHECK_ARG(!flags[1], "%s: problem_off_dev is not ascending from 0 to %lld, or a problem has more than %lld tracks; nothing was written", me, num_tracks,
                    max_problem_tracks);
    hipLaunchKernelGGL(gba_solve_kernel, dim3((unsigned)num_problems), dim3(SOLVER_THREADS), 0, stream, a);
    GTSFM_CHECK_LAUNCH("gba_solve_kernel");
    return GTSFM_OK;
}
