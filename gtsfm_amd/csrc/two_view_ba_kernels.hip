// Two-view bundle adjustment on the device: what TwoViewEstimator.bundle_adjust does per image pair
// (gtsfm/two_view_estimator.py:212-288 with gtsfm/bundle/two_view_ba.py and bundle_adjustment.py), for all pairs of a verifier launch
// in one call. See include/gtsfm_amd.h; the specification is tests/two_view_ba_reference.py, float64 throughout.
//
// PARITY UNPINNED towards gtsam: its Levenberg-Marquardt path and retraction, the cheirality convention of GeneralSFMFactor2, the pivot
// thresholds of the indeterminate-system test, calibrations held fixed and the absence of pose priors are restated in the
// specification's header, none was observed running.
//
// Mapping:
//   init / prepare : every match row becomes a track of two measurements (cameras 2p and 2p + 1 of a [2P][17] table; image -1 for a row
//                    that is not verified), so that gtsfm_triangulate_tracks_f64 itself triangulates them: the points that enter the
//                    adjustment ARE that call's output.
//   adjust         : one 256-lane workgroup per pair. Lane l owns the pair's rows l, l + 256, ... and keeps their points in global memory
//                    (point_dev, and a trial copy in the workspace). Per Levenberg-Marquardt trial every lane eliminates its points'
//                    3 x 3 blocks into its own copy of the 12 x 12 Schur complement (78 unique entries), the camera gradient and the
//                    reduced right-hand side (12 + 12), in registers; the 102 sums are combined across the workgroup, lane 0 adds the pose
//                    prior and the damping, factors the system (Cholesky) and retracts the poses; every lane back-substitutes its own
//                    points and evaluates the trial cost; the cost is combined and lane 0 decides once, through LDS, for all.
// Determinism: no floating-point atomics. A lane sums its own points in row order; lanes are combined by the xor butterfly of a wave (the
// same tree in every lane: a + b and b + a are the same bits) and the four waves as (w0 + w1) + (w2 + w3). A pair's outputs depend on that
// pair's data (which of its slice's rows are verified included: the row decides the lane) and the options only -- not on the batch, its
// position in it, or the run.

#include <math.h>

#include "../../include/gtsfm_amd.h"
#include "common.h"

#define TVBA_THREADS 256
#define TVBA_WAVES (TVBA_THREADS / 64)
#define TVBA_SUMS 102  // 78 Schur entries, 12 camera gradient, 12 reduced right-hand side
#define TVBA_LAMBDA_INITIAL 1.0e-5
#define TVBA_LAMBDA_FACTOR 10.0
#define TVBA_LAMBDA_UPPER 1.0e5
#define TVBA_MIN_FIDELITY 1.0e-3
#define TVBA_ABS_TOL 1.0e-5
#define TVBA_REL_TOL 1.0e-5
// the per-point and per-pair arithmetic also compiles for the host, where a stand-alone program can run it under a sanitizer
#define TVBA_HD __host__ __device__

enum { TVBA_OK = 0, TVBA_SKIPPED = 1, TVBA_NO_INITIAL_POSE = 2, TVBA_NONE_TRIANGULATED = 3, TVBA_INDETERMINATE = 4 };

namespace {

struct TvbaPose {  // world from camera
    double r[9], t[3];
};

struct TvbaCal {
    double fx, fy, cx, cy;
};

struct TvbaOptions {
    double huber_k, inv_sigma, pose_prior_inv_sigma, point_prior_inv_var;
};

// index of (a, b), a <= b, in the packed upper triangle of a 12 x 12 matrix
TVBA_HD constexpr int tvba_idx(int a, int b) { return a * 12 - a * (a - 1) / 2 + (b - a); }

// One measurement: the residual over sigma (pixels), its Huber weight and loss, and the Jacobians of the scaled residual towards the
// camera's tangent (rotation, then translation) and the point. Depth <= 0: false, and nothing is contributed.
TVBA_HD inline bool tvba_measure(const TvbaPose& x, const TvbaCal& k, const double* p, double u, double v, const TvbaOptions& o, double* res,
                                 double& weight, double& loss, double jc[2][6], double jp[2][3]) {
    const double d0 = p[0] - x.t[0], d1 = p[1] - x.t[1], d2 = p[2] - x.t[2];
    const double q0 = x.r[0] * d0 + x.r[3] * d1 + x.r[6] * d2;
    const double q1 = x.r[1] * d0 + x.r[4] * d1 + x.r[7] * d2;
    const double q2 = x.r[2] * d0 + x.r[5] * d1 + x.r[8] * d2;
    if (!(q2 > 0.0)) return false;
    res[0] = (k.fx * q0 / q2 + k.cx - u) * o.inv_sigma;
    res[1] = (k.fy * q1 / q2 + k.cy - v) * o.inv_sigma;
    const double e = sqrt(res[0] * res[0] + res[1] * res[1]);
    const bool small = e <= o.huber_k;
    weight = small ? 1.0 : o.huber_k / e;
    loss = small ? e * e * 0.5 : o.huber_k * (e - o.huber_k * 0.5);
    // d (projection) / d q, scaled
    const double a0 = k.fx / q2 * o.inv_sigma, a2 = -k.fx * q0 / (q2 * q2) * o.inv_sigma;
    const double b1 = k.fy / q2 * o.inv_sigma, b2 = -k.fy * q1 / (q2 * q2) * o.inv_sigma;
    // d q / d omega = [q]x, d q / d v = -I
    jc[0][0] = -(a2 * q1);
    jc[0][1] = a2 * q0 - a0 * q2;
    jc[0][2] = a0 * q1;
    jc[0][3] = -a0;
    jc[0][4] = 0.0;
    jc[0][5] = -a2;
    jc[1][0] = b1 * q2 - b2 * q1;
    jc[1][1] = b2 * q0;
    jc[1][2] = -(b1 * q0);
    jc[1][3] = 0.0;
    jc[1][4] = -b1;
    jc[1][5] = -b2;
    // d q / d P = R^T
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        jp[0][j] = a0 * x.r[3 * j] + a2 * x.r[3 * j + 2];
        jp[1][j] = b1 * x.r[3 * j + 1] + b2 * x.r[3 * j + 2];
    }
    return true;
}

// the robust loss of one measurement (0 behind the camera)
TVBA_HD inline double tvba_loss(const TvbaPose& x, const TvbaCal& k, const double* p, double u, double v, const TvbaOptions& o) {
    const double d0 = p[0] - x.t[0], d1 = p[1] - x.t[1], d2 = p[2] - x.t[2];
    const double q0 = x.r[0] * d0 + x.r[3] * d1 + x.r[6] * d2;
    const double q1 = x.r[1] * d0 + x.r[4] * d1 + x.r[7] * d2;
    const double q2 = x.r[2] * d0 + x.r[5] * d1 + x.r[8] * d2;
    if (!(q2 > 0.0)) return 0.0;
    const double r0 = (k.fx * q0 / q2 + k.cx - u) * o.inv_sigma, r1 = (k.fy * q1 / q2 + k.cy - v) * o.inv_sigma;
    const double e = sqrt(r0 * r0 + r1 * r1);
    return e <= o.huber_k ? e * e * 0.5 : o.huber_k * (e - o.huber_k * 0.5);
}

// reprojection error in pixels; NaN for depth <= 0
TVBA_HD inline double tvba_error(const TvbaPose& x, const TvbaCal& k, const double* p, double u, double v) {
    const double d0 = p[0] - x.t[0], d1 = p[1] - x.t[1], d2 = p[2] - x.t[2];
    const double q0 = x.r[0] * d0 + x.r[3] * d1 + x.r[6] * d2;
    const double q1 = x.r[1] * d0 + x.r[4] * d1 + x.r[7] * d2;
    const double q2 = x.r[2] * d0 + x.r[5] * d1 + x.r[8] * d2;
    if (!(q2 > 0.0)) return NAN;
    const double r0 = k.fx * q0 / q2 + k.cx - u, r1 = k.fy * q1 / q2 + k.cy - v;
    return sqrt(r0 * r0 + r1 * r1);
}

// The cost of one point: both measurements and, for the pair's first point, its prior.
TVBA_HD inline double tvba_point_cost(const TvbaPose* x, const TvbaCal* k, const double* p, const float* uv1, const float* uv2, const double* prior_at,
                                      const TvbaOptions& o) {
    double c = tvba_loss(x[0], k[0], p, (double)uv1[0], (double)uv1[1], o) + tvba_loss(x[1], k[1], p, (double)uv2[0], (double)uv2[1], o);
    if (prior_at) {
        const double e0 = p[0] - prior_at[0], e1 = p[1] - prior_at[1], e2 = p[2] - prior_at[2];
        c = c + 0.5 * ((e0 * e0 + e1 * e1 + e2 * e2) * o.point_prior_inv_var);
    }
    return c;
}

// The Gauss-Newton blocks of one point: V (upper triangle, 6), W [12][3], gp [3]; with `sums`, the cameras' own blocks and gradient are
// added to it (the Schur entries at tvba_idx, the gradient at 78 ..).
template <bool CAMERAS>
TVBA_HD inline void tvba_point_system(const TvbaPose* x, const TvbaCal* k, const double* p, const float* uv1, const float* uv2, const double* prior_at,
                                      const TvbaOptions& o, double* v, double w[12][3], double* gp, double* sums) {
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) gp[i] = 0.0;
#pragma unroll
    for (int cam = 0; cam < 2; ++cam) {
        double res[2], weight, loss, jc[2][6], jp[2][3];
        const float* uv = cam == 0 ? uv1 : uv2;
        const bool ok = tvba_measure(x[cam], k[cam], p, (double)uv[0], (double)uv[1], o, res, weight, loss, jc, jp);
        if (!ok) {
            res[0] = res[1] = weight = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) jc[0][i] = jc[1][i] = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) jp[0][i] = jp[1][i] = 0.0;
        }
        int n = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gp[i] = gp[i] + weight * (jp[0][i] * res[0] + jp[1][i] * res[1]);
#pragma unroll
            for (int j = i; j < 3; ++j) v[n++] += weight * (jp[0][i] * jp[0][j] + jp[1][i] * jp[1][j]);
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int j = 0; j < 3; ++j) w[6 * cam + a][j] = weight * (jc[0][a] * jp[0][j] + jc[1][a] * jp[1][j]);
            if (CAMERAS) {
                sums[78 + 6 * cam + a] += weight * (jc[0][a] * res[0] + jc[1][a] * res[1]);
#pragma unroll
                for (int b = a; b < 6; ++b) sums[tvba_idx(6 * cam + a, 6 * cam + b)] += weight * (jc[0][a] * jc[0][b] + jc[1][a] * jc[1][b]);
            }
        }
    }
    if (prior_at) {
        v[0] += o.point_prior_inv_var;
        v[3] += o.point_prior_inv_var;
        v[5] += o.point_prior_inv_var;
#pragma unroll
        for (int i = 0; i < 3; ++i) gp[i] = gp[i] + o.point_prior_inv_var * (p[i] - prior_at[i]);
    }
}

// V + lam I = L D L^T by elimination without pivoting; f = (l10, l20, l21, a01, a02, a12'), piv = the three pivots. false for a pivot
// that is not positive or not finite.
TVBA_HD inline bool tvba_factor3(const double* v, double lam, double* f, double* piv) {
    const double a00 = v[0] + lam, a01 = v[1], a02 = v[2];
    double a11 = v[3] + lam, a12 = v[4], a22 = v[5] + lam;
    const double l10 = a01 / a00, l20 = a02 / a00;
    a11 = a11 - l10 * a01;
    a12 = a12 - l10 * a02;
    a22 = a22 - l20 * a02;
    const double l21 = a12 / a11;
    a22 = a22 - l21 * a12;
    f[0] = l10;
    f[1] = l20;
    f[2] = l21;
    f[3] = a01;
    f[4] = a02;
    f[5] = a12;
    piv[0] = a00;
    piv[1] = a11;
    piv[2] = a22;
    return a00 > 0.0 && a11 > 0.0 && a22 > 0.0 && isfinite(a00) && isfinite(a11) && isfinite(a22);
}

TVBA_HD inline void tvba_solve3(const double* f, const double* piv, const double* b, double* x) {
    const double b0 = b[0], b1 = b[1] - f[0] * b0, b2 = b[2] - f[1] * b0 - f[2] * b1;
    x[2] = b2 / piv[2];
    x[1] = (b1 - f[5] * x[2]) / piv[1];
    x[0] = (b0 - f[3] * x[1] - f[4] * x[2]) / piv[0];
}

// One point's part of the reduced camera system at damping lam, added to sums [102]; false for a point block without a positive pivot.
TVBA_HD inline bool tvba_point_reduce(const TvbaPose* x, const TvbaCal* k, const double* p, const float* uv1, const float* uv2, const double* prior_at,
                                      const TvbaOptions& o, double lam, double* sums) {
    double v[6], w[12][3], gp[3], f[6], piv[3], y[3];
    tvba_point_system<true>(x, k, p, uv1, uv2, prior_at, o, v, w, gp, sums);
    const bool ok = tvba_factor3(v, lam, f, piv);
#pragma unroll
    for (int b = 0; b < 12; ++b) {
        tvba_solve3(f, piv, w[b], y);
#pragma unroll
        for (int a = 0; a <= b; ++a) sums[tvba_idx(a, b)] -= w[a][0] * y[0] + w[a][1] * y[1] + w[a][2] * y[2];
    }
    tvba_solve3(f, piv, gp, y);
#pragma unroll
    for (int a = 0; a < 12; ++a) sums[90 + a] += w[a][0] * y[0] + w[a][1] * y[1] + w[a][2] * y[2];
    return ok;
}

// One point's step for the cameras' step dc: dp = -(V + lam I)^-1 (gp + W^T dc); also gp . dp.
TVBA_HD inline void tvba_point_step(const TvbaPose* x, const TvbaCal* k, const double* p, const float* uv1, const float* uv2, const double* prior_at,
                                    const TvbaOptions& o, double lam, const double* dc, double* dp, double& gtd) {
    double v[6], w[12][3], gp[3], f[6], piv[3], b[3], y[3];
    tvba_point_system<false>(x, k, p, uv1, uv2, prior_at, o, v, w, gp, nullptr);
    tvba_factor3(v, lam, f, piv);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double s = gp[j];
#pragma unroll
        for (int a = 0; a < 12; ++a) s = s + w[a][j] * dc[a];
        b[j] = s;
    }
    tvba_solve3(f, piv, b, y);
    dp[0] = -y[0];
    dp[1] = -y[1];
    dp[2] = -y[2];
    gtd = gp[0] * dp[0] + gp[1] * dp[1] + gp[2] * dp[2];
}

TVBA_HD inline void tvba_skew_terms(const double* w, double a, double b, double c, double* m) {  // c I + a [w]x + b [w]x^2, row-major
    const double x = w[0], y = w[1], z = w[2];
    m[0] = c + b * (-(y * y) - z * z);
    m[1] = a * -z + b * (x * y);
    m[2] = a * y + b * (x * z);
    m[3] = a * z + b * (x * y);
    m[4] = c + b * (-(x * x) - z * z);
    m[5] = a * -x + b * (y * z);
    m[6] = a * -y + b * (x * z);
    m[7] = a * x + b * (y * z);
    m[8] = c + b * (-(x * x) - y * y);
}

TVBA_HD inline void tvba_exp_so3(const double* w, double* m) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], theta = sqrt(t2);
    double a, b;
    if (theta < 1.0e-4) {
        a = 1.0 - t2 / 6.0;
        b = 0.5 - t2 / 24.0;
    } else {
        a = sin(theta) / theta;
        b = (1.0 - cos(theta)) / t2;
    }
    tvba_skew_terms(w, a, b, 1.0, m);
}

TVBA_HD inline void tvba_log_so3(const double* r, double* w) {
    const double v0 = (r[7] - r[5]) * 0.5, v1 = (r[2] - r[6]) * 0.5, v2 = (r[3] - r[1]) * 0.5;
    const double s = sqrt(v0 * v0 + v1 * v1 + v2 * v2), c = (r[0] + r[4] + r[8] - 1.0) * 0.5;
    const double f = s < 1.0e-4 ? 1.0 + s * s / 6.0 : atan2(s, c) / s;
    w[0] = v0 * f;
    w[1] = v1 * f;
    w[2] = v2 * f;
}

// (R, t) -> (R Exp(omega), t + R v)
TVBA_HD inline void tvba_retract(const TvbaPose& x, const double* d, TvbaPose& out) {
    double e[9];
    tvba_exp_so3(d, e);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out.r[3 * i + j] = x.r[3 * i] * e[j] + x.r[3 * i + 1] * e[3 + j] + x.r[3 * i + 2] * e[6 + j];
        out.t[i] = x.t[i] + (x.r[3 * i] * d[3] + x.r[3 * i + 1] * d[4] + x.r[3 * i + 2] * d[5]);
    }
}

// PriorFactorPose3 on camera 0 at the identity: its cost, and (with sums) its part of the camera system.
TVBA_HD inline double tvba_pose_prior(const TvbaPose& x, double inv_sigma, double* sums) {
    double w[3], res[6], jac[6][6];
    tvba_log_so3(x.r, w);
    for (int i = 0; i < 3; ++i) {
        res[i] = w[i] * inv_sigma;
        res[3 + i] = x.t[i] * inv_sigma;
    }
    double cost = 0.0;
    for (int i = 0; i < 6; ++i) cost = cost + res[i] * res[i];
    cost = 0.5 * cost;
    if (!sums) return cost;
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], theta = sqrt(t2);
    const double c = theta < 1.0e-3 ? 1.0 / 12.0 + t2 / 720.0 : 1.0 / t2 - (1.0 + cos(theta)) / (2.0 * theta * sin(theta));
    double m[9];
    tvba_skew_terms(w, 0.5, c, 1.0, m);
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) jac[i][j] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            jac[i][j] = m[3 * i + j] * inv_sigma;
            jac[3 + i][3 + j] = x.r[3 * i + j] * inv_sigma;
        }
    for (int a = 0; a < 6; ++a) {
        double g = 0.0;
        for (int i = 0; i < 6; ++i) g = g + jac[i][a] * res[i];
        sums[78 + a] += g;
        for (int b = a; b < 6; ++b) {
            double h = 0.0;
            for (int i = 0; i < 6; ++i) h = h + jac[i][a] * jac[i][b];
            sums[tvba_idx(a, b)] += h;
        }
    }
    return cost;
}

// (S + lam I) x = b with S packed (upper triangle): Cholesky row by row. low [144] is scratch. false for a pivot that is not positive or
// not finite, or a solution that is not finite.
TVBA_HD inline bool tvba_cholesky12(const double* s, double lam, const double* b, double* low, double* x) {
    for (int i = 0; i < 12; ++i)
        for (int j = 0; j <= i; ++j) {
            double acc = s[tvba_idx(j, i)] + (i == j ? lam : 0.0);
            for (int k = 0; k < j; ++k) acc = acc - low[12 * i + k] * low[12 * j + k];
            if (i == j) {
                if (!(acc > 0.0) || !isfinite(acc)) return false;
                low[12 * i + i] = sqrt(acc);
            } else {
                low[12 * i + j] = acc / low[12 * j + j];
            }
        }
    if (!b) return true;
    double y[12];
    for (int i = 0; i < 12; ++i) {
        double acc = b[i];
        for (int k = 0; k < i; ++k) acc = acc - low[12 * i + k] * y[k];
        y[i] = acc / low[12 * i + i];
    }
    bool finite = true;
    for (int i = 11; i >= 0; --i) {
        double acc = y[i];
        for (int k = i + 1; k < 12; ++k) acc = acc - low[12 * k + i] * x[k];
        x[i] = acc / low[12 * i + i];
        finite = finite && isfinite(x[i]);
    }
    return finite;
}

// What a lane needs of its pair. A lane owns rows a + lane, a + lane + TVBA_THREADS, ... below a + count; a row takes part when it is
// verified and its triangulation succeeded.
struct TvbaPair {
    long long a, count, first_row;
    const uint8_t* inlier_mask;
    const int* tri_exit;
    const float* uv;  // [M][4]: the pixel in image 1, then in image 2
    double prior_at[3];
    TvbaCal cal[2];
    TvbaOptions opt;
    TVBA_HD inline bool takes_part(long long row) const { return inlier_mask[row] != 0 && tri_exit[row] == 0; }
    TVBA_HD inline const double* prior(long long row) const { return row == first_row ? prior_at : nullptr; }
};

struct TvbaControl {
    double lam, cost, first_cost;
    int accepted, solves, stop, solved, accept;
};

// a lane's part of the cost of `values` at `pose`, its points in row order
TVBA_HD inline double tvba_lane_cost(const TvbaPair& q, int lane, const TvbaPose* pose, const double* values) {
    const TvbaPose x[2] = {pose[0], pose[1]};
    double c = 0.0;
    for (long long j = lane; j < q.count; j += TVBA_THREADS) {
        const long long row = q.a + j;
        if (!q.takes_part(row)) continue;
        c = c + tvba_point_cost(x, q.cal, values + 3 * row, q.uv + 4 * row, q.uv + 4 * row + 2, q.prior(row), q.opt);
    }
    return c;
}

// a lane's part of the reduced camera system at damping lam -> sums [102]; a point block without a positive pivot poisons it
TVBA_HD inline void tvba_lane_reduce(const TvbaPair& q, int lane, const TvbaPose* pose, const double* point, double lam, double* sums) {
    const TvbaPose x[2] = {pose[0], pose[1]};
#pragma unroll
    for (int i = 0; i < TVBA_SUMS; ++i) sums[i] = 0.0;
    bool all_ok = true;
    for (long long j = lane; j < q.count; j += TVBA_THREADS) {
        const long long row = q.a + j;
        if (!q.takes_part(row)) continue;
        all_ok = tvba_point_reduce(x, q.cal, point + 3 * row, q.uv + 4 * row, q.uv + 4 * row + 2, q.prior(row), q.opt, lam, sums) && all_ok;
    }
    if (!all_ok) sums[0] = NAN;
}

// a lane's points stepped for the cameras' step dc -> trial; sums [2] = its part of g . d and |d|^2
TVBA_HD inline void tvba_lane_step(const TvbaPair& q, int lane, const TvbaPose* pose, const double* point, double lam, const double* dc_in, double* trial,
                                   double* sums) {
    const TvbaPose x[2] = {pose[0], pose[1]};
    double dc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) dc[i] = dc_in[i];
    sums[0] = sums[1] = 0.0;
    for (long long j = lane; j < q.count; j += TVBA_THREADS) {
        const long long row = q.a + j;
        if (!q.takes_part(row)) continue;
        double dp[3], gtd;
        tvba_point_step(x, q.cal, point + 3 * row, q.uv + 4 * row, q.uv + 4 * row + 2, q.prior(row), q.opt, lam, dc, dp, gtd);
        trial[3 * row] = point[3 * row] + dp[0];
        trial[3 * row + 1] = point[3 * row + 1] + dp[1];
        trial[3 * row + 2] = point[3 * row + 2] + dp[2];
        sums[0] = sums[0] + gtd;
        sums[1] = sums[1] + (dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
    }
}

TVBA_HD inline void tvba_lane_accept(const TvbaPair& q, int lane, double* point, const double* trial) {
    for (long long j = lane; j < q.count; j += TVBA_THREADS) {
        const long long row = q.a + j;
        if (!q.takes_part(row)) continue;
        point[3 * row] = trial[3 * row];
        point[3 * row + 1] = trial[3 * row + 1];
        point[3 * row + 2] = trial[3 * row + 2];
    }
}

// the filter: valid = both reprojection errors finite, in front of the camera and under the threshold; returns the lane's count
TVBA_HD inline int tvba_lane_filter(const TvbaPair& q, int lane, const TvbaPose* pose, const double* point, double threshold, uint8_t* valid_mask) {
    const TvbaPose x[2] = {pose[0], pose[1]};
    int valid = 0;
    for (long long j = lane; j < q.count; j += TVBA_THREADS) {
        const long long row = q.a + j;
        if (!q.takes_part(row)) continue;
        const double e1 = tvba_error(x[0], q.cal[0], point + 3 * row, (double)q.uv[4 * row], (double)q.uv[4 * row + 1]);
        const double e2 = tvba_error(x[1], q.cal[1], point + 3 * row, (double)q.uv[4 * row + 2], (double)q.uv[4 * row + 3]);
        const bool ok = e1 < threshold && e2 < threshold;  // false for NaN
        valid_mask[row] = ok ? 1 : 0;
        valid += ok ? 1 : 0;
    }
    return valid;
}

// the four waves' sums of entry i (part: [TVBA_WAVES][n]) in the one fixed order
TVBA_HD inline double tvba_combine_waves(const double* part, int n, int i) { return (part[i] + part[n + i]) + (part[2 * n + i] + part[3 * n + i]); }

// camera 0 = identity, camera 1 = the inverse of Pose3(i2Ri1, i2Ui1)
TVBA_HD inline void tvba_initial_poses(const double* r_in, const double* t_in, TvbaPose* pose) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            pose[0].r[3 * i + j] = i == j ? 1.0 : 0.0;
            pose[1].r[3 * i + j] = r_in[3 * j + i];
        }
        pose[0].t[i] = 0.0;
        pose[1].t[i] = -(r_in[i] * t_in[0] + r_in[3 + i] * t_in[1] + r_in[6 + i] * t_in[2]);
    }
}

// One lane, once per trial: the combined sums [102] get the pose prior; the damped system is factored and the poses retracted.
// low [144], rhs [12], dc [12]: scratch / the cameras' step.
TVBA_HD inline void tvba_solve_trial(TvbaControl& ctl, double* sum, double pose_prior_inv_sigma, const TvbaPose* pose, TvbaPose* trial_pose, double* low,
                                     double* rhs, double* dc) {
    tvba_pose_prior(pose[0], pose_prior_inv_sigma, sum);
    for (int i = 0; i < 12; ++i) rhs[i] = sum[90 + i] - sum[78 + i];
    ctl.solves += 1;
    ctl.solved = tvba_cholesky12(sum, ctl.lam, rhs, low, dc) ? 1 : 0;
    ctl.accept = 0;
    if (ctl.solved) {
        tvba_retract(pose[0], dc, trial_pose[0]);
        tvba_retract(pose[1], dc + 6, trial_pose[1]);
    }
}

// One lane, once per trial: gtd / dd = g . d and |d|^2 over all variables, fresh = the trial's cost. Accepts or rejects, moves lambda, stops.
TVBA_HD inline void tvba_decide(TvbaControl& ctl, double gtd, double dd, double fresh, TvbaPose* pose, const TvbaPose* trial_pose) {
    const double lam = ctl.lam;
    if (ctl.solved) {
        const double model = -0.5 * gtd + 0.5 * lam * dd;
        if (isfinite(fresh) && model > 0.0 && (ctl.cost - fresh) / model > TVBA_MIN_FIDELITY) {
            const double dec = ctl.cost - fresh, rel = dec / ctl.cost;
            ctl.accept = 1;
            ctl.cost = fresh;
            ctl.accepted += 1;
            ctl.lam = lam / TVBA_LAMBDA_FACTOR;
            pose[0] = trial_pose[0];
            pose[1] = trial_pose[1];
            if (dec < TVBA_ABS_TOL || rel < TVBA_REL_TOL) ctl.stop = 1;
        }
    }
    if (!ctl.accept) {
        ctl.lam = lam * TVBA_LAMBDA_FACTOR;
        if (ctl.lam > TVBA_LAMBDA_UPPER) ctl.stop = 1;
    }
}

// i2Ti1 = wTi2.between(wTi1) with a unit translation, or NaN
TVBA_HD inline void tvba_relative_pose(const TvbaPose* pose, bool give_up, double* r_out, double* t_out) {
    if (give_up) {
        for (int i = 0; i < 9; ++i) r_out[i] = NAN;
        for (int i = 0; i < 3; ++i) t_out[i] = NAN;
        return;
    }
    const TvbaPose &x0 = pose[0], &x1 = pose[1];
    double t[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) r_out[3 * i + j] = x1.r[i] * x0.r[j] + x1.r[3 + i] * x0.r[3 + j] + x1.r[6 + i] * x0.r[6 + j];
        t[i] = x1.r[i] * (x0.t[0] - x1.t[0]) + x1.r[3 + i] * (x0.t[1] - x1.t[1]) + x1.r[6 + i] * (x0.t[2] - x1.t[2]);
    }
    const double norm = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int i = 0; i < 3; ++i) t_out[i] = t[i] / norm;
}

struct TvbaWorkspace {
    long long* track_off;  // [M + 1]
    int* image;            // [2 M]
    float* uv;             // [2 M][2]
    double* cams;          // [2 P][17]
    double* tri_point;     // [M][3]
    double* tri_avg;       // [M]
    int* tri_exit;         // [M]
    uint8_t* tri_mask;     // [2 M]
    int* tri_stats;        // [M][4]
    double* trial;         // [M][3]
    int* flags;            // [0]: match_off_dev not ascending within 0 .. M
    void* tri_ws;
    size_t tri_ws_bytes;
    size_t bytes;
};

TvbaWorkspace tvba_layout(void* base, long long num_pairs, long long total) {
    TvbaWorkspace w;
    WorkspaceCarver ws{base, 0};
    const size_t m = (size_t)total, p = (size_t)num_pairs;
    w.track_off = (long long*)ws.take((m + 1) * 8);
    w.image = (int*)ws.take(2 * m * 4);
    w.uv = (float*)ws.take(4 * m * 4);
    w.cams = (double*)ws.take(2 * p * 17 * 8);
    w.tri_point = (double*)ws.take(3 * m * 8);
    w.tri_avg = (double*)ws.take(m * 8);
    w.tri_exit = (int*)ws.take(m * 4);
    w.tri_mask = (uint8_t*)ws.take(2 * m);
    w.tri_stats = (int*)ws.take(4 * m * 4);
    w.trial = (double*)ws.take(3 * m * 8);
    w.flags = (int*)ws.take(16);
    w.tri_ws_bytes = gtsfm_triangulate_workspace_bytes(total, 2 * total, 0);
    w.tri_ws = ws.take(w.tri_ws_bytes);
    w.bytes = ws.used;
    return w;
}

// every row: a track of two measurements without cameras (rows that belong to no pair, or are not verified, stay so)
TVBA_HD inline void tvba_init_rows(long long first, long long stride, long long total, long long* __restrict__ track_off, int* __restrict__ image,
                                   float* __restrict__ uv) {
    for (long long r = first; r <= total; r += stride) {
        track_off[r] = 2 * r;
        if (r < total) {
            image[2 * r] = image[2 * r + 1] = -1;
            uv[4 * r] = uv[4 * r + 1] = uv[4 * r + 2] = uv[4 * r + 3] = 0.0f;
        }
    }
}

__global__ __launch_bounds__(TVBA_THREADS) void tvba_init_kernel(long long total, long long* __restrict__ track_off, int* __restrict__ image,
                                                                  float* __restrict__ uv) {
    tvba_init_rows((long long)blockIdx.x * TVBA_THREADS + threadIdx.x, (long long)gridDim.x * TVBA_THREADS, total, track_off, image, uv);
}

// the rows a pair owns, clamped into 0 .. total; count = how many of them are matches
TVBA_HD inline void tvba_pair_rows(const long long* __restrict__ match_off, const int* __restrict__ match_count, int p, long long total, long long& a,
                                      long long& count, bool& bad) {
    a = match_off[p];
    long long b = match_off[p + 1];
    bad = a < 0 || b < a || b > total;
    if (bad) a = b = 0;
    count = b - a;
    if (match_count) {
        const long long c = match_count[p];
        count = c < 0 ? 0 : (c < count ? c : count);
    }
}

// pair p: its two cameras (lane 0), and the measurements of its verified rows lane, lane + stride, ...
TVBA_HD inline void tvba_prepare_pair(int p, int lane, int stride, const float* __restrict__ kp_xy, const long long* __restrict__ kp_off1,
                                      const long long* __restrict__ kp_off2, const int* __restrict__ match_idx, const long long* __restrict__ match_off,
                                      const int* __restrict__ match_count, const uint8_t* __restrict__ inlier_mask, long long total,
                                      const double* __restrict__ intrinsics, const double* __restrict__ rotation, const double* __restrict__ translation,
                                      int* __restrict__ image, float* __restrict__ uv, double* __restrict__ cams, int* flags) {
    long long a, count;
    bool bad;
    tvba_pair_rows(match_off, match_count, p, total, a, count, bad);
    if (lane == 0) {
        if (bad) flags[0] = 1;
        const double *r = rotation + 9 * (long long)p, *t = translation + 3 * (long long)p, *k = intrinsics + 8 * (long long)p;
        bool finite = true;
        for (int i = 0; i < 9; ++i) finite = finite && isfinite(r[i]);
        for (int i = 0; i < 3; ++i) finite = finite && isfinite(t[i]);
        double* c0 = cams + 34 * (long long)p;
        double* c1 = c0 + 17;
        c0[0] = c1[0] = finite ? 1.0 : 0.0;
        for (int i = 0; i < 4; ++i) {
            c0[1 + i] = k[i];
            c1[1 + i] = k[4 + i];
        }
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                c0[5 + 3 * i + j] = i == j ? 1.0 : 0.0;
                c1[5 + 3 * i + j] = r[3 * j + i];  // camera 1 = the inverse of Pose3(i2Ri1, i2Ui1)
            }
            c0[14 + i] = 0.0;
            c1[14 + i] = -(r[i] * t[0] + r[3 + i] * t[1] + r[6 + i] * t[2]);
        }
    }
    const float* xy1 = kp_xy + 2 * kp_off1[p];
    const float* xy2 = kp_xy + 2 * kp_off2[p];
    for (long long j = lane; j < count; j += stride) {
        const long long row = a + j;
        if (!inlier_mask[row]) continue;
        const long long i1 = match_idx[2 * row], i2 = match_idx[2 * row + 1];
        if (i1 < 0 || i2 < 0) continue;  // not a keypoint: the row stays without cameras
        image[2 * row] = 2 * p;
        image[2 * row + 1] = 2 * p + 1;
        uv[4 * row] = xy1[2 * i1];
        uv[4 * row + 1] = xy1[2 * i1 + 1];
        uv[4 * row + 2] = xy2[2 * i2];
        uv[4 * row + 3] = xy2[2 * i2 + 1];
    }
}

// one workgroup per pair
__global__ __launch_bounds__(TVBA_THREADS) void tvba_prepare_kernel(const float* __restrict__ kp_xy, const long long* __restrict__ kp_off1,
                                                                     const long long* __restrict__ kp_off2, const int* __restrict__ match_idx,
                                                                     const long long* __restrict__ match_off, const int* __restrict__ match_count,
                                                                     const uint8_t* __restrict__ inlier_mask, long long total,
                                                                     const double* __restrict__ intrinsics, const double* __restrict__ rotation,
                                                                     const double* __restrict__ translation, int* __restrict__ image, float* __restrict__ uv,
                                                                     double* __restrict__ cams, int* flags) {
    tvba_prepare_pair(blockIdx.x, threadIdx.x, TVBA_THREADS, kp_xy, kp_off1, kp_off2, match_idx, match_off, match_count, inlier_mask, total, intrinsics, rotation,
                      translation, image, uv, cams, flags);
}

// sums [N] of every lane -> out [N] in LDS, the same bits whatever the lane; part: [TVBA_WAVES][N] of LDS
template <int N>
__device__ inline void tvba_block_sum(const double* sums, double* part, double* out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = sums[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
        if (lane == 0) part[wave * N + i] = v;
    }
    __syncthreads();
    for (int i = tid; i < N; i += TVBA_THREADS) out[i] = tvba_combine_waves(part, N, i);
    __syncthreads();
}

__global__ __launch_bounds__(TVBA_THREADS) void tvba_adjust_kernel(const long long* __restrict__ match_off, const int* __restrict__ match_count,
                                                                    const uint8_t* __restrict__ inlier_mask, long long total,
                                                                    const double* __restrict__ intrinsics, const double* __restrict__ rotation,
                                                                    const double* __restrict__ translation, const float* __restrict__ uv,
                                                                    const double* __restrict__ tri_point, const int* __restrict__ tri_exit,
                                                                    double* __restrict__ trial, int max_iterations, double reproj_threshold,
                                                                    TvbaOptions opt, int min_verified, int allow_indeterminate,
                                                                    double* __restrict__ rotation_out, double* __restrict__ translation_out,
                                                                    uint8_t* __restrict__ valid_mask, double* __restrict__ point, double* __restrict__ cost_out,
                                                                    int* __restrict__ stats) {
    __shared__ double s_part[TVBA_WAVES * TVBA_SUMS], s_sum[TVBA_SUMS], s_low[144], s_dc[12], s_rhs[12];
    __shared__ TvbaPose s_pose[2], s_trial_pose[2];
    __shared__ TvbaControl s_ctl;
    __shared__ int s_count[3];
    __shared__ long long s_first;
    const int p = blockIdx.x, tid = threadIdx.x;
    long long a, count;
    bool bad;
    tvba_pair_rows(match_off, match_count, p, total, a, count, bad);
    long long owned = match_off[p + 1] - match_off[p];  // every row of the slice gets its outputs, matches or not
    if (bad) owned = 0;

    if (tid == 0) {
        s_count[0] = s_count[1] = s_count[2] = 0;
        s_first = count;
    }
    __syncthreads();
    {
        int verified = 0, triangulated = 0;
        long long first = count;
        for (long long j = tid; j < owned; j += TVBA_THREADS) {
            const long long row = a + j;
            const bool active = j < count && inlier_mask[row] != 0;
            const bool ok = active && tri_exit[row] == 0;
            verified += active ? 1 : 0;
            triangulated += ok ? 1 : 0;
            if (ok && j < first) first = j;
            point[3 * row] = ok ? tri_point[3 * row] : NAN;
            point[3 * row + 1] = ok ? tri_point[3 * row + 1] : NAN;
            point[3 * row + 2] = ok ? tri_point[3 * row + 2] : NAN;
            valid_mask[row] = 0;
        }
        atomicAdd(&s_count[0], verified);
        atomicAdd(&s_count[1], triangulated);
        atomicMin((unsigned long long*)&s_first, (unsigned long long)first);
    }
    __syncthreads();
    const int verified = s_count[0], triangulated = s_count[1];
    const long long first_row = a + s_first;

    const double* r_in = rotation + 9 * (long long)p;
    const double* t_in = translation + 3 * (long long)p;
    bool finite = true;
    for (int i = 0; i < 9; ++i) finite = finite && isfinite(r_in[i]);
    for (int i = 0; i < 3; ++i) finite = finite && isfinite(t_in[i]);
    int status = TVBA_OK;
    if (verified < min_verified) status = TVBA_SKIPPED;
    else if (!finite) status = TVBA_NO_INITIAL_POSE;
    else if (triangulated == 0) status = TVBA_NONE_TRIANGULATED;

    if (status != TVBA_OK) {  // uniform over the workgroup
        const bool keep_pose = status != TVBA_NO_INITIAL_POSE, keep_rows = status != TVBA_NONE_TRIANGULATED;
        int valid = 0;
        for (long long j = tid; j < owned; j += TVBA_THREADS) {
            const long long row = a + j;
            const bool active = j < count && inlier_mask[row] != 0;
            valid_mask[row] = keep_rows && active ? 1 : 0;
            point[3 * row] = point[3 * row + 1] = point[3 * row + 2] = NAN;
        }
        valid = keep_rows ? verified : 0;
        if (tid < 9) rotation_out[9 * (long long)p + tid] = keep_pose ? r_in[tid] : NAN;
        if (tid < 3) translation_out[3 * (long long)p + tid] = keep_pose ? t_in[tid] : NAN;
        if (tid < 2) cost_out[2 * (long long)p + tid] = NAN;
        if (tid == 0) {
            int* s = stats + 8 * (long long)p;
            s[0] = status;
            s[1] = verified;
            s[2] = status == TVBA_SKIPPED ? 0 : triangulated;  // the reference does not triangulate a pair it skips
            s[3] = valid;
            s[4] = s[5] = s[6] = s[7] = 0;
        }
        return;
    }

    TvbaPair q;
    q.a = a;
    q.count = count;
    q.first_row = first_row;
    q.inlier_mask = inlier_mask;
    q.tri_exit = tri_exit;
    q.uv = uv;
    q.opt = opt;
    {
        const double* k = intrinsics + 8 * (long long)p;
        q.cal[0].fx = k[0], q.cal[0].fy = k[1], q.cal[0].cx = k[2], q.cal[0].cy = k[3];
        q.cal[1].fx = k[4], q.cal[1].fy = k[5], q.cal[1].cx = k[6], q.cal[1].cy = k[7];
        for (int i = 0; i < 3; ++i) q.prior_at[i] = tri_point[3 * first_row + i];
    }
    if (tid == 0) {
        tvba_initial_poses(r_in, t_in, s_pose);
        s_ctl.lam = TVBA_LAMBDA_INITIAL;
        s_ctl.accepted = s_ctl.solves = s_ctl.stop = s_ctl.solved = s_ctl.accept = 0;
    }
    __syncthreads();

    // the cost of `values` at `pose`: every lane's points in row order, then the tree; -> s_sum[0]
    auto total_cost = [&](const TvbaPose* pose, const double* values) {
        const double c[1] = {tvba_lane_cost(q, tid, pose, values)};
        tvba_block_sum<1>(c, s_part, s_sum);
    };
    // the points' part of the reduced camera system at damping lam -> s_sum [102]
    auto reduced_system = [&](double lam) {
        double sums[TVBA_SUMS];
        tvba_lane_reduce(q, tid, s_pose, point, lam, sums);
        tvba_block_sum<TVBA_SUMS>(sums, s_part, s_sum);
    };

    total_cost(s_pose, point);
    if (tid == 0) s_ctl.cost = s_ctl.first_cost = s_sum[0] + tvba_pose_prior(s_pose[0], opt.pose_prior_inv_sigma, nullptr);
    __syncthreads();

    while (s_ctl.accepted < max_iterations && !s_ctl.stop) {  // uniform: s_ctl changes between barriers only
        const double lam = s_ctl.lam;
        reduced_system(lam);
        if (tid == 0) tvba_solve_trial(s_ctl, s_sum, opt.pose_prior_inv_sigma, s_pose, s_trial_pose, s_low, s_rhs, s_dc);
        __syncthreads();
        double gtd = 0.0, dd = 0.0;
        if (s_ctl.solved) {
            double sums[2];
            tvba_lane_step(q, tid, s_pose, point, lam, s_dc, trial, sums);
            for (int i = 0; i < 12; ++i) {  // s_sum is about to be overwritten: the cameras' part first
                gtd = gtd + s_sum[78 + i] * s_dc[i];
                dd = dd + s_dc[i] * s_dc[i];
            }
            __syncthreads();
            tvba_block_sum<2>(sums, s_part, s_sum);
            gtd = gtd + s_sum[0];
            dd = dd + s_sum[1];
            __syncthreads();
            total_cost(s_trial_pose, trial);  // a lane reads the trial points it wrote itself
        }
        if (tid == 0) tvba_decide(s_ctl, gtd, dd, s_ctl.solved ? s_sum[0] + tvba_pose_prior(s_trial_pose[0], opt.pose_prior_inv_sigma, nullptr) : NAN, s_pose, s_trial_pose);
        __syncthreads();
        if (s_ctl.accept) tvba_lane_accept(q, tid, point, trial);
    }

    // the undamped system at the final values
    reduced_system(0.0);
    if (tid == 0) {
        tvba_pose_prior(s_pose[0], opt.pose_prior_inv_sigma, s_sum);
        s_ctl.solved = tvba_cholesky12(s_sum, 0.0, nullptr, s_low, nullptr) ? 1 : 0;
        s_count[2] = 0;
    }
    __syncthreads();
    const bool indeterminate = !s_ctl.solved;
    const bool give_up = indeterminate && !allow_indeterminate;
    const int valid = give_up ? 0 : tvba_lane_filter(q, tid, s_pose, point, reproj_threshold, valid_mask);
    atomicAdd(&s_count[2], valid);
    __syncthreads();
    if (tid == 0) {
        tvba_relative_pose(s_pose, give_up, rotation_out + 9 * (long long)p, translation_out + 3 * (long long)p);
        cost_out[2 * (long long)p] = s_ctl.first_cost;
        cost_out[2 * (long long)p + 1] = s_ctl.cost;
        int* s = stats + 8 * (long long)p;
        s[0] = indeterminate ? TVBA_INDETERMINATE : TVBA_OK;
        s[1] = verified;
        s[2] = triangulated;
        s[3] = s_count[2];
        s[4] = s_ctl.accepted;
        s[5] = s_ctl.solves;
        s[6] = s[7] = 0;
    }
}

}  // namespace

extern "C" size_t gtsfm_two_view_ba_workspace_bytes(long long num_pairs, long long total_matches) {
    if (num_pairs < 0 || total_matches < 0 || num_pairs >= (1ll << 30) || total_matches >= (1ll << 30)) return 0;
    return tvba_layout(nullptr, num_pairs, total_matches).bytes;
}

extern "C" int gtsfm_two_view_ba_f64(const float* kp_xy_dev, const long long* kp_off1_dev, const long long* kp_off2_dev, const int32_t* match_idx_dev,
                                     const long long* match_off_dev, const int32_t* match_count_dev, long long total_matches,
                                     const uint8_t* inlier_mask_dev, const double* intrinsics_dev, const double* rotation_dev,
                                     const double* translation_dev, int num_pairs, int max_iterations, double reproj_error_threshold, double huber_k,
                                     double measurement_sigma, double pose_prior_sigma, double point_prior_sigma, int min_verified,
                                     int allow_indeterminate, double triangulation_threshold, double triangulation_min_angle_deg, void* workspace_dev,
                                     size_t workspace_bytes, double* rotation_out_dev, double* translation_out_dev, uint8_t* valid_mask_dev,
                                     double* point_dev, double* cost_dev, int32_t* stats_dev, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GTSFM_CHECK_ARG(num_pairs >= 0 && total_matches >= 0 && num_pairs < (1 << 30) && total_matches < (1ll << 30),
                    "gtsfm_two_view_ba_f64: size out of range (%d pairs, %lld matches)", num_pairs, total_matches);
    GTSFM_CHECK_ARG(max_iterations >= 0, "gtsfm_two_view_ba_f64: max_iterations %d is negative", max_iterations);
    GTSFM_CHECK_ARG(reproj_error_threshold > 0.0, "gtsfm_two_view_ba_f64: reproj_error_threshold %g must be positive (infinity allowed)", reproj_error_threshold);
    GTSFM_CHECK_ARG(huber_k > 0.0, "gtsfm_two_view_ba_f64: huber_k %g must be positive (infinity: no robust loss)", huber_k);
    GTSFM_CHECK_ARG(measurement_sigma > 0.0 && pose_prior_sigma > 0.0 && point_prior_sigma > 0.0 && isfinite(measurement_sigma) && isfinite(pose_prior_sigma) &&
                        isfinite(point_prior_sigma),
                    "gtsfm_two_view_ba_f64: sigmas %g / %g / %g must be positive and finite", measurement_sigma, pose_prior_sigma, point_prior_sigma);
    GTSFM_CHECK_ARG(triangulation_threshold > 0.0, "gtsfm_two_view_ba_f64: triangulation_threshold %g must be positive (infinity allowed)", triangulation_threshold);
    GTSFM_CHECK_ARG(triangulation_min_angle_deg == triangulation_min_angle_deg, "gtsfm_two_view_ba_f64: triangulation_min_angle_deg is NaN");
    if (num_pairs == 0) return GTSFM_OK;
    GTSFM_CHECK_ARG(kp_off1_dev && kp_off2_dev && match_off_dev && intrinsics_dev && rotation_dev && translation_dev && workspace_dev && rotation_out_dev &&
                        translation_out_dev && cost_dev && stats_dev,
                    "gtsfm_two_view_ba_f64: null pointer");
    GTSFM_CHECK_ARG(total_matches == 0 || (kp_xy_dev && match_idx_dev && inlier_mask_dev && valid_mask_dev && point_dev),
                    "gtsfm_two_view_ba_f64: null match pointer");
    GTSFM_CHECK_ARG(total_matches == 0 || valid_mask_dev != inlier_mask_dev, "gtsfm_two_view_ba_f64: valid_mask_dev must not be inlier_mask_dev");
    GTSFM_CHECK_ARG(((uintptr_t)workspace_dev & 255) == 0, "gtsfm_two_view_ba_f64: the workspace must be aligned to 256 bytes");
    const TvbaWorkspace w = tvba_layout(workspace_dev, num_pairs, total_matches);
    if (workspace_bytes < w.bytes) {
        gtsfm_set_error("gtsfm_two_view_ba_f64: workspace of %zu bytes, %zu needed for %d pairs / %lld matches", workspace_bytes, w.bytes, num_pairs, total_matches);
        return GTSFM_ERR_WORKSPACE;
    }
    if (hipMemsetAsync(w.flags, 0, 16, stream) != hipSuccess) {
        gtsfm_set_error("gtsfm_two_view_ba_f64: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
        return GTSFM_ERR_HIP;
    }
    const dim3 threads(TVBA_THREADS);
    const long long want = (total_matches + TVBA_THREADS) / TVBA_THREADS;
    hipLaunchKernelGGL(tvba_init_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), threads, 0, stream, total_matches, w.track_off, w.image, w.uv);
    GTSFM_CHECK_LAUNCH("tvba_init_kernel");
    hipLaunchKernelGGL(tvba_prepare_kernel, dim3((unsigned)num_pairs), threads, 0, stream, kp_xy_dev, kp_off1_dev, kp_off2_dev, match_idx_dev, match_off_dev,
                       match_count_dev, inlier_mask_dev, total_matches, intrinsics_dev, rotation_dev, translation_dev, w.image, w.uv, w.cams, w.flags);
    GTSFM_CHECK_LAUNCH("tvba_prepare_kernel");
    if (total_matches > 0) {
        const int rc = gtsfm_triangulate_tracks_f64(w.track_off, w.image, w.uv, total_matches, 2 * total_matches, w.cams, 2 * num_pairs, 0, triangulation_threshold,
                                                    triangulation_min_angle_deg, 0, 0ull, w.tri_ws, w.tri_ws_bytes, w.tri_point, w.tri_avg, w.tri_exit, w.tri_mask,
                                                    w.tri_stats, stream_);
        if (rc != GTSFM_OK) return rc;
    }
    TvbaOptions opt;
    opt.huber_k = huber_k;
    opt.inv_sigma = 1.0 / measurement_sigma;
    opt.pose_prior_inv_sigma = 1.0 / pose_prior_sigma;
    opt.point_prior_inv_var = 1.0 / (point_prior_sigma * point_prior_sigma);
    hipLaunchKernelGGL(tvba_adjust_kernel, dim3((unsigned)num_pairs), threads, 0, stream, match_off_dev, match_count_dev, inlier_mask_dev, total_matches,
                       intrinsics_dev, rotation_dev, translation_dev, w.uv, w.tri_point, w.tri_exit, w.trial, max_iterations, reproj_error_threshold, opt,
                       min_verified, allow_indeterminate, rotation_out_dev, translation_out_dev, valid_mask_dev, point_dev, cost_dev, stats_dev);
    GTSFM_CHECK_LAUNCH("tvba_adjust_kernel");
    int flag[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(flag, w.flags, sizeof(flag), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        gtsfm_set_error("gtsfm_two_view_ba_f64: failed: %s", hipGetErrorString(hipGetLastError()));
        return GTSFM_ERR_HIP;
    }
    GTSFM_CHECK_ARG(!flag[0], "gtsfm_two_view_ba_f64: match_off_dev is not ascending within 0 .. %lld; such pairs were treated as empty", total_matches);
    return GTSFM_OK;
}
