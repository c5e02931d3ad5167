// Triangulation of feature tracks on the device: what Point3dInitializer.triangulate does per track
// (gtsfm/data_association/point3d_initializer.py:139-295, called from data_assoc.py:205-273), for all tracks of a scene in one call.
// See include/gtsfm_amd.h; the specification is tests/triangulation_reference.py, float64 throughout.
//
// PARITY UNPINNED towards gtsam: gtsam.triangulatePoint3(rank_tol=1e-9, optimize=True) is restated (DLT, a fixed number of damped
// Gauss-Newton steps instead of Levenberg-Marquardt's data-dependent stop, cheirality), and np.random.choice is replaced by a
// counter-based sampler (the verifier's splitmix64).
//
// Mapping (the work is ragged: most tracks have 2 - 6 measurements, 1 - 15 pairs; a few have dozens):
//   count      : per track, hypotheses = min(C(n,2), num_hypotheses) (0 without RANSAC); validates the offsets.
//   scan       : one workgroup, exclusive prefix sum -> hyp_off [T + 1].
//   select     : only tracks with more pairs than hypotheses (one workgroup each, the others leave at once): a pair's rank among the
//                track's sampling keys is counted against every other pair; rank < hypotheses takes slot hyp_off[t] + rank.
//   hypothesis : one LANE per (track, hypothesis), grid-stride over hyp_off[T]: two-view DLT, the fixed damped steps, cheirality, then a
//                serial walk over the track's measurements in order: votes and mean inlier error -> one 16-byte record.
//   final      : one lane per track: a serial pass over its records with the key (votes descending, mean error ascending, pair index
//                ascending), so the winner does not depend on which lane computed which record; the winner's point is recomputed (same
//                code, same bits) for the inlier mask; then the n-view DLT, refinement, errors, angle test and exit code.
// Every sum over a track's measurements is a serial loop in measurement order inside one lane: no atomics, no cross-lane reduction, so
// the outputs of a track depend on that track's data and the options only -- not on the batch, the grid or the run.
// The stages are one function over a runner of stage_runner.h (tri_triangulate_stages): the device call launches them,
// tools/triangulation_host_main.cpp walks the same function on a CPU.
//
// DLT without squaring the condition number: the rows u P2 - P0, v P2 - P1 are rotated one by one into a 4 x 4 upper triangle (Givens,
// O(1) state for any track length), whose singular values and last right singular vector come from a one-sided Jacobi (Hestenes) with
// a fixed number of sweeps. rank_tol = 1e-9 is far below what eigenvalues of A^T A (entries ~ f^2) could resolve.

#include <math.h>

#include "../../include/gtsfm_amd.h"
#include "stage_runner.h"

#define TRI_THREADS 256
#define TRI_FINAL_THREADS 64  // one wave per workgroup: 11 789 tracks spread over 185 CUs instead of 47
#define TRI_GN_STEPS 8
#define TRI_JACOBI_SWEEPS 10
#define TRI_RANK_TOL 1.0e-9
#define TRI_LAMBDA_INITIAL 1.0e-5
#define TRI_LAMBDA_FACTOR 10.0
#define TRI_LAMBDA_FLOOR 1.0e-20
#define TRI_MAX_ERROR 3.4028234663852886e38  // float32's maximum (MAX_TRACK_REPROJ_ERROR)
#define TRI_MAX_TRACK_LENGTH 65535           // C(n, 2) stays below 2^31
#define TRI_HYP_BLOCKS 2048
// the per-track arithmetic also compiles for the host, where a stand-alone program can run it under a sanitizer
#define TRI_HD __host__ __device__

enum { TRI_NO_RANSAC = 0, TRI_UNIFORM = 1, TRI_BIASED = 2, TRI_TOPK = 3 };
enum { TRI_SUCCESS = 0, TRI_CHEIRALITY = 1, TRI_INLIERS = 2, TRI_POSES = 3, TRI_EXCEEDS = 4, TRI_LOW_ANGLE = 5 };

namespace {

struct TriHyp {
    int votes;  // -1: skipped (camera missing, underconstrained, numeric failure or cheirality)
    int pair;
    double mean;
};

struct TriWorkspace {
    long long* hyp_off;  // [T + 1]
    TriHyp* hyp;         // [cap]
    int* sel;            // [cap]
    int* flags;          // [0]: bad offsets / too long a track, [1]: more hypotheses than the workspace holds
    long long cap;
    size_t bytes;
};

// sum over tracks of min(C(n,2), H) <= min(T * H, sum n * sqrt(H / 2)), since min(a, b) <= sqrt(a b) and C(n,2) <= n^2 / 2
long long tri_hyp_capacity(long long num_tracks, long long total, long long max_hyp) {
    if (max_hyp <= 0) return 16;
    const double by_tracks = (double)num_tracks * (double)max_hyp;
    const double by_meas = (double)total * sqrt((double)max_hyp / 2.0) + (double)num_tracks;
    const double cap = (by_tracks < by_meas ? by_tracks : by_meas) + 16.0;
    return cap > 4.0e18 ? -1 : (long long)cap;
}

TriWorkspace tri_layout(void* base, long long num_tracks, long long total, long long max_hyp) {
    TriWorkspace w;
    WorkspaceCarver ws{base, 0};
    w.cap = tri_hyp_capacity(num_tracks, total, max_hyp);
    const size_t cap = w.cap < 0 ? 0 : (size_t)w.cap;
    w.hyp_off = (long long*)ws.take(((size_t)num_tracks + 1) * 8);
    w.hyp = (TriHyp*)ws.take(cap * sizeof(TriHyp));
    w.sel = (int*)ws.take(cap * 4);
    w.flags = (int*)ws.take(16);
    w.bytes = ws.used;
    return w;
}

struct TriCam {
    double fx, fy, cx, cy, r[9], t[3];
};

TRI_HD inline bool tri_load_cam(const double* __restrict__ cams, int num_images, int i, TriCam& c) {
    if (i < 0 || i >= num_images) return false;
    const double* p = cams + (long long)i * 17;
    if (p[0] == 0.0) return false;
    c.fx = p[1];
    c.fy = p[2];
    c.cx = p[3];
    c.cy = p[4];
#pragma unroll
    for (int k = 0; k < 9; ++k) c.r[k] = p[5 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) c.t[k] = p[14 + k];
    return true;
}

TRI_HD inline unsigned long long tri_splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// camera coordinates of x: wRc^T (x - wtc)
TRI_HD inline void tri_to_camera(const TriCam& c, const double* x, double& p0, double& p1, double& p2) {
    const double d0 = x[0] - c.t[0], d1 = x[1] - c.t[1], d2 = x[2] - c.t[2];
    p0 = c.r[0] * d0 + c.r[3] * d1 + c.r[6] * d2;
    p1 = c.r[1] * d0 + c.r[4] * d1 + c.r[7] * d2;
    p2 = c.r[2] * d0 + c.r[5] * d1 + c.r[8] * d2;
}

// rotates one row into the upper triangle R (a is destroyed)
TRI_HD inline void tri_givens_row(double R[4][4], double* a) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double r = sqrt(R[j][j] * R[j][j] + a[j] * a[j]);
        if (a[j] == 0.0 || !(r > 0.0)) continue;
        const double c = R[j][j] / r, s = a[j] / r;
#pragma unroll
        for (int k = j; k < 4; ++k) {
            const double t = c * R[j][k] + s * a[k];
            a[k] = c * a[k] - s * R[j][k];
            R[j][k] = t;
        }
    }
}

// the two DLT rows of one measurement: u P2 - P0 and v P2 - P1 with P = K [wRc^T | -wRc^T wtc]
TRI_HD inline void tri_dlt_add(double R[4][4], const TriCam& c, double u, double v) {
    double P[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        P[j][0] = c.r[j];
        P[j][1] = c.r[3 + j];
        P[j][2] = c.r[6 + j];
        P[j][3] = -(c.r[j] * c.t[0] + c.r[3 + j] * c.t[1] + c.r[6 + j] * c.t[2]);
    }
    double a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[k] = u * P[2][k] - (c.fx * P[0][k] + c.cx * P[2][k]);
        b[k] = v * P[2][k] - (c.fy * P[1][k] + c.cy * P[2][k]);
    }
    tri_givens_row(R, a);
    tri_givens_row(R, b);
}

// singular values and the last right singular vector of the triangle; false when fewer than 3 exceed rank_tol or the point is not finite
TRI_HD bool tri_dlt_solve(double G[4][4], double* x) {
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < TRI_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    alpha += G[i][p] * G[i][p];
                    beta += G[i][q] * G[i][q];
                    gamma += G[i][p] * G[i][q];
                }
                if (!(fabs(gamma) > 1.0e-17 * sqrt(alpha * beta))) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double gp = G[i][p], gq = G[i][q];
                    G[i][p] = c * gp - s * gq;
                    G[i][q] = s * gp + c * gq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
    }
    int rank = 0, last = 0;
    double smallest = INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double sigma = sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j] + G[3][j] * G[3][j]);
        rank += sigma > TRI_RANK_TOL ? 1 : 0;
        if (sigma < smallest) {
            smallest = sigma;
            last = j;
        }
    }
    if (rank < 3) return false;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j == last) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = V[i][j];
        }
    x[0] = v[0] / v[3];
    x[1] = v[1] / v[3];
    x[2] = v[2] / v[3];
    return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
}

// (H + lam I) d = -g, H's upper triangle as h[6]; elimination without pivoting, false for a pivot that is not positive
TRI_HD inline bool tri_solve_spd3(const double* h, const double* g, double lam, double* d) {
    const double a00 = h[0] + lam, a01 = h[1], a02 = h[2];
    double a11 = h[3] + lam, a12 = h[4], a22 = h[5] + lam;
    const double b0 = -g[0];
    double b1 = -g[1], b2 = -g[2];
    if (!(a00 > 0.0)) return false;
    const double l10 = a01 / a00, l20 = a02 / a00;
    a11 = a11 - l10 * a01;
    a12 = a12 - l10 * a02;
    a22 = a22 - l20 * a02;
    b1 = b1 - l10 * b0;
    b2 = b2 - l20 * b0;
    if (!(a11 > 0.0)) return false;
    const double l21 = a12 / a11;
    a22 = a22 - l21 * a12;
    b2 = b2 - l21 * b1;
    if (!(a22 > 0.0)) return false;
    d[2] = b2 / a22;
    d[1] = (b1 - a12 * d[2]) / a11;
    d[0] = (b0 - a01 * d[1] - a02 * d[2]) / a00;
    return isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
}

TRI_HD inline void tri_accumulate(const TriCam& c, const double* x, double u, double v, double& cost, double* h, double* g) {
    double p0, p1, p2;
    tri_to_camera(c, x, p0, p1, p2);
    const double ru = c.fx * p0 / p2 + c.cx - u, rv = c.fy * p1 / p2 + c.cy - v;
    const double a = 1.0 / p2, b0 = c.fx * p0 / (p2 * p2), b1 = c.fy * p1 / (p2 * p2);
    double ju[3], jv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ju[k] = c.fx * a * c.r[3 * k] - b0 * c.r[3 * k + 2];
        jv[k] = c.fy * a * c.r[3 * k + 1] - b1 * c.r[3 * k + 2];
    }
    cost += 0.5 * (ru * ru + rv * rv);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[i] += ju[i] * ru + jv[i] * rv;
#pragma unroll
        for (int j = i; j < 3; ++j) h[k++] += ju[i] * ju[j] + jv[i] * jv[j];
    }
}

TRI_HD inline double tri_cost_term(const TriCam& c, const double* x, double u, double v) {
    double p0, p1, p2;
    tri_to_camera(c, x, p0, p1, p2);
    const double du = c.fx * p0 / p2 + c.cx - u, dv = c.fy * p1 / p2 + c.cy - v;
    return 0.5 * (du * du + dv * dv);
}

// reprojection error in pixels; NaN for depth <= 0
TRI_HD inline double tri_error(const TriCam& c, const double* x, double u, double v) {
    double p0, p1, p2;
    tri_to_camera(c, x, p0, p1, p2);
    if (!(p2 > 0.0)) return NAN;
    const double du = c.fx * p0 / p2 + c.cx - u, dv = c.fy * p1 / p2 + c.cy - v;
    return sqrt(du * du + dv * dv);
}

// The measurements a triangulation uses. Src::count() and Src::get(j, cam, u, v) -> false for one that is not used.
struct TriPairSrc {
    TriCam cam[2];
    double uv[2][2];
    TRI_HD inline int count() const { return 2; }
    TRI_HD inline bool get(int j, TriCam& c, double& u, double& v) const {
        c = j == 0 ? cam[0] : cam[1];
        u = j == 0 ? uv[0][0] : uv[1][0];
        v = j == 0 ? uv[0][1] : uv[1][1];
        return true;
    }
};

struct TriTrackSrc {  // the inliers of a track whose camera is estimated
    const double* cams;
    int num_images;
    const int* image;
    const float* uv;
    const uint8_t* mask;
    int n;
    TRI_HD inline int count() const { return n; }
    TRI_HD inline bool get(int j, TriCam& c, double& u, double& v) const {
        if (!mask[j]) return false;
        u = (double)uv[2 * j];
        v = (double)uv[2 * j + 1];
        return tri_load_cam(cams, num_images, image[j], c);
    }
};

// gtsam.triangulatePoint3(rank_tol = 1e-9, optimize = true); false where it raises
template <class Src>
TRI_HD bool tri_triangulate(const Src& src, double* x) {
    const int n = src.count();
    TriCam c;
    double u, v;
    {
        double R[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) R[i][j] = 0.0;
        for (int j = 0; j < n; ++j)
            if (src.get(j, c, u, v)) tri_dlt_add(R, c, u, v);
        if (!tri_dlt_solve(R, x)) return false;
    }
    double lam = TRI_LAMBDA_INITIAL;
    for (int step = 0; step < TRI_GN_STEPS; ++step) {
        double e = 0.0, h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, d[3];
        for (int j = 0; j < n; ++j)
            if (src.get(j, c, u, v)) tri_accumulate(c, x, u, v, e, h, g);
        if (!tri_solve_spd3(h, g, lam, d)) return false;
        const double xn[3] = {x[0] + d[0], x[1] + d[1], x[2] + d[2]};
        double en = 0.0;
        for (int j = 0; j < n; ++j)
            if (src.get(j, c, u, v)) en += tri_cost_term(c, xn, u, v);
        if (isfinite(en) && !(en > e)) {
            x[0] = xn[0];
            x[1] = xn[1];
            x[2] = xn[2];
            lam = fmax(lam / TRI_LAMBDA_FACTOR, TRI_LAMBDA_FLOOR);
        } else {
            lam = lam * TRI_LAMBDA_FACTOR;
        }
    }
    for (int j = 0; j < n; ++j)
        if (src.get(j, c, u, v)) {
            double p0, p1, p2;
            tri_to_camera(c, x, p0, p1, p2);
            if (!(p2 > 0.0)) return false;
        }
    return true;
}

// pair index in itertools.combinations order -> (k1, k2)
TRI_HD inline void tri_unrank_pair(int p, int n, int& k1, int& k2) {
    k1 = 0;
    while (p >= n - 1 - k1) {
        p -= n - 1 - k1;
        ++k1;
    }
    k2 = k1 + 1 + p;
}

// the hypothesis of measurements (k1, k2): false when it is skipped
TRI_HD bool tri_pair_point(const double* __restrict__ cams, int num_images, const int* __restrict__ image, const float* __restrict__ uv, int k1,
                               int k2, double* x) {
    TriPairSrc src;
    if (!tri_load_cam(cams, num_images, image[k1], src.cam[0]) || !tri_load_cam(cams, num_images, image[k2], src.cam[1])) return false;
    src.uv[0][0] = (double)uv[2 * k1];
    src.uv[0][1] = (double)uv[2 * k1 + 1];
    src.uv[1][0] = (double)uv[2 * k2];
    src.uv[1][1] = (double)uv[2 * k2 + 1];
    return tri_triangulate(src, x);
}

TRI_HD inline double tri_measurement_error(const double* __restrict__ cams, int num_images, int image, const float* __restrict__ uv,
                                                        const double* x) {
    TriCam c;
    if (!tri_load_cam(cams, num_images, image, c)) return NAN;
    return tri_error(c, x, (double)uv[0], (double)uv[1]);
}

// |wRc1^T (wtc2 - wtc1)|; 0 with a camera missing
TRI_HD inline double tri_baseline(const double* __restrict__ cams, int num_images, int i1, int i2) {
    if (i1 < 0 || i1 >= num_images || i2 < 0 || i2 >= num_images) return 0.0;
    const double *a = cams + (long long)i1 * 17, *b = cams + (long long)i2 * 17;
    if (a[0] == 0.0 || b[0] == 0.0) return 0.0;
    const double d0 = b[14] - a[14], d1 = b[15] - a[15], d2 = b[16] - a[16];
    const double x = a[5] * d0 + a[8] * d1 + a[11] * d2;
    const double y = a[6] * d0 + a[9] * d1 + a[12] * d2;
    const double z = a[7] * d0 + a[10] * d1 + a[13] * d2;
    return sqrt(x * x + y * y + z * z);
}

// the sampling key of pair p = (k1, k2): the smallest keys are taken
TRI_HD inline double tri_pair_key(int mode, unsigned long long seed, unsigned long long tkey, int p, const double* __restrict__ cams,
                                               int num_images, int i1, int i2) {
    if (mode == TRI_UNIFORM) return (double)(tri_splitmix64(seed ^ tri_splitmix64(tkey ^ (unsigned long long)p)) >> 11);
    const double w = tri_baseline(cams, num_images, i1, i2);
    if (mode == TRI_TOPK) return -w;
    const double u = ((double)(tri_splitmix64(seed ^ tri_splitmix64(tkey ^ (unsigned long long)p)) >> 11) + 0.5) * 0x1.0p-53;
    return w > 0.0 ? -log(u) / w : INFINITY;
}

TRI_HD void tri_count_track(long long t, const long long* __restrict__ track_off, long long num_tracks, long long total, int mode, long long num_hyp,
                            long long* __restrict__ hyp_off, int* flags) {
    if (t >= num_tracks) return;
    const long long a = track_off[t], b = track_off[t + 1];
    long long n = b - a;
    if (a < 0 || b > total || n < 0 || n > TRI_MAX_TRACK_LENGTH) {
        flags[0] = 1;
        n = 0;
    }
    const long long pairs = n * (n - 1) / 2;
    hyp_off[t] = mode == TRI_NO_RANSAC ? 0 : (pairs < num_hyp ? pairs : num_hyp);
}

// one workgroup: val[0 .. n) -> its exclusive scan in place, val[n] = the total
__global__ __launch_bounds__(TRI_THREADS) void tri_scan_kernel(long long* val, long long n, long long cap, int* flags) {
    __shared__ long long lds[TRI_THREADS];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (long long base = 0; base < n; base += TRI_THREADS) {  // uniform bounds: the barriers stay matched
        const long long i = base + tid;
        const long long x = i < n ? val[i] : 0;
        lds[tid] = x;
        __syncthreads();
        for (int off = 1; off < TRI_THREADS; off <<= 1) {
            const long long add = tid >= off ? lds[tid - off] : 0;
            __syncthreads();
            lds[tid] += add;
            __syncthreads();
        }
        if (i < n) val[i] = carry + lds[tid] - x;
        carry += lds[TRI_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) {
        val[n] = carry;
        if (carry > cap) flags[1] = 1;
    }
}
// its stand-in on a CPU
void tri_scan_host(const HostRunner& run, long long* val, long long n, long long cap, int* flags) {
    run.scan(val, n);
    if (val[n] > cap) flags[1] = 1;
}

TRI_HD inline unsigned long long tri_float_bits(float f) {
    unsigned int b;
    __builtin_memcpy(&b, &f, sizeof(b));
    return (unsigned long long)b;
}

TRI_HD inline unsigned long long tri_track_key(int image0, const float* uv0) {
    const unsigned long long k = tri_splitmix64(((unsigned long long)(unsigned int)image0 << 32) ^ tri_float_bits(uv0[0]));
    return tri_splitmix64(k ^ tri_float_bits(uv0[1]));
}

// pairs first, first + stride, ... of track t; only a track with more pairs than hypotheses has work
TRI_HD void tri_select_track(long long t, int first_pair, int stride, const long long* __restrict__ track_off, const int* __restrict__ track_image,
                                                                 const float* __restrict__ track_uv, const double* __restrict__ cams, int num_images,
                                                                 int mode, long long num_hyp, unsigned long long seed,
                                                                 const long long* __restrict__ hyp_off, int* __restrict__ sel, long long cap,
                                                                 const int* __restrict__ flags) {
    if (flags[0]) return;
    const long long a = track_off[t];
    const int n = (int)(track_off[t + 1] - a);
    if (n < 2 || n > TRI_MAX_TRACK_LENGTH) return;
    const int pairs = (int)((long long)n * (n - 1) / 2);
    if ((long long)pairs <= num_hyp) return;
    const int* image = track_image + a;
    const unsigned long long tkey = tri_track_key(image[0], track_uv + 2 * a);
    const long long first = hyp_off[t];
    for (int p = first_pair; p < pairs; p += stride) {
        int k1, k2;
        tri_unrank_pair(p, n, k1, k2);
        const double mine = tri_pair_key(mode, seed, tkey, p, cams, num_images, image[k1], image[k2]);
        long long rank = 0;
        int q = 0;
        for (int j1 = 0; j1 < n - 1; ++j1)
            for (int j2 = j1 + 1; j2 < n; ++j2, ++q) {
                const double other = tri_pair_key(mode, seed, tkey, q, cams, num_images, image[j1], image[j2]);
                const bool tie_first = mode == TRI_TOPK ? q > p : q < p;
                rank += (other < mine || (other == mine && tie_first)) ? 1 : 0;
            }
        if (rank < num_hyp && first + rank < cap) sel[first + rank] = p;
    }
}

// hypotheses first, first + stride, ... of the whole batch
TRI_HD void tri_hypothesis_lane(long long first_hyp, long long stride, const long long* __restrict__ track_off, const int* __restrict__ track_image,
                                                                     const float* __restrict__ track_uv, long long num_tracks,
                                                                     const double* __restrict__ cams, int num_images, double threshold,
                                                                     long long num_hyp, const long long* __restrict__ hyp_off,
                                                                     const int* __restrict__ sel, TriHyp* __restrict__ hyp, long long cap,
                                                                     const int* __restrict__ flags) {
    if (flags[0]) return;
    long long total = hyp_off[num_tracks];
    if (total > cap) total = cap;
    for (long long g = first_hyp; g < total; g += stride) {
        long long lo = 0, hi = num_tracks;  // the largest t with hyp_off[t] <= g
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (hyp_off[mid] <= g) lo = mid; else hi = mid;
        }
        const long long t = lo, a = track_off[t];
        const int n = (int)(track_off[t + 1] - a);
        const long long pairs = (long long)n * (n - 1) / 2;
        const int p = pairs > num_hyp ? sel[g] : (int)(g - hyp_off[t]);
        TriHyp out;
        out.votes = -1;
        out.pair = p;
        out.mean = 0.0;
        if (p >= 0 && (long long)p < pairs) {  // always true for offsets that passed the count kernel
            const int* image = track_image + a;
            const float* uv = track_uv + 2 * a;
            int k1, k2;
            tri_unrank_pair(p, n, k1, k2);
            double x[3];
            if (tri_pair_point(cams, num_images, image, uv, k1, k2, x)) {
                int votes = 0;
                double sum = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double err = tri_measurement_error(cams, num_images, image[k], uv + 2 * k, x);
                    if (err < threshold) {
                        ++votes;
                        sum += err;
                    }
                }
                out.votes = votes;
                out.mean = votes > 0 ? sum / (double)votes : 0.0;
            }
        }
        hyp[g] = out;
    }
}

TRI_HD void tri_final_track(long long t, const long long* __restrict__ track_off, const int* __restrict__ track_image,
                                                                const float* __restrict__ track_uv, long long num_tracks,
                                                                const double* __restrict__ cams, int num_images, int mode, double threshold,
                                                                double min_angle_deg, const long long* __restrict__ hyp_off,
                                                                const TriHyp* __restrict__ hyp, long long cap, const int* __restrict__ flags,
                                                                double* __restrict__ point, double* __restrict__ avg_error, int* __restrict__ exit_code,
                                                                uint8_t* inlier_mask, int* __restrict__ stats) {
    if (t >= num_tracks || flags[0] || flags[1]) return;
    const long long a = track_off[t];
    const int n = (int)(track_off[t + 1] - a);
    const int* image = track_image + a;
    const float* uv = track_uv + 2 * a;
    uint8_t* mask = inlier_mask + a;
    int evaluated = 0, skipped = 0, best_pair = -1, best_votes = 0;
    double best_err = TRI_MAX_ERROR;
    if (mode != TRI_NO_RANSAC) {
        const long long first = hyp_off[t], last = hyp_off[t + 1] < cap ? hyp_off[t + 1] : cap;
        for (long long g = first; g < last; ++g) {
            const TriHyp h = hyp[g];
            ++evaluated;
            if (h.votes < 0) {
                ++skipped;
                continue;
            }
            if (h.votes == 0) continue;
            // the reference's update rule, made independent of the order of evaluation: exact ties go to the lowest pair index
            // written as three selects under one condition: a branchy form of this update was compiled for gfx950 so that a win by mean
            // error kept the old pair index (seen in the assembly and on the device; the host build was right)
            bool better;
            if (h.votes != best_votes) better = h.votes > best_votes;
            else if (h.mean != best_err) better = h.mean < best_err;
            else better = best_pair >= 0 && h.pair < best_pair;
            best_votes = better ? h.votes : best_votes;
            best_err = better ? h.mean : best_err;
            best_pair = better ? h.pair : best_pair;
        }
    }
    stats[4 * t] = evaluated;
    stats[4 * t + 1] = skipped;
    stats[4 * t + 2] = best_pair;
    stats[4 * t + 3] = best_votes;

    double x[3];
    int inliers = 0, used = 0;
    if (mode == TRI_NO_RANSAC) {
        for (int k = 0; k < n; ++k) mask[k] = 1;
    } else {
        bool have = false;
        if (best_pair >= 0) {
            int k1, k2;
            tri_unrank_pair(best_pair, n, k1, k2);
            have = tri_pair_point(cams, num_images, image, uv, k1, k2, x);  // the same code as the hypothesis lane: the same bits
        }
        for (int k = 0; k < n; ++k) mask[k] = have && tri_measurement_error(cams, num_images, image[k], uv + 2 * k, x) < threshold ? 1 : 0;
    }
    for (int k = 0; k < n; ++k)
        if (mask[k]) {
            ++inliers;
            used += image[k] >= 0 && image[k] < num_images && cams[(long long)image[k] * 17] != 0.0 ? 1 : 0;
        }
    int code = TRI_SUCCESS;
    double avg = NAN;
    bool ok = false;
    if (inliers < 2) {
        code = TRI_INLIERS;
    } else if (used < 2) {
        code = TRI_POSES;
    } else {
        TriTrackSrc src;
        src.cams = cams;
        src.num_images = num_images;
        src.image = image;
        src.uv = uv;
        src.mask = mask;
        src.n = n;
        if (!tri_triangulate(src, x)) {
            code = TRI_CHEIRALITY;
        } else {
            double sum = 0.0;
            int finite = 0;
            bool all_below = true;
            for (int k = 0; k < n; ++k) {
                if (!mask[k]) continue;
                const double err = tri_measurement_error(cams, num_images, image[k], uv + 2 * k, x);
                all_below = all_below && err < threshold;
                if (err == err) {
                    sum += err;
                    ++finite;
                }
            }
            avg = finite > 0 ? sum / (double)finite : NAN;
            if (!all_below) {
                code = TRI_EXCEEDS;
            } else {
                ok = true;
                if (min_angle_deg > 0.0) {  // every inlier has a camera here: a missing one made its error NaN
                    double best = -INFINITY;
                    for (int k1 = 0; k1 < n - 1; ++k1) {
                        if (!mask[k1]) continue;
                        const double* c1 = cams + (long long)image[k1] * 17 + 14;
                        const double a0 = x[0] - c1[0], a1 = x[1] - c1[1], a2 = x[2] - c1[2];
                        const double na = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
                        for (int k2 = k1 + 1; k2 < n; ++k2) {
                            if (!mask[k2]) continue;
                            const double* c2 = cams + (long long)image[k2] * 17 + 14;
                            const double b0 = x[0] - c2[0], b1 = x[1] - c2[1], b2 = x[2] - c2[2];
                            const double nb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
                            double dot = (a0 / na) * (b0 / nb) + (a1 / na) * (b1 / nb) + (a2 / na) * (b2 / nb);
                            dot = dot > 1.0 ? 1.0 : (dot < -1.0 ? -1.0 : dot);
                            const double angle = acos(dot) * (180.0 / M_PI);
                            best = angle > best ? angle : best;
                        }
                    }
                    if (best < min_angle_deg) {
                        code = TRI_LOW_ANGLE;
                        ok = false;
                    }
                }
            }
        }
    }
    point[3 * t] = ok ? x[0] : NAN;
    point[3 * t + 1] = ok ? x[1] : NAN;
    point[3 * t + 2] = ok ? x[2] : NAN;
    avg_error[t] = avg;
    exit_code[t] = code;
}

// ---- the pipeline: every stage once, for the device call and for tools/triangulation_host_main.cpp (stage_runner.h) ----

struct TriCall {  // the checked arguments; max_hyp is 0 without RANSAC
    const long long* track_off;
    const int* image;
    const float* uv;
    long long num_tracks, total;
    const double* cams;
    int num_images, mode;
    double threshold, min_angle_deg;
    long long max_hyp;
    unsigned long long seed;
    double *point, *avg_error;
    int* exit_code;
    uint8_t* inlier_mask;
    int* stats;
};

// at least one track; w is laid out for c.num_tracks, c.total and c.max_hyp
template <class Runner>
int tri_triangulate_stages(Runner& run, const char* me, const TriCall& c, const TriWorkspace& w) {
    run.zero(w.flags, 16);
    run.template each<struct tri_count_stage>(c.num_tracks, STAGE_FN(long long t) { tri_count_track(t, c.track_off, c.num_tracks, c.total, c.mode, c.max_hyp, w.hyp_off, w.flags); });
    run.block(
        "tri_scan_kernel", [&](hipStream_t stream) { hipLaunchKernelGGL(tri_scan_kernel, dim3(1), dim3(TRI_THREADS), 0, stream, w.hyp_off, c.num_tracks, w.cap, w.flags); },
        [&](const HostRunner& host) { tri_scan_host(host, w.hyp_off, c.num_tracks, w.cap, w.flags); });
    if (c.mode != TRI_NO_RANSAC) {
        run.template group<struct tri_select_stage, TRI_THREADS, TRI_THREADS>(c.num_tracks, STAGE_FN(long long t, int lane, int lanes) {
            tri_select_track(t, lane, lanes, c.track_off, c.image, c.uv, c.cams, c.num_images, c.mode, c.max_hyp, c.seed, w.hyp_off, w.sel, w.cap, w.flags);
        });
        const long long want = (w.cap + TRI_THREADS - 1) / TRI_THREADS, groups = want < TRI_HYP_BLOCKS ? want : TRI_HYP_BLOCKS;
        run.template group<struct tri_hypothesis_stage, TRI_THREADS, TRI_THREADS>(groups, STAGE_FN(long long group, int lane, int lanes) {
            tri_hypothesis_lane(group * lanes + lane, groups * lanes, c.track_off, c.image, c.uv, c.num_tracks, c.cams, c.num_images, c.threshold, c.max_hyp, w.hyp_off, w.sel,
                                w.hyp, w.cap, w.flags);
        });
    }
    run.template each<struct tri_final_stage, TRI_FINAL_THREADS, TRI_THREADS>(c.num_tracks, STAGE_FN(long long t) {
        tri_final_track(t, c.track_off, c.image, c.uv, c.num_tracks, c.cams, c.num_images, c.mode, c.threshold, c.min_angle_deg, w.hyp_off, w.hyp, w.cap, w.flags, c.point,
                        c.avg_error, c.exit_code, c.inlier_mask, c.stats);
    });
    int flag[2] = {0, 0};
    if (run.fetch(flag, w.flags, 2, "reading the flags") != GTSFM_OK) return run.status;
    GTSFM_CHECK_ARG(!flag[0], "%s: track_off_dev is not ascending within 0 .. %lld, or a track is longer than %d; nothing was written", me, c.total, TRI_MAX_TRACK_LENGTH);
    GTSFM_CHECK_ARG(!flag[1], "%s: the tracks hold more than %lld measurements; nothing was written", me, c.total);
    return run.status;
}

}  // namespace

extern "C" size_t gtsfm_triangulate_workspace_bytes(long long num_tracks, long long total_measurements, long long max_hypotheses) {
    if (num_tracks < 0 || total_measurements < 0 || max_hypotheses < 0 || num_tracks >= (1ll << 31) || total_measurements >= (1ll << 40)) return 0;
    const TriWorkspace w = tri_layout(nullptr, num_tracks, total_measurements, max_hypotheses);
    return w.cap < 0 ? 0 : w.bytes;
}

extern "C" int gtsfm_triangulate_tracks_f64(const long long* track_off_dev, const int32_t* track_image_dev, const float* track_uv_dev, long long num_tracks,
                                            long long total_measurements, const double* cameras_dev, int num_images, int mode,
                                            double reproj_error_threshold, double min_triangulation_angle_deg, long long num_hypotheses,
                                            unsigned long long seed, void* workspace_dev, size_t workspace_bytes, double* point_dev,
                                            double* avg_error_dev, int32_t* exit_code_dev, uint8_t* inlier_mask_dev, int32_t* stats_dev, void* stream_) {
    const char* me = "gtsfm_triangulate_tracks_f64";
    GTSFM_CHECK_ARG(num_tracks >= 0 && total_measurements >= 0 && num_images >= 0 && num_tracks < (1ll << 31) && total_measurements < (1ll << 40),
                    "%s: size out of range (%lld tracks, %lld measurements, %d images)", me, num_tracks, total_measurements, num_images);
    GTSFM_CHECK_ARG(mode >= TRI_NO_RANSAC && mode <= TRI_TOPK, "%s: mode %d outside 0 .. 3", me, mode);
    GTSFM_CHECK_ARG(reproj_error_threshold > 0.0, "%s: reproj_error_threshold %g must be positive (infinity allowed)", me, reproj_error_threshold);
    GTSFM_CHECK_ARG(min_triangulation_angle_deg == min_triangulation_angle_deg, "%s: min_triangulation_angle_deg is NaN", me);
    GTSFM_CHECK_ARG(mode == TRI_NO_RANSAC || num_hypotheses >= 0, "%s: %lld hypotheses", me, num_hypotheses);
    if (num_tracks == 0) return GTSFM_OK;
    GTSFM_CHECK_ARG(track_off_dev && point_dev && avg_error_dev && exit_code_dev && stats_dev && workspace_dev, "%s: null pointer", me);
    GTSFM_CHECK_ARG(total_measurements == 0 || (track_image_dev && track_uv_dev && inlier_mask_dev), "%s: null measurement pointer", me);
    GTSFM_CHECK_ARG(num_images == 0 || cameras_dev, "%s: null camera table", me);
    const long long max_hyp = mode == TRI_NO_RANSAC ? 0 : num_hypotheses;
    const TriWorkspace w = tri_layout(workspace_dev, num_tracks, total_measurements, max_hyp);
    // a hypothesis capacity beyond 4e18 (w.cap < 0) fits no workspace
    const int fits = gtsfm_check_workspace(me, workspace_dev, w.cap >= 0 && workspace_bytes >= w.bytes, workspace_bytes, w.bytes, "%lld tracks / %lld measurements / %lld hypotheses", num_tracks,
                                           total_measurements, max_hyp);
    if (fits != GTSFM_OK) return fits;
    const TriCall c{track_off_dev, track_image_dev, track_uv_dev, num_tracks, total_measurements, cameras_dev, num_images, mode, reproj_error_threshold,
                    min_triangulation_angle_deg, max_hyp, seed, point_dev, avg_error_dev, exit_code_dev, inlier_mask_dev, stats_dev};
    DeviceRunner run{(hipStream_t)stream_, me};
    return tri_triangulate_stages(run, me, c, w);
}
