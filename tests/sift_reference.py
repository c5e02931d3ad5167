"""A numpy float32 restatement of OpenCV's ``SIFT_create().detectAndCompute`` with its defaults (nOctaveLayers 3, contrastThreshold
0.04, edgeThreshold 10, sigma 1.6, first octave -1) followed by the top-k of the reference's ``SIFTDetectorDescriptor``, in explicit
operation order. ``gtsfm_amd/csrc/sift_kernels.hip`` follows this file operation for operation, so the two agree bit for bit:

* every product and sum is a separate float32 rounding (no fused multiply-add), evaluated left to right as written;
* a blur sums from the centre tap outwards: ``acc = k0 c``, then ``acc = acc + k_j (left_j + right_j)`` for j = 1 .. r;
* the 3 x 3 systems are solved by elimination with partial pivoting, in the order of ``solve3``;
* ``exp``, ``exp2``, ``sin`` and ``cos`` are the explicit polynomials below, the arc tangent is OpenCV's ``fastAtan2`` polynomial;
  square roots and divisions are IEEE (correctly rounded);
* histograms are summed in window order (row by row), one sample after the other.

Not a copy of OpenCV: written from the algorithm's description ("SIFT")."""

from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np

F = np.float32
SIGMA = 1.6
LAYERS = 3
BORDER = 5
MAX_OCTAVES = 16
FLT_EPSILON = F(1.1920929e-07)


# ----------------------------------------------------------------------------------------------------------------------
# explicit mathematics
# ----------------------------------------------------------------------------------------------------------------------
def exp2_f32(t: np.ndarray) -> np.ndarray:
    t = np.asarray(t, dtype=F)
    n = np.rint(t)
    g = (t - n) * F(0.6931471805599453)
    p = np.full_like(g, F(1.0 / 5040.0))
    for c in (1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
        p = p * g + F(c)
    return np.ldexp(p, n.astype(np.int32)).astype(F)


def exp_f32(x: np.ndarray) -> np.ndarray:
    return exp2_f32(np.asarray(x, dtype=F) * F(1.4426950408889634))


def atan2_deg(y: np.ndarray, x: np.ndarray) -> np.ndarray:
    """OpenCV's ``fastAtan2``: degrees in [0, 360)."""
    scale = F(180.0 / math.pi)
    p1, p3, p5, p7 = (F(c) * scale for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    ax, ay = np.abs(x), np.abs(y)
    a = np.minimum(ax, ay) / (np.maximum(ax, ay) + F(2.220446049250313e-16))
    a2 = a * a
    p = (((p7 * a2 + p5) * a2 + p3) * a2 + p1) * a
    p = np.where(ay > ax, F(90.0) - p, p)
    p = np.where(x < 0, F(180.0) - p, p)
    p = np.where(y < 0, F(360.0) - p, p)
    return p.astype(F)


def sincos_deg(a):
    """(cos, sin) of an angle in degrees: quadrant reduction, then Taylor polynomials on [-45, 45] degrees."""
    a = F(a)
    q = np.rint(a / F(90.0))
    t = (a - F(90.0) * q) * F(math.pi / 180.0)
    t2 = t * t
    s = F(1.0 / 362880.0)
    for c in (-1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0):
        s = s * t2 + F(c)
    s = s * t2 * t + t
    c_ = F(-1.0 / 3628800.0)
    for c in (1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5, 1.0):
        c_ = c_ * t2 + F(c)
    qi = int(q) & 3
    return ((c_, s), (-s, c_), (-c_, -s), (s, -c_))[qi]


def round_half_even(v: float) -> int:
    return int(round(v))  # Python rounds halves to even, as cvRound does


# ----------------------------------------------------------------------------------------------------------------------
# pyramid
# ----------------------------------------------------------------------------------------------------------------------
def num_octaves(height: int, width: int) -> int:
    n = round_half_even(math.log2(min(2 * height, 2 * width))) - 2
    return max(0, min(n, MAX_OCTAVES))


def octave_shapes(height: int, width: int) -> List[tuple]:
    return [((2 * height) >> o, (2 * width) >> o) for o in range(num_octaves(height, width))]


def layer_sigma(i: int) -> float:
    """i = 0: the blur of the doubled image; i = 1 .. 5: the increment from Gaussian image i - 1 to image i."""
    if i == 0:
        return math.sqrt(max(SIGMA * SIGMA - 1.0 * 1.0, 0.01))
    k = math.pow(2.0, 1.0 / 3.0)
    prev = math.pow(k, float(i - 1)) * SIGMA
    total = prev * k
    return math.sqrt(total * total - prev * prev)


def gaussian_taps(sigma: float) -> np.ndarray:
    """``round(8 sigma + 1) | 1`` taps exp(-x^2 / 2 sigma^2) / sum, float64 (the sum left to right), rounded to float32."""
    n = round_half_even(8.0 * sigma + 1.0) | 1
    r = n // 2
    w = [math.exp(-(float(i - r) * float(i - r)) / (2.0 * sigma * sigma)) for i in range(n)]
    total = 0.0
    for v in w:
        total += v
    return np.array([v / total for v in w], dtype=np.float64).astype(F)


def reflect101(idx: np.ndarray, n: int) -> np.ndarray:
    """BORDER_REFLECT_101, reflected as often as it takes."""
    if n == 1:
        return np.zeros_like(idx)
    idx = idx.copy()
    while True:
        bad = (idx < 0) | (idx >= n)
        if not bad.any():
            return idx
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= n, 2 * n - 2 - idx, idx)


def _blur_axis1(img: np.ndarray, taps: np.ndarray) -> np.ndarray:
    r = len(taps) // 2
    w = img.shape[1]
    p = img[:, reflect101(np.arange(-r, w + r), w)]
    acc = taps[r] * p[:, r : r + w]
    for j in range(1, r + 1):
        acc = acc + taps[r + j] * (p[:, r - j : r - j + w] + p[:, r + j : r + j + w])
    return acc


def gaussian_blur(img: np.ndarray, sigma: float) -> np.ndarray:
    taps = gaussian_taps(sigma)
    rows = _blur_axis1(np.ascontiguousarray(img, dtype=F), taps)
    return np.ascontiguousarray(_blur_axis1(np.ascontiguousarray(rows.T), taps).T)


def upsample2(gray: np.ndarray) -> np.ndarray:
    """2 x bilinear, half-pixel centres, clamped edges (``F.interpolate(scale_factor=2, mode="bilinear", align_corners=False)``)."""

    def axis0(a):
        n = a.shape[0]
        k = np.arange(n)
        lo, hi = a[np.maximum(k - 1, 0)], a[np.minimum(k + 1, n - 1)]
        out = np.empty((2 * n,) + a.shape[1:], dtype=F)
        out[0::2] = F(0.25) * lo + F(0.75) * a
        out[1::2] = F(0.75) * a + F(0.25) * hi
        return out

    a = np.asarray(gray).astype(F)
    return np.ascontiguousarray(axis0(axis0(a.T).T))


def build_pyramid(gray: np.ndarray):
    """(gaussians, dogs): per octave a (6, H, W) and a (5, H, W) float32 array."""
    h, w = gray.shape
    n = num_octaves(h, w)
    gaussians, dogs = [], []
    if n == 0:
        return gaussians, dogs
    base = gaussian_blur(upsample2(gray), layer_sigma(0))
    for o in range(n):
        g = [base]
        for i in range(1, LAYERS + 3):
            g.append(gaussian_blur(g[-1], layer_sigma(i)))
        g = np.stack(g)
        gaussians.append(g)
        dogs.append(g[1:] - g[:-1])
        hh, ww = g.shape[1] // 2, g.shape[2] // 2
        base = np.ascontiguousarray(g[LAYERS][: 2 * hh : 2, : 2 * ww : 2])
    return gaussians, dogs


def flatten_pyramid(gaussians, dogs) -> np.ndarray:
    """The device layout: every octave's Gaussian images, then every octave's DoG images."""
    parts = [g.ravel() for g in gaussians] + [d.ravel() for d in dogs]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=F)


# ----------------------------------------------------------------------------------------------------------------------
# detection
# ----------------------------------------------------------------------------------------------------------------------
def find_candidates(dogs) -> np.ndarray:
    """(n, 4) int32 (octave, layer, row, column), sorted."""
    out = []
    for o, d in enumerate(dogs):
        _, h, w = d.shape
        if h <= 2 * BORDER or w <= 2 * BORDER:
            continue
        for layer in range(1, LAYERS + 1):
            v = d[layer, BORDER : h - BORDER, BORDER : w - BORDER]
            is_max, is_min = v > 0, v < 0
            for dl in (-1, 0, 1):
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        nb = d[layer + dl, BORDER + dr : h - BORDER + dr, BORDER + dc : w - BORDER + dc]
                        is_max &= v >= nb
                        is_min &= v <= nb
            hit = (np.abs(v) > F(1.0)) & (is_max | is_min)
            rc = np.argwhere(hit)
            out.append(np.column_stack([np.full(len(rc), o), np.full(len(rc), layer), rc[:, 0] + BORDER, rc[:, 1] + BORDER]))
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 4), dtype=np.int32)


def solve3(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """X with A X = b for m systems (a: (m, 3, 3), b: (m, 3)), elimination with partial pivoting; a singular system gives X = 0."""
    a, b = a.astype(F).copy(), b.astype(F).copy()
    m = len(a)
    ar = np.arange(m)
    singular = np.zeros(m, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(3):
            k = np.full(m, i)
            for j in range(i + 1, 3):
                k = np.where(np.abs(a[:, j, i]) > np.abs(a[ar, k, i]), j, k)
            singular |= ~singular & (np.abs(a[ar, k, i]) < FLT_EPSILON * F(10.0))
            row_i, row_k = a[ar, i].copy(), a[ar, k].copy()
            a[ar, k] = row_i
            a[ar, i] = row_k
            b_i, b_k = b[ar, i].copy(), b[ar, k].copy()
            b[ar, k] = b_i
            b[ar, i] = b_k
            d = F(-1.0) / a[:, i, i]
            for j in range(i + 1, 3):
                alpha = a[:, j, i] * d
                for q in range(i + 1, 3):
                    a[:, j, q] = a[:, j, q] + alpha * a[:, i, q]
                b[:, j] = b[:, j] + alpha * b[:, i]
        for i in (2, 1, 0):
            s = b[:, i]
            for q in range(i + 1, 3):
                s = s - a[:, i, q] * b[:, q]
            b[:, i] = s / a[:, i, i]
    b[singular] = 0
    return b


def _derivatives(d: np.ndarray, l: np.ndarray, r: np.ndarray, c: np.ndarray):
    img_scale = F(1.0) / F(255.0)
    deriv, second, cross = img_scale * F(0.5), img_scale, img_scale * F(0.25)
    v = d[l, r, c]
    dx = (d[l, r, c + 1] - d[l, r, c - 1]) * deriv
    dy = (d[l, r + 1, c] - d[l, r - 1, c]) * deriv
    ds = (d[l + 1, r, c] - d[l - 1, r, c]) * deriv
    v2 = v * F(2.0)
    dxx = (d[l, r, c + 1] + d[l, r, c - 1] - v2) * second
    dyy = (d[l, r + 1, c] + d[l, r - 1, c] - v2) * second
    dss = (d[l + 1, r, c] + d[l - 1, r, c] - v2) * second
    dxy = (d[l, r + 1, c + 1] - d[l, r + 1, c - 1] - d[l, r - 1, c + 1] + d[l, r - 1, c - 1]) * cross
    dxs = (d[l + 1, r, c + 1] - d[l + 1, r, c - 1] - d[l - 1, r, c + 1] + d[l - 1, r, c - 1]) * cross
    dys = (d[l + 1, r + 1, c] - d[l + 1, r - 1, c] - d[l - 1, r + 1, c] + d[l - 1, r - 1, c]) * cross
    grad = np.stack([dx, dy, ds], axis=1)
    hess = np.stack([np.stack([dxx, dxy, dxs], 1), np.stack([dxy, dyy, dys], 1), np.stack([dxs, dys, dss], 1)], axis=1)
    return v, grad, hess


def refine(dogs, candidates: np.ndarray) -> Dict[str, np.ndarray]:
    """Refined keypoints sorted by (octave, layer, row, column), one per final position. Fields: octave, layer, row, column (int32);
    x = column + X0, y = row + X1 (octave coordinates), scl = 1.6 * 2^((layer + X2) / 3), response (float32)."""
    recs = {k: [] for k in ("octave", "layer", "row", "column", "x", "y", "scl", "response")}
    limit = F(2147483647 // 3)
    img_scale = F(1.0) / F(255.0)
    for o, d in enumerate(dogs):
        sel = candidates[candidates[:, 0] == o]
        if len(sel) == 0:
            continue
        _, h, w = d.shape
        l, r, c = (sel[:, i].astype(np.int64) for i in (1, 2, 3))
        m = len(sel)
        active = np.ones(m, dtype=bool)
        converged = np.zeros(m, dtype=bool)
        X = np.zeros((m, 3), dtype=F)
        V = np.zeros(m, dtype=F)
        G = np.zeros((m, 3), dtype=F)
        Hm = np.zeros((m, 3, 3), dtype=F)
        for _ in range(5):
            idx = np.flatnonzero(active & ~converged)
            if len(idx) == 0:
                break
            v, grad, hess = _derivatives(d, l[idx], r[idx], c[idx])
            x = -solve3(hess, grad)  # X0 (column), X1 (row), X2 (layer)
            X[idx], V[idx], G[idx], Hm[idx] = x, v, grad, hess
            conv = (np.abs(x) < F(0.5)).all(axis=1)
            converged[idx[conv]] = True
            mv = idx[~conv]
            xm = x[~conv]
            ok = (np.abs(xm) <= limit).all(axis=1)
            active[mv[~ok]] = False
            mv, xm = mv[ok], xm[ok]
            c[mv] += np.rint(xm[:, 0]).astype(np.int64)
            r[mv] += np.rint(xm[:, 1]).astype(np.int64)
            l[mv] += np.rint(xm[:, 2]).astype(np.int64)
            inside = (l[mv] >= 1) & (l[mv] <= LAYERS) & (c[mv] >= BORDER) & (c[mv] < w - BORDER) & (r[mv] >= BORDER) & (r[mv] < h - BORDER)
            active[mv[~inside]] = False
        keep = active & converged
        t = (G[:, 0] * X[:, 0] + G[:, 1] * X[:, 1]) + G[:, 2] * X[:, 2]
        contr = V * img_scale + t * F(0.5)
        keep &= ~((np.abs(contr) * F(3.0)).astype(np.float64) < 0.04)
        dxx, dyy, dxy = Hm[:, 0, 0], Hm[:, 1, 1], Hm[:, 0, 1]
        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
        keep &= ~((det <= 0) | ((tr * tr).astype(np.float64) * 10.0 >= 121.0 * det.astype(np.float64)))
        k = np.flatnonzero(keep)
        key = (l[k] * h + r[k]) * w + c[k]
        _, first = np.unique(key, return_index=True)  # sorted by key; equal positions carry equal records
        k = k[first]
        recs["octave"].append(np.full(len(k), o, dtype=np.int32))
        recs["layer"].append(l[k].astype(np.int32))
        recs["row"].append(r[k].astype(np.int32))
        recs["column"].append(c[k].astype(np.int32))
        recs["x"].append(c[k].astype(F) + X[k, 0])
        recs["y"].append(r[k].astype(F) + X[k, 1])
        recs["scl"].append(F(1.6) * exp2_f32((l[k].astype(F) + X[k, 2]) / F(3.0)))
        recs["response"].append(np.abs(contr[k]))
    int_fields = ("octave", "layer", "row", "column")
    return {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int32 if k in int_fields else F)) for k, v in recs.items()}


def orientation_histogram(img: np.ndarray, r: int, c: int, scl) -> np.ndarray:
    """The smoothed 36-bin histogram around (c, r) of one Gaussian image."""
    h, w = img.shape
    radius = int(np.rint(F(4.5) * scl))
    sigma = F(1.5) * scl
    expf_scale = F(-1.0) / (F(2.0) * sigma * sigma)
    rng = np.arange(-radius, radius + 1)
    i, j = (a.ravel() for a in np.meshgrid(rng, rng, indexing="ij"))
    y, x = r + i, c + j
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    i, j, y, x = i[ok], j[ok], y[ok], x[ok]
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    wgt = exp_f32((i * i + j * j).astype(F) * expf_scale)
    ang = atan2_deg(dy, dx)
    mag = np.sqrt(dx * dx + dy * dy)
    b = np.rint((F(36.0) / F(360.0)) * ang).astype(np.int64)
    b = np.where(b >= 36, b - 36, b)
    b = np.where(b < 0, b + 36, b)
    raw = np.zeros(36, dtype=F)
    np.add.at(raw, b, wgt * mag)  # unbuffered: one sample after the other
    return (np.roll(raw, 2) + np.roll(raw, -2)) * F(1.0 / 16.0) + (np.roll(raw, 1) + np.roll(raw, -1)) * F(4.0 / 16.0) + raw * F(6.0 / 16.0)


def histogram_peaks(hist: np.ndarray) -> List:
    """Angles (degrees) of the peaks of a smoothed histogram, by bin."""
    thr = hist.max() * F(0.8)
    out = []
    for j in range(36):
        hl, hr, hj = hist[(j + 35) % 36], hist[(j + 1) % 36], hist[j]
        if hj > hl and hj > hr and hj >= thr:
            b = F(j) + F(0.5) * (hl - hr) / (hl - F(2.0) * hj + hr)
            b = F(36.0) + b if b < 0 else (b - F(36.0) if b >= F(36.0) else b)
            angle = F(360.0) - (F(360.0) / F(36.0)) * b
            if abs(angle - F(360.0)) < FLT_EPSILON:
                angle = F(0.0)
            out.append(F(angle))
    return out


def final_xy(kp: Dict[str, np.ndarray]) -> np.ndarray:
    """(n, 2) final (x, y): octave coordinates * 2^octave * 0.5."""
    e = kp["octave"].astype(np.int32) - 1
    return np.stack([np.ldexp(kp["x"], e), np.ldexp(kp["y"], e)], axis=1).astype(F)


def orient(gaussians, kp: Dict[str, np.ndarray], mask: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """One record per histogram peak, after the mask, in the output order: response descending, then (octave, layer, row, column, angle)."""
    n = len(kp["octave"])
    keep = np.ones(n, dtype=bool)
    if mask is not None and n:
        xy = np.rint(final_xy(kp)).astype(np.int64)
        mx = np.clip(xy[:, 0], 0, mask.shape[1] - 1)
        my = np.clip(xy[:, 1], 0, mask.shape[0] - 1)
        keep = mask[my, mx] != 0
    src, angles = [], []
    for t in np.flatnonzero(keep):
        img = gaussians[kp["octave"][t]][kp["layer"][t]]
        for a in histogram_peaks(orientation_histogram(img, int(kp["row"][t]), int(kp["column"][t]), kp["scl"][t])):
            src.append(t)
            angles.append(a)
    src = np.array(src, dtype=np.int64)
    out = {k: v[src] for k, v in kp.items()}
    out["angle"] = np.array(angles, dtype=F)
    order = np.lexsort((out["angle"], out["column"], out["row"], out["layer"], out["octave"], -out["response"].astype(np.float64)))
    return {k: v[order] for k, v in out.items()}


def describe_one(img: np.ndarray, x, y, scl, angle) -> np.ndarray:
    """The 128 integers (as float32) of one oriented keypoint; (x, y) in octave coordinates."""
    h, w = img.shape
    ori = F(360.0) - F(angle)
    if abs(ori - F(360.0)) < FLT_EPSILON:
        ori = F(0.0)
    px, py = int(np.rint(F(x))), int(np.rint(F(y)))
    cos_t, sin_t = sincos_deg(ori)
    bins_per_deg = F(8.0) / F(360.0)
    exp_scale = F(-1.0) / (F(4.0) * F(4.0) * F(0.5))
    hist_width = F(3.0) * F(scl)
    radius = int(np.rint(hist_width * F(1.4142135623730951) * F(5.0) * F(0.5)))
    radius = min(radius, int(math.sqrt(float(w) * w + float(h) * h)))
    cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
    rng = np.arange(-radius, radius + 1)
    i, j = (a.ravel() for a in np.meshgrid(rng, rng, indexing="ij"))
    fi, fj = i.astype(F), j.astype(F)
    c_rot = fj * cos_t - fi * sin_t
    r_rot = fj * sin_t + fi * cos_t
    rbin = r_rot + F(2.0) - F(0.5)
    cbin = c_rot + F(2.0) - F(0.5)
    r, c = py + i, px + j
    ok = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (r > 0) & (r < h - 1) & (c > 0) & (c < w - 1)
    r, c, rbin, cbin, c_rot, r_rot = r[ok], c[ok], rbin[ok], cbin[ok], c_rot[ok], r_rot[ok]
    dx = img[r, c + 1] - img[r, c - 1]
    dy = img[r - 1, c] - img[r + 1, c]
    wgt = exp_f32((c_rot * c_rot + r_rot * r_rot) * exp_scale)
    obin = (atan2_deg(dy, dx) - ori) * bins_per_deg
    mag = np.sqrt(dx * dx + dy * dy) * wgt
    fr, fc, fo = np.floor(rbin), np.floor(cbin), np.floor(obin)
    r0, c0, o0 = fr.astype(np.int64), fc.astype(np.int64), fo.astype(np.int64)
    rbin, cbin, obin = rbin - fr, cbin - fc, obin - fo
    o0 = np.where(o0 < 0, o0 + 8, o0)
    o0 = np.where(o0 >= 8, o0 - 8, o0)
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin
    v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin
    v_rc00 = v_r0 - v_rc01
    vals, offs = [], []
    for vrc, off in ((v_rc00, 0), (v_rc01, 10), (v_rc10, 60), (v_rc11, 70)):
        v1 = vrc * obin
        vals += [vrc - v1, v1]
        offs += [off, off + 1]
    idx = ((r0 + 1) * 6 + c0 + 1) * 10 + o0
    hist = np.zeros(360, dtype=F)
    # unbuffered and sample by sample: every cell receives its contributions in window order
    np.add.at(hist, (idx[:, None] + np.array(offs)[None, :]).ravel(), np.stack(vals, axis=1).ravel())
    hist = hist.reshape(6, 6, 10)
    hist[:, :, 0] = hist[:, :, 0] + hist[:, :, 8]
    hist[:, :, 1] = hist[:, :, 1] + hist[:, :, 9]
    dst = np.ascontiguousarray(hist[1:5, 1:5, :8]).ravel()
    thr = np.sqrt(np.cumsum(dst * dst, dtype=F)[-1]) * F(0.2)  # cumsum: a left-to-right sum
    dst = np.minimum(dst, thr)
    scale = F(512.0) / np.maximum(np.sqrt(np.cumsum(dst * dst, dtype=F)[-1]), FLT_EPSILON)
    return np.clip(np.rint(dst * scale), F(0.0), F(255.0)).astype(F)


def describe(gaussians, ori: Dict[str, np.ndarray], count: int) -> np.ndarray:
    out = np.zeros((count, 128), dtype=F)
    for t in range(count):
        img = gaussians[ori["octave"][t]][ori["layer"][t]]
        out[t] = describe_one(img, ori["x"][t], ori["y"][t], ori["scl"][t], ori["angle"][t])
    return out


def final_outputs(ori: Dict[str, np.ndarray], count: int):
    """coordinates (count, 2), sizes (count,), responses (count,) of the first ``count`` oriented keypoints."""
    head = {k: v[:count] for k, v in ori.items()}
    return final_xy(head), np.ldexp(head["scl"], head["octave"].astype(np.int32)).astype(F), head["response"].astype(F)


def to_gray(image: np.ndarray) -> np.ndarray:
    """(H, W) passes; (H, W, 3 / 4) through the package's 15-bit formula (``gtsfm_amd.common.image.rgb_to_gray_u8``)."""
    image = np.asarray(image)
    if image.ndim == 2:
        return image
    if image.ndim != 3 or image.shape[2] not in (3, 4):
        raise ValueError("Input image dimensions are wrong")
    rgb = image[..., :3].astype(np.uint32)
    return ((rgb[..., 0] * 9798 + rgb[..., 1] * 19235 + rgb[..., 2] * 3735 + (1 << 14)) >> 15).astype(np.uint8)


def detect_and_describe(image: np.ndarray, max_keypoints: int = 5000, mask: Optional[np.ndarray] = None, stages: bool = False):
    """``(coordinates (N, 2), sizes (N,), responses (N,), descriptors (N, 128))``, all float32; with ``stages`` also a dict holding every
    stage's output (pyramid in the device layout, candidates, keypoints, oriented keypoints)."""
    gray = to_gray(image)
    gaussians, dogs = build_pyramid(gray)
    cand = find_candidates(dogs)
    kp = refine(dogs, cand)
    ori = orient(gaussians, kp, mask)
    count = min(len(ori["angle"]), max_keypoints)
    desc = describe(gaussians, ori, count)
    xy, sizes, responses = final_outputs(ori, count)
    if not stages:
        return xy, sizes, responses, desc
    return xy, sizes, responses, desc, {"pyramid": flatten_pyramid(gaussians, dogs), "candidates": cand, "keypoints": kp, "oriented": ori}
