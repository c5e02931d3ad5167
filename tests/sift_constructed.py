"""Constructed SIFT images and a census of the events they reach in the numpy restatement (``tests/sift_reference.py``).

Photographs leave whole branches of ``gtsfm_amd/csrc/sift_kernels.hip`` unexecuted: a descriptor radius clipped by the octave's diagonal,
a response tie between two different keypoints, a singular 3 x 3 solve, an octave twelve pixels wide. Every image here is generated from
code and a seed, is at most 64 x 64 (thin strips: at most 12 x 256) and is named after the event it exists for.

``census`` runs the restatement on an image and counts events. It never edits the restatement: ``atan2_deg`` and ``gaussian_blur`` are
wrapped while it runs (and restored), and the decisions inside ``refine``, ``solve3``, ``histogram_peaks`` and ``describe_one`` are
re-derived next to them by the ``trace_*`` functions, each of which asserts that what it re-derives is byte for byte what the restatement
returns. An event count is therefore a statement about the restatement's own run."""

from __future__ import annotations

import math
from collections import Counter
from typing import Dict, Optional

import numpy as np

import sift_reference as S

F = np.float32

EVENTS = (
    # pyramid
    "blur_radius_exceeds_extent", "odd_octave_is_decimated", "octave_too_small_beside_others",
    # extrema
    "adjacent_candidates_in_a_layer", "maxima_and_minima",
    # refinement
    "move_by_column", "move_by_row", "move_by_layer", "leaves_layer_range", "leaves_border", "offset_beyond_limit", "five_steps_without_convergence",
    "singular_solve", "row_exchange_at_pivot_0", "row_exchange_at_pivot_1", "rejected_by_contrast", "rejected_by_det", "rejected_by_edge_ratio",
    "two_candidates_one_position",
    # orientation
    "orientation_window_clipped", "atan2_equals_360", "peak_bin_below_0", "peak_bin_at_least_36", "angle_360_set_to_0", "two_peaks",
    "three_or_more_peaks", "dropped_by_mask",
    # order
    "equal_response_different_keypoints", "equal_response_across_layers_or_octaves",
    # descriptor
    "radius_clipped_by_diagonal", "descriptor_window_clipped", "descriptor_atan2_equals_360", "o0_below_0_wraps", "o0_at_least_8_wraps",
    "element_reaches_the_0.2_clip", "element_saturates_at_255", "fewer_than_64_samples",
    # shapes
    "keypoint_in_a_thin_strip", "keypoint_in_a_12_pixel_octave",
)


# ----------------------------------------------------------------------------------------------------------------------
# images
# ----------------------------------------------------------------------------------------------------------------------
def _to_u8(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    a = (a - a.min()) / max(a.max() - a.min(), 1e-12)
    return np.rint(a * 255.0).astype(np.uint8)


def _texture(seed: int, h: int, w: int, sigma: float) -> np.ndarray:
    """Seeded white noise, blurred: a smooth texture with blobs of about ``sigma`` pixels."""
    rng = np.random.default_rng(seed)
    return _to_u8(S.gaussian_blur(rng.standard_normal((h, w)).astype(F), sigma))


def blob_24x24() -> np.ndarray:
    """One Gaussian blob of sigma 5 px: its keypoint sits in the 12 x 12 octave and every descriptor radius is clipped by the diagonal."""
    y, x = np.mgrid[0:24, 0:24].astype(np.float64)
    return np.rint(255.0 * np.exp(-((y - 11.5) ** 2 + (x - 11.5) ** 2) / (2.0 * 5.0 * 5.0))).astype(np.uint8)


def mirror_48x48() -> np.ndarray:
    """A smooth texture and its left-right mirror image: mirrored keypoints carry bit-equal responses."""
    half = _texture(11, 48, 24, 2.0)
    return np.ascontiguousarray(np.concatenate([half, half[:, ::-1]], axis=1))


def bars_40x40() -> np.ndarray:
    """Two bright bars on black: constant along the bars, so Hessians are singular and extrema sit on exact plateaus."""
    a = np.zeros((40, 40), dtype=np.uint8)
    a[8:32, 12:15] = 255
    a[8:32, 24:28] = 255
    return a


def strip_12x200() -> np.ndarray:
    return _texture(5, 12, 200, 1.5)


def strip_200x12() -> np.ndarray:
    return np.ascontiguousarray(strip_12x200().T)


def odd_45x51() -> np.ndarray:
    """Doubles to 90 x 102: octaves 90 x 102, 45 x 51 (odd in both axes, so the decimation drops a row and a column), 22 x 25, 11 x 12."""
    return _texture(7, 45, 51, 1.8)


def noise_48x48() -> np.ndarray:
    """Nearly white noise: weak, crowded extrema whose refinement wanders, leaves the border and the layer range or does not converge."""
    return _texture(3, 48, 48, 0.7)


def dots_48x48() -> np.ndarray:
    """Bright and dark dots of several sizes on gray, some near the edge: maxima and minima, clipped windows, several orientations."""
    a = np.full((48, 48), 128.0)
    y, x = np.mgrid[0:48, 0:48].astype(np.float64)
    rng = np.random.default_rng(17)
    for _ in range(14):
        cy, cx = rng.uniform(2, 46, size=2)
        s = rng.uniform(1.0, 3.5)
        e = rng.uniform(0.5, 1.0)
        a += rng.choice((-1.0, 1.0)) * 120.0 * np.exp(-(((y - cy) * e) ** 2 + (x - cx) ** 2) / (2.0 * s * s))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def edge_dots_48x48(seed: int = 264) -> np.ndarray:
    """A vertical step edge with a few faint dots: along the edge the vertical difference is a few units in the last place below zero
    beside a large horizontal one, where the arc tangent rounds to exactly 360; descriptors beside the edge hold few strong elements."""
    rng = np.random.default_rng(seed)
    a = np.zeros((48, 48))
    a[:, 24:] = rng.integers(120, 256)
    y, x = np.mgrid[0:48, 0:48].astype(np.float64)
    for _ in range(rng.integers(1, 6)):
        cy, cx = rng.uniform(4, 44, 2)
        s = rng.uniform(1, 3)
        a += rng.choice((-1.0, 1.0)) * rng.uniform(20, 120) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def edge_atan_48x48() -> np.ndarray:
    """The same construction with another seed: here the arc tangent of 360 falls inside orientation windows (bin 36 wraps to 0)."""
    return edge_dots_48x48(62)


def claim_48x48() -> np.ndarray:
    """A fine texture in which two candidates converge on one position (the claim bit) and a ridge fails the edge ratio."""
    return _texture(0, 48, 48, 1.0)


IMAGES = {
    "blob_24x24": blob_24x24,
    "mirror_48x48": mirror_48x48,
    "bars_40x40": bars_40x40,
    "strip_12x200": strip_12x200,
    "strip_200x12": strip_200x12,
    "odd_45x51": odd_45x51,
    "noise_48x48": noise_48x48,
    "dots_48x48": dots_48x48,
    "claim_48x48": claim_48x48,
    "edge_dots_48x48": edge_dots_48x48,
    "edge_atan_48x48": edge_atan_48x48,
}


def images() -> Dict[str, np.ndarray]:
    return {name: make() for name, make in IMAGES.items()}


# ----------------------------------------------------------------------------------------------------------------------
# the restatement's decisions, re-derived and checked against it
# ----------------------------------------------------------------------------------------------------------------------
def _same(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def trace_solve3(a: np.ndarray, b: np.ndarray):
    """``S.solve3`` with its pivot choices: (X, singular (m,), exchanged (m, 3)). ``exchanged[:, i]`` is set where step i swaps rows and
    no earlier step has found the system singular (the device returns at the first singular pivot)."""
    a, b = a.astype(F).copy(), b.astype(F).copy()
    want = S.solve3(a, b)
    m = len(a)
    ar = np.arange(m)
    singular = np.zeros(m, dtype=bool)
    exchanged = np.zeros((m, 3), dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(3):
            k = np.full(m, i)
            for j in range(i + 1, 3):
                k = np.where(np.abs(a[:, j, i]) > np.abs(a[ar, k, i]), j, k)
            singular |= ~singular & (np.abs(a[ar, k, i]) < S.FLT_EPSILON * F(10.0))
            exchanged[:, i] = (k != i) & ~singular
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
    assert _same(b, want), "trace_solve3 departs from the restatement"
    return b, singular, exchanged


def trace_refine(dogs, candidates: np.ndarray, ev: Counter) -> Dict[str, np.ndarray]:
    """``S.refine`` with every decision counted; returns the restatement's own result after checking that the retraced one equals it."""
    want = S.refine(dogs, candidates)
    limit = F(2147483647 // 3)
    img_scale = F(1.0) / F(255.0)
    positions = []
    for o, d in enumerate(dogs):
        sel = candidates[candidates[:, 0] == o]
        if len(sel) == 0:
            continue
        _, h, w = d.shape
        l, r, c = (sel[:, i].astype(np.int64) for i in (1, 2, 3))
        m = len(sel)
        active, converged = np.ones(m, dtype=bool), np.zeros(m, dtype=bool)
        X, V, G, Hm = np.zeros((m, 3), dtype=F), np.zeros(m, dtype=F), np.zeros((m, 3), dtype=F), np.zeros((m, 3, 3), dtype=F)
        for _ in range(5):
            idx = np.flatnonzero(active & ~converged)
            if len(idx) == 0:
                break
            v, grad, hess = S._derivatives(d, l[idx], r[idx], c[idx])
            sol, singular, exchanged = trace_solve3(hess, grad)
            ev["singular_solve"] += int(singular.sum())
            ev["row_exchange_at_pivot_0"] += int(exchanged[:, 0].sum())
            ev["row_exchange_at_pivot_1"] += int(exchanged[:, 1].sum())
            x = -sol
            X[idx], V[idx], G[idx], Hm[idx] = x, v, grad, hess
            conv = (np.abs(x) < F(0.5)).all(axis=1)
            converged[idx[conv]] = True
            mv, xm = idx[~conv], x[~conv]
            ok = (np.abs(xm) <= limit).all(axis=1)
            ev["offset_beyond_limit"] += int((~ok).sum())
            active[mv[~ok]] = False
            mv, xm = mv[ok], xm[ok]
            step = np.rint(xm).astype(np.int64)
            ev["move_by_column"] += int((step[:, 0] != 0).sum())
            ev["move_by_row"] += int((step[:, 1] != 0).sum())
            ev["move_by_layer"] += int((step[:, 2] != 0).sum())
            c[mv] += step[:, 0]
            r[mv] += step[:, 1]
            l[mv] += step[:, 2]
            in_layers = (l[mv] >= 1) & (l[mv] <= S.LAYERS)
            in_border = (c[mv] >= S.BORDER) & (c[mv] < w - S.BORDER) & (r[mv] >= S.BORDER) & (r[mv] < h - S.BORDER)
            ev["leaves_layer_range"] += int((~in_layers).sum())
            ev["leaves_border"] += int((~in_border).sum())
            active[mv[~(in_layers & in_border)]] = False
        ev["five_steps_without_convergence"] += int((active & ~converged).sum())
        keep = active & converged
        t = (G[:, 0] * X[:, 0] + G[:, 1] * X[:, 1]) + G[:, 2] * X[:, 2]
        contr = V * img_scale + t * F(0.5)
        weak = (np.abs(contr) * F(3.0)).astype(np.float64) < 0.04
        ev["rejected_by_contrast"] += int((keep & weak).sum())
        keep &= ~weak
        dxx, dyy, dxy = Hm[:, 0, 0], Hm[:, 1, 1], Hm[:, 0, 1]
        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
        flat = det <= 0
        edge = ~flat & ((tr * tr).astype(np.float64) * 10.0 >= 121.0 * det.astype(np.float64))
        ev["rejected_by_det"] += int((keep & flat).sum())
        ev["rejected_by_edge_ratio"] += int((keep & edge).sum())
        keep &= ~(flat | edge)
        k = np.flatnonzero(keep)
        key = (l[k] * h + r[k]) * w + c[k]
        uniq = np.unique(key)
        ev["two_candidates_one_position"] += len(k) - len(uniq)
        for q in uniq:
            positions.append((o, q // (h * w), (q // w) % h, q % w))
    got = np.array(positions, dtype=np.int32).reshape(-1, 4)
    assert np.array_equal(got, np.stack([want[f] for f in ("octave", "layer", "row", "column")], axis=1)), "trace_refine departs from the restatement"
    return want


def peak_angle(j: int, hl, hj, hr):
    """The lines of ``S.histogram_peaks`` that turn a peak at bin j into an angle, without the peak test: the twin of the device's
    ``sift_peak_angle``. Returns (angle, raw bin, angle before the 360 -> 0 rule)."""
    hl, hj, hr = F(hl), F(hj), F(hr)
    with np.errstate(all="ignore"):
        raw = F(j) + F(0.5) * (hl - hr) / (hl - F(2.0) * hj + hr)
    b = F(36.0) + raw if raw < 0 else (raw - F(36.0) if raw >= F(36.0) else raw)
    before = F(360.0) - (F(360.0) / F(36.0)) * b
    angle = F(0.0) if abs(before - F(360.0)) < S.FLT_EPSILON else before
    return F(angle), raw, before


def trace_peaks(hist: np.ndarray, ev: Counter):
    """``S.histogram_peaks`` with the wraps counted; the angles are the restatement's own, checked against ``peak_angle``."""
    want = S.histogram_peaks(hist)
    thr = hist.max() * F(0.8)
    got = []
    for j in range(36):
        hl, hr, hj = hist[(j + 35) % 36], hist[(j + 1) % 36], hist[j]
        if hj > hl and hj > hr and hj >= thr:
            angle, raw, before = peak_angle(j, hl, hj, hr)
            ev["peak_bin_below_0"] += int(raw < 0)
            ev["peak_bin_at_least_36"] += int(raw >= F(36.0))
            ev["angle_360_set_to_0"] += int(abs(before - F(360.0)) < S.FLT_EPSILON)
            got.append(angle)
    assert len(got) == len(want) and all(F(a).tobytes() == F(b).tobytes() for a, b in zip(got, want)), "trace_peaks departs from the restatement"
    ev["two_peaks"] += int(len(want) == 2)
    ev["three_or_more_peaks"] += int(len(want) >= 3)
    return want


def trace_describe(img: np.ndarray, x, y, scl, angle, ev: Counter, calls: list) -> np.ndarray:
    """``S.describe_one`` with its window, its orientation-bin wraps, its clip and its saturation counted. ``calls`` is the list the
    ``atan2_deg`` wrapper appends to: the restatement's own call hands over the samples' arc tangents."""
    del calls[:]
    want = S.describe_one(img, x, y, scl, angle)
    (ang,) = [a for a in calls]  # one call per descriptor: the window's samples, in window order
    h, w = img.shape
    ori = F(360.0) - F(angle)
    if abs(ori - F(360.0)) < S.FLT_EPSILON:
        ori = F(0.0)
    px, py = int(np.rint(F(x))), int(np.rint(F(y)))
    cos_t, sin_t = S.sincos_deg(ori)
    hist_width = F(3.0) * F(scl)
    radius = int(np.rint(hist_width * F(1.4142135623730951) * F(5.0) * F(0.5)))
    diag = int(math.sqrt(float(w) * w + float(h) * h))
    ev["radius_clipped_by_diagonal"] += int(radius > diag)
    radius = min(radius, diag)
    cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
    rng = np.arange(-radius, radius + 1)
    i, j = (a.ravel() for a in np.meshgrid(rng, rng, indexing="ij"))
    fi, fj = i.astype(F), j.astype(F)
    c_rot = fj * cos_t - fi * sin_t
    r_rot = fj * sin_t + fi * cos_t
    rbin = r_rot + F(2.0) - F(0.5)
    cbin = c_rot + F(2.0) - F(0.5)
    r, c = py + i, px + j
    in_bins = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4)
    in_image = (r > 0) & (r < h - 1) & (c > 0) & (c < w - 1)
    ev["descriptor_window_clipped"] += int((in_bins & ~in_image).any())
    assert int((in_bins & in_image).sum()) == len(ang), "trace_describe's window departs from the restatement's"
    ev["fewer_than_64_samples"] += int(len(ang) < 64)
    o0 = np.floor((ang - ori) * (F(8.0) / F(360.0))).astype(np.int64)
    ev["o0_below_0_wraps"] += int((o0 < 0).sum())
    ev["o0_at_least_8_wraps"] += int((o0 >= 8).sum())
    # without a clip the largest element is at most 0.2 of the norm and 512 x 0.2 = 102.4 rounds to 102: more proves a clip
    ev["element_reaches_the_0.2_clip"] += int(want.max() >= 103)
    ev["element_saturates_at_255"] += int((want == 255).sum())
    return want


# ----------------------------------------------------------------------------------------------------------------------
# the census
# ----------------------------------------------------------------------------------------------------------------------
def census(image: np.ndarray, mask: Optional[np.ndarray] = None, describe: bool = True):
    """(events, stages): a Counter over ``EVENTS`` and the restatement's stage outputs for ``image`` (``pyramid`` flattened, ``candidates``,
    ``keypoints``, ``oriented`` after ``mask``, ``oriented_free`` without it, ``descriptors`` of every oriented keypoint)."""
    ev = Counter({name: 0 for name in EVENTS})
    gray = S.to_gray(image)
    atan2_calls, blurs, phase = [], [], ["atan2_equals_360"]
    real_atan2, real_blur = S.atan2_deg, S.gaussian_blur

    def counting_atan2(y, x):
        out = real_atan2(y, x)
        ev[phase[0]] += int((np.asarray(out) == F(360.0)).sum())
        atan2_calls.append(out)
        return out

    def counting_blur(img, sigma):
        blurs.append((img.shape, len(S.gaussian_taps(sigma)) // 2))
        return real_blur(img, sigma)

    S.atan2_deg, S.gaussian_blur = counting_atan2, counting_blur
    try:
        gaussians, dogs = S.build_pyramid(gray)
        for (bh, bw), radius in blurs:
            ev["blur_radius_exceeds_extent"] += int(radius >= min(bh, bw))  # an index -radius reflects to radius, beyond the last pixel
        shapes = [g.shape[1:] for g in gaussians]
        ev["odd_octave_is_decimated"] += sum(1 for hh, ww in shapes[:-1] if hh % 2 or ww % 2)
        cand = S.find_candidates(dogs)
        with_candidates = set(cand[:, 0].tolist())
        if with_candidates:
            ev["octave_too_small_beside_others"] += sum(1 for hh, ww in shapes if hh <= 2 * S.BORDER or ww <= 2 * S.BORDER)
        signs = np.array([dogs[o][l, r, c] > 0 for o, l, r, c in cand], dtype=bool)
        ev["maxima_and_minima"] += int(min(signs.sum(), (~signs).sum())) if len(cand) else 0
        at = {tuple(row) for row in cand.tolist()}
        ev["adjacent_candidates_in_a_layer"] += sum(
            1 for o, l, r, c in at if any((o, l, r + dr, c + dc) in at for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr, dc) != (0, 0)))
        kp = trace_refine(dogs, cand, ev)
        for t in range(len(kp["octave"])):
            o, l, r, c, scl = int(kp["octave"][t]), int(kp["layer"][t]), int(kp["row"][t]), int(kp["column"][t]), kp["scl"][t]
            hh, ww = shapes[o]
            radius = int(np.rint(F(4.5) * scl))
            ev["orientation_window_clipped"] += int(r - radius <= 0 or r + radius >= hh - 1 or c - radius <= 0 or c + radius >= ww - 1)
            trace_peaks(S.orientation_histogram(gaussians[o][l], r, c, scl), ev)
            ev["keypoint_in_a_thin_strip"] += int(min(gray.shape) <= 12)
            ev["keypoint_in_a_12_pixel_octave"] += int(min(hh, ww) == 12)
        free = S.orient(gaussians, kp, None)
        ori = S.orient(gaussians, kp, mask) if mask is not None else free
        if mask is not None and len(kp["octave"]):
            xy = np.rint(S.final_xy(kp)).astype(np.int64)
            ev["dropped_by_mask"] += int((mask[np.clip(xy[:, 1], 0, mask.shape[0] - 1), np.clip(xy[:, 0], 0, mask.shape[1] - 1)] == 0).sum())
        ties, across = response_ties(free)
        ev["equal_response_different_keypoints"] += ties
        ev["equal_response_across_layers_or_octaves"] += across
        n = len(free["angle"])
        desc = np.zeros((n, 128), dtype=F)
        phase[0] = "descriptor_atan2_equals_360"
        if describe:  # every oriented keypoint of the unmasked image
            for t in range(n):
                desc[t] = trace_describe(gaussians[free["octave"][t]][free["layer"][t]], free["x"][t], free["y"][t], free["scl"][t], free["angle"][t], ev,
                                         atan2_calls)
    finally:
        S.atan2_deg, S.gaussian_blur = real_atan2, real_blur
    stages = {"pyramid": S.flatten_pyramid(gaussians, dogs), "candidates": cand, "keypoints": kp, "oriented": ori, "oriented_free": free, "descriptors": desc}
    return ev, stages


def _position(ori, t):
    return tuple(int(ori[f][t]) for f in ("octave", "layer", "row", "column"))


def response_ties(ori: Dict[str, np.ndarray]):
    """(pairs of neighbours in the output order that are different keypoints with bit-equal responses, those of them in different layers or
    octaves)."""
    ties = across = 0
    for t in range(1, len(ori["angle"])):
        if ori["response"][t].tobytes() == ori["response"][t - 1].tobytes() and _position(ori, t) != _position(ori, t - 1):
            ties += 1
            across += int(_position(ori, t)[:2] != _position(ori, t - 1)[:2])
    return ties, across


def tie_cuts(ori: Dict[str, np.ndarray]):
    """Every k at which the first k output rows end between two different keypoints of equal response."""
    return [t for t in range(1, len(ori["angle"]))
            if ori["response"][t].tobytes() == ori["response"][t - 1].tobytes() and _position(ori, t) != _position(ori, t - 1)]


def lone_keypoint_pixel(kp: Dict[str, np.ndarray]):
    """(index, (x, y)) of the first keypoint whose rounded final coordinates no other keypoint shares, or None."""
    xy = np.rint(S.final_xy(kp)).astype(np.int64)
    for t in range(len(xy)):
        if (xy == xy[t]).all(axis=1).sum() == 1:
            return t, (int(xy[t, 0]), int(xy[t, 1]))
    return None


def lone_keypoint_mask(image: np.ndarray, kp: Dict[str, np.ndarray]):
    """A mask that is zero but for one pixel, to which exactly one keypoint's ``rint`` coordinates fall: (mask, index, (x, y))."""
    t, (x, y) = lone_keypoint_pixel(kp)
    assert 0 <= x < image.shape[1] and 0 <= y < image.shape[0]  # inside the image: the clamp of the mask lookup plays no part
    mask = np.zeros(image.shape[:2], dtype=np.uint8)
    mask[y, x] = 1
    return mask, t, (x, y)


def half_mask(shape, seed: int) -> np.ndarray:
    """A seeded mask of 6 x 6 blocks, about half of them on."""
    h, w = shape
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 2, size=((h + 5) // 6, (w + 5) // 6), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(blocks, np.ones((6, 6), dtype=np.uint8))[:h, :w])


def table(counts: Dict[str, Counter]) -> str:
    names = list(counts)
    width = max(len(e) for e in EVENTS)
    head = " " * width + "".join(f" {n[:12]:>12}" for n in names)
    rows = [head] + [f"{e:<{width}}" + "".join(f" {counts[n][e]:>12}" for n in names) for e in EVENTS]
    return "\n".join(rows)
