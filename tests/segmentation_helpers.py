"""References for the instance masks of the scene generator and for the segmentation metrics -- numpy, float64 and exact integers.

scene_planes:      oracle/scenes_oracle.generate restated per glyph: the same image, bbox and count, plus every glyph's own plane.
mask_rule:         the mask the planes define (the glyph with the largest value, the lowest index on a tie, -1 where nothing is lit) and
                   the pixels a device comparison leaves out: the device contracts a * b + c into an fma, so its values may differ from
                   numpy's by a rounding, which can flip a decision only where the two candidates are closer than that.
segmentation_ref:  the definitions of include/spair_hip.h ("segmentation metrics") on Python integers: nothing is rounded before the one
                   division of each score.

The five scene cases the CPU and GPU tests share are SCENE_CASES.
"""
from fractions import Fraction

import numpy as np

from oracle import scenes_oracle as so

# (B, I, K, seed, first, smin, smax)
SCENE_CASES = [(8, 64, 7, 1234, 0, 14, 28), (4, 128, 11, 7, 100, 14, 28), (6, 48, 5, 99, 3, 8, 20), (8, 32, 11, 5, 0, 14, 28),
               (5, 40, 32, 11, 0, 6, 12)]
LEFT_OUT_CAP = 1e-3          # share of a case's pixels that mask_rule may leave out
MARGIN = 1e-5                # fp32 values in [0, 1] formed by a handful of operations: an fma changes them by a few 2^-24


def scene_planes(seed, first, B, I, K, smin=14, smax=28):
    """(image [B,1,I,I], bbox [B,K,4], count [B], planes [B,K,I,I]): planes[b, j] is glyph j alone on the canvas (zeros for j >= count)."""
    f = np.float32
    planes = np.zeros((B, K, I, I), np.float32)
    bbox = np.zeros((B, K, 4), np.float32)
    count = np.zeros((B,), np.int64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for b in range(B):
        gi = first + b
        g0, g1 = gi & 0xFFFFFFFF, (gi >> 32) & 0xFFFFFFFF
        k = so.philox(g0, g1, 0, 0, k0, k1)[0] % (K + 1)
        count[b] = k
        for j in range(k):
            r = so.philox(g0, g1, 1 + j, 0, k0, k1)
            size = min(smin + r[0] % (smax - smin + 1), I)
            y0, x0 = r[1] % (I - size + 1), r[2] % (I - size + 1)
            ns = 2 + (r[3] & 1)
            bbox[b, j] = (x0, y0, size, size)
            n = f(size)
            c = (n - f(1)) * f(0.5)
            yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
            g = np.zeros((size, size), np.float32)
            for s in range(ns):
                a = so.philox(g0, g1, 1 + j, 1 + 2 * s, k0, k1)
                q = so.philox(g0, g1, 1 + j, 2 + 2 * s, k0, k1)
                arc = so.uni(a[0]) < f(0.45)
                vx, vy = f(2) * so.uni(q[0]) - f(1), f(2) * so.uni(q[1]) - f(1)
                vn = np.sqrt(vx * vx + vy * vy, dtype=np.float32)
                if vn < f(1e-3):
                    vx, vy = f(1), f(0)
                else:
                    vx, vy = vx / vn, vy / vn
                if arc:
                    cy = c + (f(0.3) * so.uni(a[1]) - f(0.15)) * n
                    cx = c + (f(0.3) * so.uni(a[2]) - f(0.15)) * n
                    r0 = (f(0.2) + f(0.22) * so.uni(a[3])) * n
                    cth = f(1.3) * so.uni(q[2]) - f(1)
                    dy, dx = yy - cy, xx - cx
                    rr = np.sqrt(dy * dy + dx * dx, dtype=np.float32)
                    v = np.clip(f(1.4) - np.abs(rr - r0) / f(1.2), 0, 1).astype(np.float32)
                    v = np.where(dx * vx + dy * vy >= cth * rr, v, f(0))
                else:
                    cy = c + (f(0.4) * so.uni(a[1]) - f(0.2)) * n
                    cx = c + (f(0.4) * so.uni(a[2]) - f(0.2)) * n
                    hl = (f(0.25) + f(0.2) * so.uni(a[3])) * n
                    dy, dx = yy - cy, xx - cx
                    across, along = np.abs(dy * vx - dx * vy), np.abs(dy * vy + dx * vx)
                    v = np.clip(f(1.4) - across / f(1.2), 0, 1).astype(np.float32)
                    v = np.where(along < hl, v, f(0))
                g = np.maximum(g, v.astype(np.float32))
            planes[b, j, y0:y0 + size, x0:x0 + size] = g
    image = planes.max(axis=1, keepdims=True)
    return image, bbox, count, planes


def mask_rule(planes):
    """(mask int32 [B,I,I], left_out bool [B,I,I], stats dict).  Left out: a top value in (0, MARGIN) (lit or not is a rounding away),
    0 < top1 - top2 <= MARGIN (which glyph is larger is a rounding away), and top1 == top2 < 1 between two glyphs (equal here, maybe not
    on the device).  Exact ties at the saturated value 1.0 are exact on the device too and stay in: they test the lowest-index rule."""
    p = np.asarray(planes, np.float32)
    B, K = p.shape[:2]
    top1 = p.max(axis=1)
    who = p.argmax(axis=1).astype(np.int32)                     # numpy's argmax: the first (lowest) index of the maximum
    if K > 1:
        top2 = np.sort(p, axis=1)[:, -2]                        # the largest value of any OTHER glyph (equal to top1 on a tie)
    else:
        top2 = np.zeros_like(top1)
    mask = np.where(top1 > 0, who, np.int32(-1)).astype(np.int32)
    d = top1.astype(np.float64) - top2.astype(np.float64)
    faint = (top1 > 0) & (top1 < MARGIN)
    close = (d > 0) & (d <= MARGIN)
    soft_tie = (top1 > 0) & (top1 == top2) & (top1 < 1)
    stats = dict(foreground=float((top1 > 0).mean()), overlap=int((top2 > 0).sum()), ties=int(((top1 == top2) & (top1 > 0)).sum()),
                 saturated_ties=int(((top1 == top2) & (top1 == 1)).sum()))
    return mask, faint | close | soft_tie, stats


def clean_labels(a, n):
    """labels outside {0 .. n-1} -> -1 (background), as int64"""
    a = np.asarray(a).astype(np.int64)
    return np.where((a >= 0) & (a < n), a, -1)


def c2(v):
    return v * (v - 1) // 2


def ari_exact(X, A, Bs, C):
    """(X - E) / (M - E), E = A Bs / C, M = (A + Bs) / 2, on Python integers; 1.0 where M = E (C = 0 included)."""
    num = 2 * (X * C - A * Bs)
    den = (A + Bs) * C - 2 * A * Bs
    if den == 0:
        return 1.0
    return float(Fraction(num, den))


def segmentation_ref(pred, truth, NP, K):
    """pred, truth: integer arrays [B, ...] (any trailing shape).  Returns dict(contingency int64 [B,NP+1,K+1], scores float64 [B,5] =
    (ari, ari_fg, msc, sc, fg_iou), match int64 [B,K], match_iou float64 [B,K])."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    B = pred.shape[0]
    p = clean_labels(pred, NP).reshape(B, -1) + 1
    t = clean_labels(truth, K).reshape(B, -1) + 1
    N = p.shape[1]
    cont = np.zeros((B, NP + 1, K + 1), np.int64)
    scores = np.zeros((B, 5), np.float64)
    match = np.full((B, K), -1, np.int64)
    miou = np.zeros((B, K), np.float64)
    for b in range(B):
        n = np.bincount(p[b] * (K + 1) + t[b], minlength=(NP + 1) * (K + 1)).reshape(NP + 1, K + 1).astype(np.int64)
        cont[b] = n
        a, bj = n.sum(axis=1), n.sum(axis=0)
        X, A, Bs = int(c2(n).sum()), int(c2(a).sum()), int(c2(bj).sum())
        scores[b, 0] = ari_exact(X, A, Bs, c2(N))
        Nf = int(N - bj[0])
        if Nf > 0:
            nf = n[:, 1:]
            scores[b, 1] = ari_exact(int(c2(nf).sum()), int(c2(nf.sum(axis=1)).sum()), int(c2(bj[1:]).sum()), c2(Nf))
        else:
            scores[b, 1] = np.nan
        best, weight = [], []
        for j in range(1, K + 1):
            if bj[j] == 0:
                continue
            top, arg = Fraction(0), -1
            for i in np.nonzero(n[1:, j])[0] + 1:                # ascending i: a strict > keeps the lowest label of a tie
                q = Fraction(int(n[i, j]), int(a[i] + bj[j] - n[i, j]))
                if q > top:
                    top, arg = q, int(i) - 1
            match[b, j - 1], miou[b, j - 1] = arg, float(top)
            best.append(top)
            weight.append(int(bj[j]))
        if best:
            scores[b, 2] = float(sum(best) / len(best))
            scores[b, 3] = float(sum(q * w for q, w in zip(best, weight)) / sum(weight))
        else:
            scores[b, 2] = scores[b, 3] = np.nan
        union = N - int(n[0, 0])
        inter = N + int(n[0, 0]) - int(a[0]) - int(bj[0])
        scores[b, 4] = inter / union if union else 1.0
    return dict(contingency=cont, scores=scores, match=match, match_iou=miou)


def blocky_maps(seed, B, H, W, NP, K, background=0.5, block=4):
    """Made-up label maps with structure (runs of equal labels, as a parse has): labels drawn per block x block tile, the tiles of pred
    and truth offset against each other, a share `background` of the tiles -1; then a sprinkling of single-pixel labels, the highest
    labels NP-1 and K-1 among them."""
    rng = np.random.default_rng(seed)

    def one(n, off):
        th, tw = (H + off) // block + 2, (W + off) // block + 2
        tiles = rng.integers(0, n, size=(B, th, tw))
        tiles[rng.uniform(size=tiles.shape) < background] = -1
        full = np.repeat(np.repeat(tiles, block, axis=1), block, axis=2)[:, off:off + H, off:off + W]
        full = np.ascontiguousarray(full)
        noise = rng.uniform(size=full.shape) < 0.05
        full[noise] = rng.integers(-1, n, size=int(noise.sum()))
        full.reshape(B, -1)[:, rng.integers(0, H * W)] = n - 1
        return full.astype(np.int32)
    return one(NP, 0), one(K, 1)
