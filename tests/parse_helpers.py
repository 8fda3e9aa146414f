"""Shared by test_parse_cpu.py / test_parse_gpu.py: the float64 restatement of the scene parse's definition on raw operands, the
comparison rule against the reference's fixtures (tests/golden/parse_<case>.npz, make_golden_parse.py) and the fixture cases.

Definition (include/spair_hip.h, "scene parse"): for sample b, pixel (y, x) and cell k = h * Gw + w
    a_k = warp(alpha_k * pres_k),  m_k = warp(max(alpha_k * pres_k * depth_k, 0.01)),  D = sum_k m_k + HW * 1e-9,
    w_k = a_k (m_k + 1e-9) / D,  coverage = sum_k w_k,  owner_weight = max_k w_k,  owner = lowest arg-max (or -1: weight 0 / below threshold).
warp = bilinear, zero-padded inverse-STN sampling: a sum over the sprite's texels of hat(sx - u) hat(sy - v), hat(t) = max(0, 1 - |t|)."""
import os

import numpy as np

import golden_inputs as gi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the comparison rule of the fixtures: weights to W_TOL absolute (the bound the fp32 step's recon is held to: recon is this same sum of w_k
# times a colour in [0, 1]); an owner may differ only where two weights that close could swap
W_TOL = 2e-4
MAX_LEFT_OUT = 0.03
THRESHOLDS = (0.0, 0.25)

RECT_CASES = {"rect_h48w80_b4_step1001": dict(C=1, H=48, W=80, strides=(2, 2, 2, 1, 1, 1), B=4, wseed=31, wscale=1.0)}
PARSE_CASES = ("c1_b8_step7001", "c2_b2_step1001", "ref_default_b2_step1001", "c4_b1_step1001", "p24_c1_b4_step1001", "lb2_c1_b4_step1001",
               "rgb_c1_b4_step1001", "rect_h48w80_b4_step1001")


def case_of(name):
    """{C, H, W, strides, P, lookback, wseed, wscale} of a fixture case."""
    if name in RECT_CASES:
        c = RECT_CASES[name]
        return dict(C=c["C"], H=c["H"], W=c["W"], strides=c["strides"], P=gi.OBJ_PX, lookback=1, wseed=c["wseed"], wscale=c["wscale"])
    c = gi.all_cases()[name]
    return dict(C=c.get("in_chan", 1), H=c["I"], W=c["I"], strides=tuple(c["strides"]), P=c.get("obj_px", gi.OBJ_PX),
                lookback=c.get("lookback", 1), wseed=c["wseed"], wscale=c["wscale"])


def load_parse(name):
    return np.load(os.path.join(GOLDEN, "parse_" + name + ".npz")), np.load(os.path.join(GOLDEN, name + ".npz"))


def src_coords(t, s, n_out, P, align_corners):
    """Source coordinate (texel units) of every output index: t, s [N] (centre, scale fractions) -> [N, n_out], float64."""
    j = np.arange(n_out, dtype=np.float64)
    if align_corners:
        base = 2 * j / (n_out - 1) - 1 if n_out > 1 else np.zeros(1)
    else:
        base = (2 * j + 1) / n_out - 1
    g = base[None, :] / s[:, None] - ((2 * t - 1) / s)[:, None]
    return (g + 1) / 2 * (P - 1) if align_corners else ((g + 1) * P - 1) / 2


def composite_parts(alpha, nbox, pres, depth, I, Iw, align_corners=False, dtype=np.float64):
    """alpha [B,HW,P,P] (after the sigmoid), nbox [B,HW,4] = (xt, yt, xs, ys), pres / depth [B,HW] -> (a, m, reach), each [B,HW,I,Iw]:
    the warped alpha * pres, the warped importance, and where the pixel's source coordinate lies within a hundredth of a texel of the
    zero-padded sprite's support (-1, P) -- where an fp32 evaluation of the coordinate may see the object at all."""
    alpha, nbox, pres, depth = (np.asarray(v, dtype) for v in (alpha, nbox, pres, depth))
    B, HW, P, _ = alpha.shape
    n = B * HW
    nb = nbox.reshape(n, 4)
    u = np.arange(P, dtype=dtype)
    sx, sy = src_coords(nb[:, 0], nb[:, 2], Iw, P, align_corners), src_coords(nb[:, 1], nb[:, 3], I, P, align_corners)
    hx = np.maximum(0, 1 - np.abs(sx.astype(dtype)[:, :, None] - u))      # [n, Iw, P]
    hy = np.maximum(0, 1 - np.abs(sy.astype(dtype)[:, :, None] - u))      # [n, I, P]
    ap = alpha.reshape(n, P, P) * pres.reshape(n, 1, 1)
    mp = np.maximum(ap * depth.reshape(n, 1, 1), dtype(0.01))
    a = np.einsum("niv,nvu,nju->nij", hy, ap, hx).reshape(B, HW, I, Iw)
    m = np.einsum("niv,nvu,nju->nij", hy, mp, hx).reshape(B, HW, I, Iw)
    near = lambda s: (s > -1.01) & (s < P + 0.01)
    return a, m, (near(sy)[:, :, None] & near(sx)[:, None, :]).reshape(B, HW, I, Iw)


def composite_weights(alpha, nbox, pres, depth, I, Iw, align_corners=False):
    """w [B,HW,I,Iw], float64 (the definition)."""
    a, m, _ = composite_parts(alpha, nbox, pres, depth, I, Iw, align_corners)
    return a * (m + 1e-9) / (m.sum(axis=1, keepdims=True) + a.shape[1] * 1e-9)


def fp32_bounds(a, m, reach, nbox, pres, P):
    """How far an fp32 evaluation of the definition on the same stored operands may lie from the float64 one, from the operands' magnitudes.
    The source coordinate s = ((fma(ax, base, bx) + 1) P - 1) / 2 with ax = 1 / xs, bx = -(2 xt - 1) / xs carries one rounding of ax, two of
    bx (and 2 xt - 1's, divided by xs), two of base (|base| <= 1) and those of the fma (|g| <~ 1.1 where the object reaches) and of the
    unnormalisation: |dg| <= 2^-23 (2.5 |ax| + |bx| + 0.55), |ds| <= P/2 |dg| + 2^-24 (2.05 P + 0.5) <= 2^-24 P (2.5 |ax| + |bx| + 3) =: d
    per axis.  The zero-padded bilinear interpolation of texels in [0, 1] is 1-Lipschitz in each coordinate, so where the object can reach
    the pixel |da_k| <= (dx + dy) pres_k + 2^-22 and |dm_k| <= dx + dy + 2^-22 (the 2^-22: the tap weights' own roundings and the
    four-term sums of values <= 1).  Propagated through u = a (m + 1e-9), D = sum m + HW 1e-9 (n terms: n 2^-24 D) and w = u / D, each
    with its own rounding.  Returns (w, E_w [B,HW,I,Iw], E_cov [B,I,Iw]); a bound is inf where D itself is within its error of 0."""
    B, HW = a.shape[:2]
    nb = np.asarray(nbox, np.float64).reshape(B, HW, 4)
    d_axis = lambda t, s: 2.0 ** -24 * P * (2.5 / s + np.abs(2 * t - 1) / s + 3)
    d = (d_axis(nb[..., 0], nb[..., 2]) + d_axis(nb[..., 1], nb[..., 3]))[:, :, None, None]
    pr = np.asarray(pres, np.float64).reshape(B, HW, 1, 1)
    E_a = (d * pr + 2.0 ** -22 * (pr > 0)) * reach           # (a presence of exactly 0 gives a = 0 exactly, in any precision)
    E_m = (d + 2.0 ** -22) * reach
    u = a * (m + 1e-9)
    D = m.sum(axis=1, keepdims=True) + HW * 1e-9
    n = reach.sum(axis=1, keepdims=True)
    E_u = E_a * (m + E_m + 1e-9) + a * E_m + 2.0 ** -22 * u
    E_D = E_m.sum(axis=1, keepdims=True) + (n + 1) * 2.0 ** -24 * D
    with np.errstate(divide="ignore", invalid="ignore"):
        D_lo = np.where(D - E_D > 0, D - E_D, np.nan)
        w = u / D
        E_w = np.where(np.isnan(D_lo), np.inf, E_u / D_lo + w * E_D / D_lo + 2.0 ** -22 * w)
    E_w = np.where(reach, E_w, 0.0)
    E_cov = E_w.sum(axis=1) + (n[:, 0] + 1) * 2.0 ** -24
    return w, E_w, E_cov


def check_on_operands(alpha, nbox, pres, depth, got, threshold, align_corners=False, twin=None, what="", max_undecided=0.05):
    """The kernel's outputs ``got`` = (owner, owner_weight, coverage, area) as numpy [B,I,Iw] / [B,HW] against the float64 definition on the
    same stored operands (cell order: alpha [B,HW,P,P], nbox [B,HW,4], pres / depth [B,HW]), at fp32_bounds.  ``twin`` = (b, k1, k2): cell k2
    of sample b is a copy of k1 < k2 -- every weight of the two is equal, so k2 may never own a pixel.  The owner is compared wherever the
    largest weight leads the second by more than their two bounds and is further than its bound from the threshold (and wherever no object
    reaches the pixel at all); at most
    ``max_undecided`` of the pixels may fall outside that.  area is exact: a bincount of owner."""
    owner, weight, coverage, area = (np.asarray(v) for v in got)
    B, HW, P, _ = np.asarray(alpha).shape
    I, Iw = owner.shape[1:]
    a, m, reach = composite_parts(alpha, nbox, pres, depth, I, Iw, align_corners)
    w, E_w, E_cov = fp32_bounds(a, m, reach, nbox, pres, P)
    E_pix = E_w.max(axis=1)
    cov = w.sum(axis=1)
    wt = w.copy()
    if twin is not None:
        b, k1, k2 = twin
        assert np.array_equal(w[b, k1], w[b, k2])
        assert not (owner[b] == k2).any(), "the copy with the higher index owns pixels"
        wt[b, k2] = 0.0          # (it can never lead: compare the owners of the problem without it)
    k, w1, w2, _ = top2(wt)
    fin = np.isfinite(E_pix)
    r_w = np.abs(weight - w1)[fin] / (E_pix[fin] + 1e-30)
    r_c = np.abs(coverage - cov)[fin] / (E_cov[fin] + 1e-30)
    live = (w1 > 0) | (E_pix > 0)          # (elsewhere no object reaches the pixel, in fp32 either: the owner is -1, decided)
    undecided = ~fin | (live & ((w1 - w2 <= 2 * E_pix) | (np.abs(w1 - threshold) <= E_pix)))
    want = owner_of(k, w1, threshold)
    wrong = (owner != want) & ~undecided
    print("%s thr %.2f: owner_weight err %.3g (%.3f of its bound; bound median %.3g, max finite %.3g), coverage err %.3g (%.3f of its bound), "
          "undecided %.4f, owned %.3f, wrong owners %d" % (what, threshold, np.abs(weight - w1)[fin].max(), r_w.max(), np.median(E_pix[fin]),
                                                           E_pix[fin].max(), np.abs(coverage - cov)[fin].max(), r_c.max(), undecided.mean(),
                                                           (want >= 0).mean(), wrong.sum()))
    assert r_w.max() <= 1 and r_c.max() <= 1, (what, r_w.max(), r_c.max())
    # the bound must bind: finite on all but the fringe pixels whose whole denominator is rounding-sized, and for the typical pixel below
    # half of what the reference fixtures are compared at
    assert fin.mean() >= 0.99 and np.median(E_pix[fin]) < 0.5 * W_TOL, ("vacuous bound", fin.mean(), np.median(E_pix[fin]))
    assert undecided.mean() <= max_undecided, (what, undecided.mean())
    assert not wrong.any(), (what, int(wrong.sum()))
    assert ((weight >= 0) & (coverage >= weight * (1 - 1e-6))).all()
    counts = np.stack([np.bincount(owner[b][owner[b] >= 0], minlength=HW) for b in range(B)])
    assert np.array_equal(area, counts), "area is not the bincount of owner"
    assert int(area.sum()) + int((owner < 0).sum()) == B * I * Iw
    assert owner.min() >= -1 and owner.max() < HW


def top2(w):
    """w [B,HW,...] -> (arg-max with the lowest index on ties, largest, second largest, sum)."""
    k = np.argmax(w, axis=1)
    if w.shape[1] == 1:
        w1 = w[:, 0]
        return k, w1, np.zeros_like(w1), w1
    p = -np.partition(-w, 1, axis=1)[:, :2]
    return k, p[:, 0], p[:, 1], w.sum(axis=1)


def owner_of(k, w1, threshold):
    return np.where((w1 > 0) & (w1 >= threshold), k, -1)


def left_out(w1, w2, threshold):
    """The pixels whose owner is not compared: two weights within twice the bound could swap, or the maximum is that close to the threshold."""
    return (w1 - w2 <= 2 * W_TOL) | (np.abs(w1 - threshold) <= W_TOL)


def check_against_fixture(fx, owner, weight, coverage, threshold, what=""):
    """The comparison rule.  fx: the parse fixture (possibly the top rows of the canvas only); owner / weight / coverage: [B,I,Iw] of the
    code under test at ``threshold``.  Returns the left-out share."""
    rows = fx["owner"].shape[1]
    owner, weight, coverage = (np.asarray(v)[:, :rows] for v in (owner, weight, coverage))
    w1, w2 = fx["w1"].astype(np.float64), fx["w2"].astype(np.float64)
    ew, ec = np.abs(weight - w1).max(), np.abs(coverage - fx["coverage"].astype(np.float64)).max()
    out = left_out(w1, w2, threshold)
    want = owner_of(fx["owner"].astype(np.int64), w1, threshold)
    wrong = (owner != want) & ~out
    print("%s threshold %.2f: |owner_weight - w1| %.3g, |coverage - ref| %.3g, left out %.4f, owned %.3f, wrong owners %d"
          % (what, threshold, ew, ec, out.mean(), (want >= 0).mean(), wrong.sum()))
    assert ew <= W_TOL and ec <= W_TOL, (what, ew, ec)
    assert out.mean() <= MAX_LEFT_OUT, (what, out.mean())
    assert not wrong.any(), (what, threshold, int(wrong.sum()))
    return float(out.mean())


def make_unit_case(seed, B, G, Gw, I, Iw, P, ch, permute):
    """Made-up operands of the owner kernel, in cell order: boxes of four kinds by k % 4 -- ordinary, magnified (up to 1.4 canvases wide),
    minified to 3 - 6 pixels, half outside the canvas -- random texels, presences (a tenth exactly 0) and depths; in sample 0 cell k2 is a
    copy of the large, fully present cell k1 < k2 (an exact tie).  Returns dict(alpha [B,HW,P,P] float64 of the values to be STORED -- the
    caller rounds them to the sprite type first --, texels [B,HW,P*P,ch] (alpha last), nbox, pres, depth, rows [HW] or None, twin)."""
    rng = np.random.default_rng(seed)
    HW = G * Gw
    k = np.arange(HW)[None, :].repeat(B, 0)
    kind = k % 4
    xt, yt = rng.uniform(0.1, 0.9, (B, HW)), rng.uniform(0.1, 0.9, (B, HW))
    xs, ys = rng.uniform(0.15, 0.5, (B, HW)), rng.uniform(0.15, 0.5, (B, HW))
    big = kind == 1
    xs[big], ys[big] = rng.uniform(0.8, 1.4, big.sum()), rng.uniform(0.8, 1.4, big.sum())
    tiny = kind == 2
    xs[tiny], ys[tiny] = rng.uniform(3.0, 6.0, tiny.sum()) / Iw, rng.uniform(3.0, 6.0, tiny.sum()) / I
    edge = kind == 3
    xt[edge] = rng.choice([0.0, 1.0], edge.sum()) + rng.uniform(-0.03, 0.03, edge.sum())
    pres = rng.uniform(0.0, 1.0, (B, HW))
    pres[rng.uniform(size=(B, HW)) < 0.1] = 0.0
    depth = rng.uniform(0.05, 1.0, (B, HW))
    texels = rng.uniform(0.0, 1.0, (B, HW, P * P, ch))
    k1, k2 = HW // 3, HW // 3 + 5
    xt[0, k1], yt[0, k1], xs[0, k1], ys[0, k1], pres[0, k1], depth[0, k1] = 0.45, 0.55, 0.45, 0.5, 1.0, 1.0
    texels[0, k1, :, ch - 1] = rng.uniform(0.8, 1.0, P * P)
    for v in (xt, yt, xs, ys, pres, depth, texels):
        v[0, k2] = v[0, k1]
    nbox = np.stack((xt, yt, xs, ys), -1).astype(np.float32)
    return dict(texels=texels, nbox=nbox, pres=pres.astype(np.float32), depth=depth.astype(np.float32),
                rows=rng.permutation(HW).astype(np.int32) if permute else None, twin=(0, k1, k2))
