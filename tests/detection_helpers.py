"""References for the detection metrics (include/spair_hip.h, "detection metrics") -- numpy float32 for the IoU, plain Python loops and
integers for everything else.  Nothing here takes anything from the code under test.

iou_ref:    the IoU operation by operation in numpy float32 (an element-wise float32 op rounds once and never fuses).
match_ref:  live predictions, the ranked list, the greedy one-to-one matching per threshold, in Python loops over an IoU matrix.
ap_ref:     the pooled curve on Python integers; precisions and the envelope are fractions.Fraction (exact), and the sum is converted to
            float once: exactly (a Fraction sum) up to EXACT_RECORDS records, and beyond that as math.fsum of the correctly rounded
            envelope values (fsum is the exact sum of its arguments rounded once: at most 2^-53 relative per term, 1.2e-16 on the AP).
count_ref:  the three count statistics from integer sums.
make_case:  truth boxes, then predictions as jittered copies, exact duplicates, strays and near-misses.  Family "quarter": every coordinate
            a multiple of 0.25 px in [0, 512): widths have at most 11 significant bits, areas 22, their sums 23, so every product and sum
            of the IoU is exact in fp32 and only the correctly rounded division rounds -- numpy and the device must agree to the bit
            however a compiler contracts.  Family "float": the same boxes moved by arbitrary fp32 amounts, which proves the absence of
            contraction.
"""
import math
from fractions import Fraction

import numpy as np

F = np.float32
EXACT_RECORDS = 2048


def default_thresholds():
    """torch.arange(0.1, 1.0, 0.1) in fp32, the accumulator's default"""
    import torch
    return torch.arange(0.1, 1.0, 0.1).numpy().astype(F)


def iou_ref(boxes, bbox):
    """boxes [..., N, 4] corners, bbox [..., K, 4] = (x, y, w, h) -> float32 [..., N, K]"""
    a = np.asarray(boxes, dtype=F)[..., :, None, :]
    b = np.asarray(bbox, dtype=F)[..., None, :, :]
    with np.errstate(all="ignore"):
        ax0, ay0, ax1, ay1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
        bx0, by0 = b[..., 0], b[..., 1]
        bx1, by1 = bx0 + b[..., 2], by0 + b[..., 3]
        iw = np.maximum(np.minimum(ax1, bx1) - np.maximum(ax0, bx0), F(0))
        ih = np.maximum(np.minimum(ay1, by1) - np.maximum(ay0, by0), F(0))
        inter = iw * ih
        ua = (ax1 - ax0) * (ay1 - ay0)
        ub = (bx1 - bx0) * (by1 - by0)
        un = (ua + ub) - inter
        q = inter / un
        ok = np.isfinite(ax0) & np.isfinite(ay0) & np.isfinite(ax1) & np.isfinite(ay1) & np.isfinite(bx0) & np.isfinite(by0) & \
            np.isfinite(bx1) & np.isfinite(by1)
        out = np.where(ok & (un > 0) & (q > 0), q, F(0))
    assert out.dtype == F
    return out


def match_ref(iou, scores, cnt, thr, min_score, max_det):
    """one image: iou [N, K], scores [N] -> dict(order, score, tp: lists over the kept predictions in ranked order; n_pred; n_truth)"""
    iou, scores = np.asarray(iou, dtype=F), np.asarray(scores, dtype=F)
    N, K = iou.shape
    cnt = min(max(int(cnt), 0), K)
    lo = F(min_score)
    live = [n for n in range(N) if not math.isnan(float(scores[n])) and scores[n] >= lo]
    ranked = sorted(live, key=lambda n: (-float(scores[n]), n))
    kept = ranked[:max_det]
    tp = [0] * len(kept)
    rows = {n: iou[n].tolist() for n in kept}                   # fp32 values as Python floats: exact, and the compares are the same
    for t, th in enumerate(np.asarray(thr, dtype=F).tolist()):
        taken = [False] * cnt
        for r, n in enumerate(kept):
            best, bj, row = -1.0, -1, rows[n]
            for j in range(cnt):
                if not taken[j] and row[j] > best:              # strictly larger: the lowest j on equal IoU
                    best, bj = row[j], j
            if bj >= 0 and best >= th:
                tp[r] |= 1 << t
                taken[bj] = True
    return dict(order=kept, score=[scores[n] for n in kept], tp=tp, n_pred=len(live), n_truth=cnt)


def match_batch_ref(boxes, scores, bbox, cnt, thr, min_score, max_det, iou=None):
    iou = iou_ref(boxes, bbox) if iou is None else iou
    return [match_ref(iou[b], scores[b], cnt[b], thr, min_score, max_det) for b in range(len(boxes))]


def padded(ms, max_det):
    """the reference's rows in the device's layout: order / score / tp [B, max_det] with dead slots -1 / -inf / 0, n_pred, n_truth [B]"""
    B = len(ms)
    order = np.full((B, max_det), -1, np.int32)
    score = np.full((B, max_det), -np.inf, F)
    tp = np.zeros((B, max_det), np.int32)
    for b, m in enumerate(ms):
        k = len(m["order"])
        order[b, :k], score[b, :k], tp[b, :k] = m["order"], m["score"], m["tp"]
    return dict(order=order, score=score, tp=tp, n_pred=np.array([m["n_pred"] for m in ms], np.int32),
                n_truth=np.array([m["n_truth"] for m in ms], np.int32))


def records_of(ms):
    """(score, tp word) in insertion order: image by image, ranked order inside an image"""
    return [(float(s), int(w)) for m in ms for s, w in zip(m["score"], m["tp"])]


def ap_ref(records, NT, T):
    """-> dict(ap, recall, precision: lists of T floats; tp_total: list of T ints)"""
    recs = sorted(records, key=lambda r: -r[0])                 # Python's sort is stable
    M = len(recs)
    nan = float("nan")
    ap, recall, precision, totals = [], [], [], []
    for t in range(T):
        bits = [(w >> t) & 1 for _, w in recs]
        tp_run, prec = 0, []
        for i, bit in enumerate(bits):
            tp_run += bit
            prec.append(Fraction(tp_run, i + 1))
        env, terms = Fraction(0), []
        for i in range(M - 1, -1, -1):
            if prec[i] > env:
                env = prec[i]
            if bits[i]:
                terms.append(env)
        if NT == 0:
            ap.append(nan)
        elif M <= EXACT_RECORDS:
            ap.append(float(sum(terms, Fraction(0)) / NT))
        else:
            ap.append(math.fsum(float(v) for v in terms) / NT)
        recall.append(tp_run / NT if NT else nan)
        precision.append(tp_run / M if M else nan)
        totals.append(tp_run)
    return dict(ap=ap, recall=recall, precision=precision, tp_total=totals)


def count_ref(n_pred, cnt):
    n_pred, cnt = [int(v) for v in n_pred], [int(v) for v in cnt]
    n = len(cnt)
    if n == 0:
        return dict(count_accuracy=float("nan"), count_mae=float("nan"), count_bias=float("nan"))
    return dict(count_accuracy=float(Fraction(sum(p == c for p, c in zip(n_pred, cnt)), n)),
                count_mae=float(Fraction(sum(abs(p - c) for p, c in zip(n_pred, cnt)), n)),
                count_bias=float(Fraction(sum(p - c for p, c in zip(n_pred, cnt)), n)))


def result_ref(ms, T):
    """what DetectionAP.compute must give for these images in this order"""
    NT = sum(m["n_truth"] for m in ms)
    r = ap_ref(records_of(ms), NT, T)
    r.update(count_ref([m["n_pred"] for m in ms], [m["n_truth"] for m in ms]))
    r.update(n_images=len(ms), n_truth=NT, n_pred=sum(m["n_pred"] for m in ms), n_records=sum(len(m["order"]) for m in ms))
    return r


SCORE_LEVELS = np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.5, 0.625, 0.75, 0.875, 0.9375, 1.0, 1.0], dtype=F)


def make_case(seed, B, N, K, family="quarter", score_levels=SCORE_LEVELS):
    """-> boxes [B,N,4] corners, scores [B,N], bbox [B,K,4] (x, y, w, h; the slots past cnt hold other boxes, not zeros), cnt [B] int64.
    Scores come from a few levels, so ties are the rule; the kinds of prediction are mixed in every image."""
    rng = np.random.default_rng(seed)
    q = lambda lo, hi, size: rng.integers(int(lo * 4), int(hi * 4) + 1, size=size).astype(np.float64) / 4
    x, y = q(0, 400, (B, K)), q(0, 400, (B, K))
    w, h = q(2, 100, (B, K)), q(2, 100, (B, K))
    bbox = np.stack([x, y, w, h], -1)
    cnt = rng.integers(0, K + 1, size=B).astype(np.int64)
    src = rng.integers(0, K, size=(B, N))
    kind = rng.integers(0, 4, size=(B, N))                      # 0 jitter, 1 duplicate, 2 stray, 3 near-miss
    t = np.take_along_axis(bbox, src[..., None], 1)             # [B,N,4]
    x0, y0, x1, y1 = t[..., 0], t[..., 1], t[..., 0] + t[..., 2], t[..., 1] + t[..., 3]
    jit = q(-3, 3, (4, B, N))
    near = np.where(rng.integers(0, 2, size=(B, N)) == 0, t[..., 2], t[..., 3]) / 2
    near = np.floor(near * 4) / 4
    boxes = np.stack([x0, y0, x1, y1], -1)
    j = kind == 0
    for c in range(4):
        boxes[..., c] = np.where(j, boxes[..., c] + jit[c], boxes[..., c])
    m = kind == 3
    boxes[..., 0] = np.where(m, boxes[..., 0] + near, boxes[..., 0])
    boxes[..., 2] = np.where(m, boxes[..., 2] + near, boxes[..., 2])
    sx, sy, sw, sh = q(0, 400, (B, N)), q(0, 400, (B, N)), q(1, 100, (B, N)), q(1, 100, (B, N))
    stray = np.stack([sx, sy, sx + sw, sy + sh], -1)
    boxes = np.where((kind == 2)[..., None], stray, boxes)
    boxes = np.clip(boxes, 0.0, 511.75)
    scores = rng.choice(score_levels, size=(B, N)).astype(F)
    if family == "float":
        boxes = (boxes.astype(F) + rng.normal(0, 1.5, size=boxes.shape).astype(F)).astype(F)
        bbox = (bbox.astype(F) + np.abs(rng.normal(0, 1.5, size=bbox.shape)).astype(F)).astype(F)
        scores = np.where(rng.integers(0, 3, size=(B, N)) == 0, rng.random((B, N)).astype(F), scores).astype(F)
    else:
        assert family == "quarter"
        assert np.array_equal(boxes * 4, np.round(boxes * 4)) and boxes.min() >= 0 and boxes.max() < 512
        assert (bbox[..., 0] + bbox[..., 2]).max() < 512 and (bbox[..., 1] + bbox[..., 3]).max() < 512
    return boxes.astype(F), scores.astype(F), bbox.astype(F), cnt


# ---- cases worked out by hand: (name, boxes [N,4], scores [N], bbox [K,4], cnt, thr, min_score, max_det, expected) ------------------------
# expected: order, tp (lists over the kept predictions), n_pred, and `ap` (a list of exact Fractions per threshold, or None where NT = 0)
A_XYWH, B_XYWH = (10.0, 10.0, 20.0, 20.0), (100.0, 50.0, 40.0, 30.0)
A_BOX, B_BOX = (10.0, 10.0, 30.0, 30.0), (100.0, 50.0, 140.0, 80.0)
STRAY = (300.0, 300.0, 320.0, 330.0)


def hand_cases():
    c = []
    add = lambda name, boxes, scores, bbox, cnt, thr, min_score, max_det, **exp: c.append(dict(
        name=name, boxes=np.array(boxes, F).reshape(-1, 4), scores=np.array(scores, F), bbox=np.array(bbox, F).reshape(-1, 4), cnt=cnt,
        thr=np.array(thr, F), min_score=min_score, max_det=max_det, exp=exp))
    nine = [k / 10 for k in range(1, 10)]
    add("perfect", [A_BOX, B_BOX], [0.9, 0.8], [A_XYWH, B_XYWH], 2, nine, 0.5, 100,
        order=[0, 1], tp=[511, 511], n_pred=2, ap=[Fraction(1)] * 9)
    # the stray ranks first: FP, TP, TP -> prec 0, 1/2, 2/3; the envelope at the two true positives is 2/3, 2/3; AP = (2/3 + 2/3) / 2
    add("stray first", [A_BOX, STRAY, B_BOX], [0.8, 0.95, 0.7], [A_XYWH, B_XYWH], 2, nine, 0.5, 100,
        order=[1, 0, 2], tp=[0, 511, 511], n_pred=3, ap=[Fraction(2, 3)] * 9)
    # two predictions on one truth: the second finds the truth taken and is a false positive; TP, FP -> AP = 1 (recall 1 at precision 1)
    add("double", [A_BOX, A_BOX], [0.9, 0.8], [A_XYWH], 1, [0.5], 0.5, 100, order=[0, 1], tp=[1, 0], n_pred=2, ap=[Fraction(1)])
    # greedy: prediction 0 (score 0.9) overlaps truth 0 with IoU 0.6 and truth 1 not at all; prediction 1 (score 0.8) IS truth 0 (IoU 1)
    # and misses truth 1.  Ranked matching gives truth 0 to prediction 0, and prediction 1 is left with nothing: TP, FP, one truth of two
    # found.  A best-per-truth rule (metric.mAP's) would credit truth 0 with IoU 1 from prediction 1 and never see the false positive.
    add("greedy", [(0, 0, 10, 6), (0, 0, 10, 10)], [0.9, 0.8], [(0, 0, 10, 10), (200, 200, 10, 10)], 2, [0.5], 0.5, 100,
        order=[0, 1], tp=[1, 0], n_pred=2, ap=[Fraction(1, 2)])
    # IoU exactly 0.5: inter 2, union 4 + 2 - 2 = 4
    add("iou on the threshold", [(0, 0, 2, 2)], [0.9], [(0, 0, 2, 1)], 1, [0.5, 0.75], 0.5, 100, order=[0], tp=[1], n_pred=1,
        ap=[Fraction(1), Fraction(0)])
    # equal scores rank by index; two identical truths: the lower j goes first, so both predictions are true positives
    add("ties", [B_BOX, A_BOX, A_BOX], [0.7, 0.7, 0.7], [A_XYWH, A_XYWH, B_XYWH], 3, [0.5], 0.5, 100,
        order=[0, 1, 2], tp=[1, 1, 1], n_pred=3, ap=[Fraction(1)])
    add("zero area", [(10, 10, 10, 30), (10, 10, 30, 30)], [0.9, 0.8], [A_XYWH], 1, [0.1], 0.5, 100, order=[0, 1], tp=[0, 1], n_pred=2,
        ap=[Fraction(1, 2)])
    add("no truth", [A_BOX], [0.9], [A_XYWH], 0, [0.5], 0.5, 100, order=[0], tp=[0], n_pred=1, ap=None)
    add("no record", [A_BOX], [0.2], [A_XYWH], 1, [0.5], 0.5, 100, order=[], tp=[], n_pred=0, ap=[Fraction(0)])
    # max_det = 2 cuts the third-ranked prediction (which alone fits truth B); n_pred stays 3
    add("max_det", [A_BOX, STRAY, B_BOX], [0.9, 0.8, 0.7], [A_XYWH, B_XYWH], 2, [0.5], 0.5, 2, order=[0, 1], tp=[1, 0], n_pred=3,
        ap=[Fraction(1, 2)])
    add("nan score is dead, min_score is live", [A_BOX, B_BOX, STRAY], [float("nan"), 0.5, 0.4999], [A_XYWH, B_XYWH], 2, [0.5], 0.5, 100,
        order=[1], tp=[1], n_pred=1, ap=[Fraction(1, 2)])
    return c
