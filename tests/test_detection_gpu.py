"""The device detection metrics on the MI355X against detection_helpers.py.

IoU: bit-equal to the numpy float32 restatement (every operation rounds once on both sides; on the quarter-pixel family only the
division rounds at all).  Matching: integers and scores exactly equal to match_ref fed with iou_ref's matrix.  Curve: every count exact;
ap, recall and precision within CURVE_TOL = 1e-12 absolute of ap_ref -- the device sums at most NT float64 terms of at most 1 each and
divides by NT, one rounding apiece: NT * 2^-53 = 1.1e-16 * NT relative to a result in [0, 1], far below 1e-12 for the NT <= 4480 used
here (the reference itself is exact or within 1.2e-16).  Shapes are the smallest that reach every path of the two kernels."""
import math

import numpy as np
import pytest
import torch

import detection_helpers as dh

pytestmark = pytest.mark.gpu

CURVE_TOL = 1e-12
F = np.float32


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def device_match(boxes, scores, bbox, cnt, thr, min_score, max_det):
    from spair_pytorch_amd import detection
    batch, iou, counters = detection.match_iou(dev(boxes), dev(scores), dev(bbox), dev(cnt), thr, min_score, max_det)
    return batch, iou, counters.cpu().numpy()


def check_batch(batch, ref, what):
    for k in ("order", "tp", "n_pred", "n_truth"):
        got = getattr(batch, k).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, ref[k]), (what, k, got, ref[k])
    got = batch.score.cpu().numpy()
    assert np.array_equal(got.view(np.int32), ref["score"].view(np.int32)), (what, "score")


def check_counters(c, ms, T, what):
    n_pred, cnt = [m["n_pred"] for m in ms], [m["n_truth"] for m in ms]
    exp = [sum(cnt), sum(len(m["order"]) for m in ms), sum(p == q for p, q in zip(n_pred, cnt)), sum(abs(p - q) for p, q in zip(n_pred, cnt)),
           sum(p - q for p, q in zip(n_pred, cnt)), len(ms), 0, 0]
    exp += [sum((w >> t) & 1 for m in ms for w in m["tp"]) for t in range(T)] + [0] * (16 - T)
    assert c.tolist() == exp, (what, c.tolist(), exp)


# ---- 1. the IoU output ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("quarter", "float"))
def test_iou_bit_equal(family):
    boxes, scores, bbox, cnt = dh.make_case(11, 3, 257, 11, family)
    # degenerate and non-finite boxes on both sides
    boxes[0, 0] = (5, 5, 5, 9)
    boxes[0, 1] = (9, 9, 3, 3)
    boxes[0, 2] = (np.nan, 0, 50, 50)
    boxes[0, 3] = (0, 0, np.inf, 50)
    boxes[0, 4] = (0, 0, 3e38, 3e38)
    boxes[1, 0] = (-np.inf, 0, 50, 50)
    bbox[1, 0] = (np.nan, 0, 50, 50)
    bbox[1, 1] = (0, 0, 0, 0)
    bbox[1, 2] = (0, 0, np.inf, 4)
    bbox[2, 0] = bbox[2, 1]
    boxes[2, 5] = (bbox[2, 1, 0], bbox[2, 1, 1], bbox[2, 1, 0] + bbox[2, 1, 2], bbox[2, 1, 1] + bbox[2, 1, 3])
    ref = dh.iou_ref(boxes, bbox)
    _, iou, _ = device_match(boxes, scores, bbox, cnt, dh.default_thresholds(), 0.5, 100)
    got = iou.cpu().numpy()
    differ = got.view(np.int32) != ref.view(np.int32)
    print("%s: %d of %d differ; IoU > 0 on %d, == 1 on %d" % (family, int(differ.sum()), differ.size, int((ref > 0).sum()), int((ref == 1).sum())))
    assert not differ.any()
    assert (ref > 0).sum() > 500 and (ref == 1).any() and not ref[0, :5].any() and not ref[1, :, :3].any()


# ---- 2. matching: shapes ---------------------------------------------------------------------------------------------------------------------
NS = (1, 9, 63, 64, 65, 256, 1000, 1024)
#          K   T   B  max_det   min_score
CONFIGS = ((1, 1, 3, "one", 0.5), (11, 8, 5, "half", 0.0), (32, 9, 1, "all", 0.0), (32, 16, 3, "all", 0.5), (11, 16, 1, "half", 0.0),
           (1, 9, 5, "all", 0.0), (32, 1, 3, "one", 0.0), (11, 8, 1, "half", 0.5))


@pytest.mark.parametrize("config", range(len(CONFIGS)))
@pytest.mark.parametrize("N", NS)
def test_matching_shapes(N, config):
    K, T, B, md, min_score = CONFIGS[config]
    max_det = dict(one=1, half=max(N // 2, 1), all=N)[md]
    thr = np.linspace(0.05, 0.95, T).astype(F) if T != 9 else dh.default_thresholds()
    boxes, scores, bbox, cnt = dh.make_case(1000 * config + N, B, N, K, "quarter" if config % 2 == 0 else "float")
    ms = dh.match_batch_ref(boxes, scores, bbox, cnt, thr, min_score, max_det)
    batch, _, counters = device_match(boxes, scores, bbox, cnt, thr, min_score, max_det)
    what = "N=%d K=%d T=%d B=%d max_det=%d min_score=%g" % (N, K, T, B, max_det, min_score)
    assert batch.order.shape == (B, max_det)
    check_batch(batch, dh.padded(ms, max_det), what)
    check_counters(counters, ms, T, what)
    if min_score == 0.0:
        assert all(m["n_pred"] == N for m in ms)                     # every cell live


# ---- 3. matching: planted cases inside one batch ---------------------------------------------------------------------------------------------
def planted_batch():
    N, K = 70, 6
    boxes, scores, bbox, cnt = dh.make_case(77, 12, N, K, "quarter")
    scores[0] = 0.75                                                 # all scores equal: index order
    scores[1] = np.where(np.arange(N) % 3 == 0, 1.0, 0.0)           # hard presence
    cnt[2], cnt[3] = 0, K
    scores[4], cnt[4] = 0.125, 3                                     # no live prediction
    scores[5], cnt[5] = 0.25, 0                                      # both sides empty
    bbox[6, 1] = bbox[6, 0]                                          # duplicate truths, and two predictions that are exactly them
    scores[6] = np.minimum(scores[6], F(0.9375))
    for n in (3, 40):
        boxes[6, n] = (bbox[6, 0, 0], bbox[6, 0, 1], bbox[6, 0, 0] + bbox[6, 0, 2], bbox[6, 0, 1] + bbox[6, 0, 3])
        scores[6, n] = 1.0
    cnt[6] = K
    bbox[7, 0], boxes[7, 0], scores[7, 0], cnt[7] = (0, 0, 2, 1), (0, 0, 2, 2), 1.0, 1      # IoU exactly 0.5 = a threshold
    boxes[7, 1:] = (300, 300, 310, 310)
    scores[8, :5] = (np.nan, 0.5, -0.0, np.inf, 0.4999)
    cnt[9] = K + 7                                                   # clamped to K
    cnt[10] = -2                                                     # clamped to 0
    return boxes, scores, bbox, cnt


def test_matching_planted_cases():
    boxes, scores, bbox, cnt = planted_batch()
    thr = np.array([0.25, 0.5, 0.75, 1.0], F)
    ms = dh.match_batch_ref(boxes, scores, bbox, cnt, thr, 0.5, 100)
    batch, _, counters = device_match(boxes, scores, bbox, cnt, thr, 0.5, 100)
    check_batch(batch, dh.padded(ms, 70), "planted")
    check_counters(counters, ms, 4, "planted")
    order, tp, n_pred, n_truth = (getattr(batch, k).cpu().numpy() for k in ("order", "tp", "n_pred", "n_truth"))
    assert order[0].tolist() == list(range(70)) and n_pred[0] == 70
    assert order[1, :24].tolist() == list(range(0, 70, 3)) and n_pred[1] == 24
    assert n_truth[[2, 3, 9, 10]].tolist() == [0, 6, 6, 0] and not tp[2].any() and not tp[10].any()
    assert n_pred[4] == 0 and (order[4] == -1).all() and n_pred[5] == 0 and n_truth[5] == 0
    assert order[6, :2].tolist() == [3, 40] and tp[6, :2].tolist() == [15, 15]              # both duplicates matched, at IoU 1
    assert order[7, 0] == 0 and tp[7, 0] == 0b0011                                             # 0.5 >= 0.5, not >= 0.75
    assert order[8, 0] == 3 and 0 not in order[8] and 2 not in order[8] and 4 not in order[8] and 1 in order[8]


@pytest.mark.parametrize("case", dh.hand_cases(), ids=lambda c: c["name"])
def test_matching_hand_cases(case):
    from spair_pytorch_amd import detection
    exp = case["exp"]
    args = (case["boxes"][None], case["scores"][None], case["bbox"][None], np.array([case["cnt"]], np.int64))
    batch, _, _ = device_match(*args, case["thr"], case["min_score"], case["max_det"])
    k = len(exp["order"])
    assert batch.order[0, :k].tolist() == exp["order"] and batch.tp[0, :k].tolist() == exp["tp"] and int(batch.n_pred[0]) == exp["n_pred"]
    assert (batch.order[0, k:] == -1).all()
    r = detection.detection_ap(dev(args[0]), dev(args[2]), dev(args[3]), dev(args[1]), thresholds=case["thr"], min_score=case["min_score"],
                               max_det=case["max_det"])
    if exp["ap"] is None:
        assert torch.isnan(r.ap).all() and torch.isnan(r.mean_ap)
    else:
        assert r.ap.tolist() == [float(v) for v in exp["ap"]]
        assert abs(float(r.mean_ap) - float(sum(exp["ap"]) / len(exp["ap"]))) <= 1e-15


# ---- 4. the pooled curve -----------------------------------------------------------------------------------------------------------------------
def check_result(r, ref, what):
    for k in ("n_images", "n_truth", "n_pred", "n_records"):
        assert getattr(r, k).dtype == torch.int64 and int(getattr(r, k)) == ref[k], (what, k, int(getattr(r, k)), ref[k])
    worst = 0.0
    for k in ("ap", "recall", "precision"):
        got = getattr(r, k).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (len(ref[k]),)
        for g, e in zip(got.tolist(), ref[k]):
            assert math.isnan(g) == math.isnan(e), (what, k, g, e)
            if not math.isnan(e):
                worst = max(worst, abs(g - e))
    for k in ("count_accuracy", "count_mae", "count_bias"):
        g, e = float(getattr(r, k)), ref[k]
        assert (math.isnan(g) and math.isnan(e)) or g == e, (what, k, g, e)
    m = float(r.mean_ap)
    e = sum(ref["ap"]) / len(ref["ap"])
    assert (math.isnan(m) and math.isnan(e)) or abs(m - e) <= CURVE_TOL
    print("%s: %d records, NT %d: worst |ap, recall, precision - reference| = %.3g" % (what, ref["n_records"], ref["n_truth"], worst))
    assert worst <= CURVE_TOL, (what, worst)


def feed(acc, case, chunks):
    boxes, scores, bbox, cnt = case
    lo = 0
    for n in chunks:
        acc.update(dev(boxes[lo:lo + n]), dev(bbox[lo:lo + n]), dev(cnt[lo:lo + n]), dev(scores[lo:lo + n]))
        lo += n


#                       records: B x N        K
CURVE_SHAPES = {1: (1, 1, 1), 255: (5, 51, 4), 256: (4, 64, 7), 257: (1, 257, 32), 1023: (3, 341, 11), 1025: (5, 205, 32),
                4097: (17, 241, 32), 70000: (140, 500, 32)}


@pytest.mark.parametrize("records", sorted(CURVE_SHAPES))
def test_curve_against_reference(records):
    from spair_pytorch_amd import detection
    B, N, K = CURVE_SHAPES[records]
    T = 2 if records > 5000 else 3
    thr = np.array([0.3, 0.6, 0.9][:T], F)
    case = dh.make_case(records, B, N, K, "quarter")
    if records == 1:
        case[3][:] = 1
    acc = detection.DetectionAP(thresholds=thr, min_score=0.0, max_det=N, capacity=2, device="cuda")
    chunks = [1] * min(B, 3) + ([B - 3] if B > 3 else [])
    assert sum(chunks) == B
    feed(acc, case, chunks)
    r = acc.compute()
    ms = dh.match_batch_ref(*case, thr, 0.0, N)
    ref = dh.result_ref(ms, T)
    assert ref["n_records"] == records and acc.n_images == B
    check_result(r, ref, "%d records" % records)


@pytest.mark.parametrize("kind", ("runs of equal scores", "all true positives", "all false positives", "no truth", "no record", "nothing fed"))
def test_curve_planted(kind):
    from spair_pytorch_amd import detection
    B, N, K, thr = 9, 40, 8, np.array([0.5, 0.75], F)
    boxes, scores, bbox, cnt = dh.make_case(5, B, N, K, "quarter")
    min_score = 0.0
    if kind == "runs of equal scores":
        scores[:] = np.where(np.arange(N) % 2 == 0, 0.75, 0.25)[None]         # two long runs across all images: the stable order decides
    elif kind == "all true positives":
        N = K
        corners = np.concatenate([bbox[..., :2], bbox[..., :2] + bbox[..., 2:]], -1)
        boxes, scores, cnt = corners.astype(F), scores[:, :K], np.full(B, K, np.int64)
    elif kind == "all false positives":
        boxes[..., 0::2] = 480 + boxes[..., 0::2] / 32
        bbox[..., 0] = np.minimum(bbox[..., 0], 300)
        bbox[..., 2] = np.minimum(bbox[..., 2], 100)
        cnt[:] = np.maximum(cnt, 1)
    elif kind == "no truth":
        cnt[:] = 0
    elif kind == "no record":
        min_score, cnt[0] = 2.0, 3
    acc = detection.DetectionAP(thresholds=thr, min_score=min_score, max_det=N, capacity=4, device="cuda")
    if kind == "nothing fed":
        ms = []
    else:
        feed(acc, (boxes, scores, bbox, cnt), [4, 5])
        ms = dh.match_batch_ref(boxes, scores, bbox, cnt, thr, min_score, N)
    ref = dh.result_ref(ms, 2)
    r = acc.compute()
    check_result(r, ref, kind)
    if kind == "all true positives":
        assert r.ap.tolist() == [1.0, 1.0] and r.recall.tolist() == [1.0, 1.0] and float(r.count_accuracy) == 1.0
    if kind == "all false positives":
        assert r.ap.tolist() == [0.0, 0.0] and r.precision.tolist() == [0.0, 0.0]
    if kind in ("no truth", "nothing fed"):
        assert torch.isnan(r.ap).all() and torch.isnan(r.mean_ap)
    if kind == "no record":
        assert r.ap.tolist() == [0.0, 0.0] and int(r.n_records) == 0


# ---- 5. the accumulator ------------------------------------------------------------------------------------------------------------------------
def result_bits(r):
    return {k: getattr(r, k).cpu().numpy().tobytes() for k in r.__slots__}


def test_accumulator():
    from spair_pytorch_amd import _lib, detection
    thr = dh.default_thresholds()
    case = dh.make_case(21, 7, 64, 11, "float")
    ms = dh.match_batch_ref(*case, thr, 0.5, 20)
    kw = dict(min_score=0.5, max_det=20, capacity=2, device="cuda")
    a = detection.DetectionAP(**kw)
    assert a.thresholds_host == tuple(thr.tolist())
    feed(a, case, [1, 2])                                        # differing B; growth from capacity 2 ...
    first = a.compute()
    check_result(first, dh.result_ref(ms[:3], 9), "three images")
    feed(a, tuple(v[3:] for v in case), [3, 1])                  # ... through 7 images, with a compute in between
    assert a.capacity == 8 and a.n_images == 7
    whole = a.compute()
    check_result(whole, dh.result_ref(ms, 9), "seven images")
    assert result_bits(a.compute()) == result_bits(whole)        # compute changes nothing
    # a second complete run is bit-identical in every output
    b = detection.DetectionAP(**kw)
    batches = []
    lo = 0
    for n in (1, 2, 3, 1):
        batches.append(b.update(*(dev(case[i][lo:lo + n]) for i in (0, 2, 3, 1))))
        lo += n
    assert result_bits(b.compute()) == result_bits(whole)
    for k in ("score", "tp", "order", "n_pred", "n_truth"):
        assert torch.equal(torch.cat([getattr(x, k) for x in batches]).view(torch.int32), a._bufs[("score", "tp", "order", "n_pred", "n_truth").index(k)][:7].view(torch.int32))
    # the batch views are the reference's rows
    check_batch(batches[2], dh.padded(ms[3:6], 20), "third update")
    # merge = sequential feeding
    c, d = detection.DetectionAP(**kw), detection.DetectionAP(**kw)
    feed(c, tuple(v[:3] for v in case), [3])
    feed(d, tuple(v[3:] for v in case), [2, 2])
    assert c.merge(d) is c and c.n_images == 7 and d.n_images == 4
    assert result_bits(c.compute()) == result_bits(whole)
    with pytest.raises(_lib.SpairHipError, match="differ"):
        c.merge(detection.DetectionAP(min_score=0.25, max_det=20, device="cuda"))
    # reset
    c.reset()
    assert c.n_images == 0 and torch.isnan(c.compute().mean_ap) and int(c.compute().n_images) == 0
    feed(c, case, [7])
    assert result_bits(c.compute()) == result_bits(whole)
    # detection_ap = one update and one compute
    one = detection.detection_ap(dev(case[0]), dev(case[2]), dev(case[3]), dev(case[1]), min_score=0.5, max_det=20)
    assert result_bits(one) == result_bits(whole)
    # float counts are rounded, not truncated
    e = detection.DetectionAP(**kw)
    e.update(dev(case[0]), dev(case[2]), dev(case[3].astype(F) + F(0.25)), dev(case[1]))
    assert result_bits(e.compute()) == result_bits(whole)


# ---- 6. end to end: a parse scored against the generator's boxes -------------------------------------------------------------------------------
@pytest.fixture
def cfg():
    from spair_pytorch_amd import config as cfg
    old = (list(cfg.INPUT_IMAGE_SHAPE), [t["stride"] for t in cfg.DEFAULT_BACKBONE_TOPOLOGY])
    yield cfg
    cfg.INPUT_IMAGE_SHAPE[:] = old[0]
    for t, s in zip(cfg.DEFAULT_BACKBONE_TOPOLOGY, old[1]):
        t["stride"] = s


def test_parse_scored_against_the_boxes(cfg):
    from spair_pytorch_amd import DetectionAP, metric
    from spair_pytorch_amd.data import DeviceScatteredDigits
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(3)
    m = SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype="f32").to("cuda")
    ds = DeviceScatteredDigits(64, 8, image_side=48, max_objects=5, seed=2, obj_px=(10, 20))
    x, bbox, cnt = ds.batch(1)
    parse = m.parse(x, 2000, threshold=0.02)
    before = metric.mAP(parse.z_where, parse.z_pres, bbox, cnt, image_side=48).clone()
    status = m.step_status()
    torch.manual_seed(9)
    cpu_state, gpu_state = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    for min_score in (0.5, 0.0):
        acc = DetectionAP(min_score=min_score)
        batch = acc.update(parse, bbox, cnt)
        r = acc.compute()
        boxes, scores = parse.boxes.cpu().numpy(), parse.z_pres.reshape(8, -1).cpu().numpy()
        assert boxes.shape == (8, 36, 4)
        ms = dh.match_batch_ref(boxes, scores, bbox.cpu().numpy(), cnt.cpu().numpy(), dh.default_thresholds(), min_score, 36)
        check_batch(batch, dh.padded(ms, 36), "parse, min_score %g" % min_score)
        check_result(r, dh.result_ref(ms, 9), "parse, min_score %g" % min_score)
        print("min_score %g: mean AP %.4f, count accuracy %.3f" % (min_score, float(r.mean_ap), float(r.count_accuracy)))
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), gpu_state)
    assert m.step_status() == status
    after = metric.mAP(parse.z_where, parse.z_pres, bbox, cnt, image_side=48)
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))


# ---- 7. no host synchronisation ------------------------------------------------------------------------------------------------------------------
def test_no_synchronisation():
    from spair_pytorch_amd import detection
    case = dh.make_case(31, 6, 100, 11, "quarter")
    args = [dev(case[i]) for i in (0, 2, 3, 1)]
    acc = detection.DetectionAP(capacity=4, device="cuda")
    acc.update(*args)                                            # (the library is loaded and the kernels' code objects are resident)
    acc.compute()
    acc.reset()
    other = detection.DetectionAP(capacity=4, device="cuda")    # (its thresholds are uploaded here: the one host-to-device copy)
    probe = torch.ones(4, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.sum().item()
            works = False
        except RuntimeError:
            works = True
        if works:
            acc.update(*args)
            acc.update(*args)                                    # grows the buffers
            r = acc.compute()
            other.update(*args)
            acc.merge(other)
            r2 = acc.compute()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not works:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this build")
    assert acc.n_images == 18 and int(r.n_images) == 12 and int(r2.n_images) == 18
    ms = dh.match_batch_ref(*case, dh.default_thresholds(), 0.5, 100)
    check_result(r2, dh.result_ref(ms * 3, 9), "three times the batch")
