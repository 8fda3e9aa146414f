"""Detection metrics without a GPU: the references of detection_helpers.py on cases worked out by hand, what the two entry points refuse
before any launch, and the public surface."""
import ctypes
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import detection_helpers as dh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE = -1
F = np.float32


# ---- the references against hand-worked cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dh.hand_cases(), ids=lambda c: c["name"])
def test_references_by_hand(case):
    m = dh.match_ref(dh.iou_ref(case["boxes"], case["bbox"]), case["scores"], case["cnt"], case["thr"], case["min_score"], case["max_det"])
    exp = case["exp"]
    assert m["order"] == exp["order"] and m["tp"] == exp["tp"] and m["n_pred"] == exp["n_pred"] and m["n_truth"] == case["cnt"]
    r = dh.ap_ref(dh.records_of([m]), m["n_truth"], len(case["thr"]))
    if exp["ap"] is None:
        assert all(math.isnan(v) for v in r["ap"]) and all(math.isnan(v) for v in r["recall"])
    else:
        assert r["ap"] == [float(v) for v in exp["ap"]]


def test_stray_first_curve_by_hand():
    # FP, TP, TP: prec 0, 1/2, 2/3 -- recall 1 and precision 2/3 at the end of the curve, AP = 2/3 exactly
    r = dh.ap_ref([(0.95, 0), (0.8, 1), (0.7, 1)], 2, 1)
    assert r["ap"] == [float(Fraction(2, 3))] and r["recall"] == [1.0] and r["precision"] == [2 / 3] and r["tp_total"] == [2]
    # the pooled sort is stable: equal scores keep their insertion order, which here decides the curve (TP first: AP 1, FP first: 1/2)
    assert dh.ap_ref([(0.5, 1), (0.5, 0)], 1, 1)["ap"] == [1.0] and dh.ap_ref([(0.5, 0), (0.5, 1)], 1, 1)["ap"] == [0.5]
    # no record at all
    r = dh.ap_ref([], 3, 2)
    assert r["ap"] == [0.0, 0.0] and r["recall"] == [0.0, 0.0] and all(math.isnan(v) for v in r["precision"])
    # the exact path and the fsum path agree where both apply
    rng = np.random.default_rng(5)
    recs = [(float(s), int(w)) for s, w in zip(rng.choice(dh.SCORE_LEVELS, 3000), rng.integers(0, 4, 3000))]
    big = dh.ap_ref(recs, 2500, 2)
    old, dh.EXACT_RECORDS = dh.EXACT_RECORDS, 10 ** 9
    try:
        exact = dh.ap_ref(recs, 2500, 2)
    finally:
        dh.EXACT_RECORDS = old
    assert max(abs(a - b) for a, b in zip(big["ap"], exact["ap"])) <= 2e-16


def test_iou_ref_by_hand():
    iou = dh.iou_ref([(0, 0, 2, 2), (0, 0, 2, 2), (5, 5, 5, 9), (float("nan"), 0, 2, 2), (0, 0, float("inf"), 2), (3, 3, 1, 1)],
                     [(0, 0, 2, 1), (2, 0, 2, 2), (0, 0, 2, 2)])
    assert iou.dtype == F and iou.shape == (6, 3)
    assert iou[0].tolist() == [0.5, 0.0, 1.0]             # half, touching edges, identical
    assert not iou[2:].any() and not np.signbit(iou).any()  # zero area, NaN, infinite, inverted: +0
    assert dh.iou_ref([(0, 0, 3, 1)], [(0, 0, 1, 1)])[0, 0] == F(1) / F(3)


def test_match_ref_ranking_rules():
    iou = np.zeros((4, 1), F)
    m = dh.match_ref(iou, [0.5, -0.0, 0.0, 0.7], 1, [0.5], -1.0, 3)
    assert m["order"] == [3, 0, 1] and m["n_pred"] == 4      # -0 and +0 are equal: index order; max_det cuts the tail
    assert dh.match_ref(iou, [0.5, 0.5, 0.5, 0.5], 9, [0.5], 0.5, 100)["n_truth"] == 1        # the count is clamped to K


def test_count_ref_table():
    r = dh.count_ref([3, 0, 5, 2, 2], [3, 1, 2, 2, 4])      # differences 0, -1, 3, 0, -2
    assert r == dict(count_accuracy=0.4, count_mae=1.2, count_bias=0.0)
    assert all(math.isnan(v) for v in dh.count_ref([], []).values())


def test_generator_families():
    for fam in ("quarter", "float"):
        boxes, scores, bbox, cnt = dh.make_case(3, 4, 50, 7, fam)
        assert boxes.shape == (4, 50, 4) and scores.shape == (4, 50) and bbox.shape == (4, 7, 4) and cnt.shape == (4,)
        assert boxes.dtype == F and bbox.dtype == F and scores.dtype == F
        iou = dh.iou_ref(boxes, bbox)
        assert (iou > 0.5).any() and (iou == 0).any() and iou.max() <= 1
    boxes, scores, bbox, cnt = dh.make_case(3, 4, 50, 7, "quarter")
    assert (dh.iou_ref(boxes, bbox) == 1).any()           # exact duplicates of a truth


# ---- refusals, before any launch (the non-NULL pointers are never read) ----------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def vp(a):
    return ctypes.c_void_p(a) if a else None


MATCH_PTRS = ("boxes", "scores", "bbox", "count", "thresholds", "score", "tp", "order", "n_pred", "n_truth", "counters")


def match_call(lib, B=2, N=16, K=3, T=9, min_score=0.5, max_det=8, iou=64, **ptrs):
    p = {k: 64 for k in MATCH_PTRS}
    p.update(ptrs)
    return lib.spair_det_match(vp(p["boxes"]), vp(p["scores"]), vp(p["bbox"]), vp(p["count"]), vp(p["thresholds"]), B, N, K, T, min_score,
                               max_det, vp(p["score"]), vp(p["tp"]), vp(p["order"]), vp(p["n_pred"]), vp(p["n_truth"]), vp(p["counters"]),
                               vp(iou), None)


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(N=0), dict(N=1025), dict(K=0), dict(K=33), dict(T=0), dict(T=17), dict(max_det=0),
                                dict(max_det=17), dict(max_det=-3), dict(min_score=float("nan")), dict(min_score=float("inf")),
                                dict(min_score=float("-inf"))] + [{k: 0} for k in MATCH_PTRS] + [dict(boxes=0, iou=0)])
def test_det_match_refusals(lib, kw):
    assert match_call(lib, **kw) == ERR_SHAPE


def ap_call(lib, tp=64, M=100, T=9, counters=64, out=64):
    return lib.spair_det_ap(vp(tp), M, T, vp(counters), vp(out), None)


@pytest.mark.parametrize("kw", [dict(M=0), dict(M=-1), dict(M=2 ** 31), dict(M=2 ** 40), dict(T=0), dict(T=17), dict(tp=0), dict(counters=0),
                                dict(out=0)])
def test_det_ap_refusals(lib, kw):
    assert ap_call(lib, **kw) == ERR_SHAPE


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_surface():
    import torch
    import spair_pytorch_amd as sp
    from spair_pytorch_amd import _lib, detection
    names = ("DetectionAP", "DetectionBatch", "DetectionResult", "detection_ap")
    for n in names:
        assert getattr(sp, n) is getattr(detection, n) and n in sp.__all__
    assert sp.__all__.index("DetectionAP") > sp.__all__.index("SegmentationResult")        # appended
    sig = inspect.signature(detection.DetectionAP.__init__)
    assert list(sig.parameters) == ["self", "thresholds", "min_score", "max_det", "capacity", "device"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [None, 0.5, 100, 1024, None]
    assert list(inspect.signature(detection.DetectionAP.update).parameters) == ["self", "pred", "bbox", "count", "scores"]
    assert inspect.signature(detection.DetectionAP.update).parameters["scores"].default is None
    sig = inspect.signature(detection.detection_ap)
    assert list(sig.parameters) == ["pred", "bbox", "count", "scores", "kw"] and sig.parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
    for m in ("compute", "reset", "merge"):
        assert callable(getattr(detection.DetectionAP, m))
    assert detection.DetectionBatch.__slots__ == ("order", "score", "tp", "n_pred", "n_truth")
    for k in ("ap", "mean_ap", "recall", "precision", "thresholds", "n_images", "n_truth", "n_pred", "count_accuracy", "count_mae", "count_bias"):
        assert k in detection.DetectionResult.__slots__
    acc = detection.DetectionAP()
    assert acc.thresholds_host == tuple(torch.arange(0.1, 1.0, 0.1).tolist()) and len(acc.thresholds_host) == 9
    assert np.array_equal(np.array(acc.thresholds_host, F), dh.default_thresholds())
    for doc in (detection.DetectionAP.__doc__, detection.__doc__):
        for word in ("corner", "mAP", "object_count_accuracy", "top-left", "reference"):
            assert word in doc, word
    for word in ("ParseResult", "z_pres", "synchronisation", "GPU only", "DetectionBatch"):
        assert word in detection.DetectionAP.update.__doc__, word
    for bad in (dict(thresholds=[]), dict(thresholds=[0.5] * 17), dict(max_det=0), dict(min_score=float("nan")), dict(min_score=float("inf"))):
        with pytest.raises(_lib.SpairHipError):
            detection.DetectionAP(**bad)
    header = open(os.path.join(ROOT, "include", "spair_hip.h")).read()
    source = open(_lib.__file__).read()
    for fn in ("spair_det_match", "spair_det_ap"):
        assert "int %s(" % fn in header and "h.%s.argtypes" % fn in source
    assert "detection metrics" in header and "#define SPAIR_DET_COUNTERS %d" % detection.COUNTERS in header
    assert "#define SPAIR_ABI_VERSION 3" in header and _lib.ABI_VERSION == 3
    assert os.path.exists(os.path.join(ROOT, "spair_pytorch_amd", "csrc", "detection.hip"))
    if os.path.exists(_lib.LIB_PATH):
        h = _lib.lib()
        assert hasattr(h, "spair_det_match") and hasattr(h, "spair_det_ap") and h.spair_abi_version() == 3


def test_cpu_tensors_are_refused_not_scored():
    import torch
    from spair_pytorch_amd import _lib, detection
    boxes, scores, bbox, cnt = torch.zeros(1, 4, 4), torch.zeros(1, 4), torch.zeros(1, 2, 4), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(_lib.SpairHipError, match="GPU"):
        detection.DetectionAP().update(boxes, bbox, cnt, scores)
    with pytest.raises(_lib.SpairHipError, match="GPU"):
        detection.detection_ap(boxes, bbox, cnt, scores)
    with pytest.raises(_lib.SpairHipError, match="GPU"):
        detection.DetectionAP(device="cpu")
