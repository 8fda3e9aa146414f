"""Instance masks and segmentation metrics without a GPU: the per-glyph restatement of the scene oracle, the share of pixels the mask
comparison leaves out, segmentation_ref on examples worked out by hand, what the two entry points refuse before any launch, and the
public surface."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import segmentation_helpers as sh
from oracle import scenes_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE = 0, -1


@pytest.fixture(scope="module")
def planes():
    return {c: sh.scene_planes(c[3], c[4], c[0], c[1], c[2], c[5], c[6]) for c in sh.SCENE_CASES}


@pytest.mark.parametrize("case", sh.SCENE_CASES)
def test_scene_planes_restate_the_oracle(planes, case):
    B, I, K, seed, first, smin, smax = case
    img, bbox, count, pl = planes[case]
    ri, rb, rc = so.generate(seed, first, B, I, K, smin, smax)
    assert img.dtype == np.float32 and np.array_equal(img, ri)            # bit for bit
    assert np.array_equal(bbox, rb) and np.array_equal(count, rc)
    assert pl.shape == (B, K, I, I) and not pl[np.arange(K)[None, :] >= count[:, None]].any()


@pytest.mark.parametrize("case", sh.SCENE_CASES)
def test_left_out_share_on_the_reference_alone(planes, case):
    img, bbox, count, pl = planes[case]
    mask, left, stats = sh.mask_rule(pl)
    print("case %s: left out %d of %d pixels, %s" % (case, int(left.sum()), left.size, stats))
    assert left.mean() <= sh.LEFT_OUT_CAP
    assert np.array_equal(mask >= 0, img[:, 0] > 0) and (mask < count[:, None, None]).all()
    # the cases keep what they are there for: overlapping glyphs, and exact ties at the saturated value for the lowest-index rule
    assert stats["overlap"] > 0
    if case in (sh.SCENE_CASES[0], sh.SCENE_CASES[3]):
        assert stats["saturated_ties"] > 0
    if case == sh.SCENE_CASES[4]:
        assert count.tolist() == [13, 15, 10, 4, 4]


def test_mask_rule_by_hand():
    p = np.zeros((1, 3, 1, 8), np.float32)
    p[0, 0, 0] = [0, 0.5, 1.0, 1.0, 0.3, 0.3, 5e-6, 0.7]
    p[0, 1, 0] = [0, 0.2, 1.0, 0.4, 0.3, 0.3 + 2e-6, 0, 0]
    p[0, 2, 0] = [0, 0.0, 1.0, 1.0, 0.1, 0.0, 0, 0.7 - 1e-4]
    mask, left, stats = sh.mask_rule(p)
    assert mask[0, 0].tolist() == [-1, 0, 0, 0, 0, 1, 0, 0]
    #                        nothing, clear, 3-way tie at 1, tie at 1, soft tie, close, faint, clear by 1e-4
    assert left[0, 0].tolist() == [False, False, False, False, True, True, True, False]


def ref1(pred, truth, NP, K):
    r = sh.segmentation_ref(np.asarray(pred)[None, None, :], np.asarray(truth)[None, None, :], NP, K)
    return r, r["scores"][0]


def test_segmentation_ref_ari_by_hand():
    # n = {(0,0): 2, (1,1): 1, (2,1): 1}: X = 1, A = 1, Bs = 2, C = 6 -> E = 1/3, M = 3/2 -> (2/3) / (7/6) = 4/7
    _, s = ref1([0, 0, 1, 2], [0, 0, 1, 1], 3, 2)
    assert abs(s[0] - 0.5714285714) < 1e-10 and s[0] == 4 / 7
    # every pair split the other way: X = 0, A = Bs = 2, C = 6 -> E = 2/3, M = 2 -> (-2/3) / (4/3)
    _, s = ref1([0, 0, 1, 1], [0, 1, 0, 1], 2, 2)
    assert s[0] == -0.5
    # a relabelled identical partition (background is one more cluster)
    _, s = ref1([2, 2, 0, 0, 1, -1], [0, 0, 1, 1, 2, -1], 3, 3)
    assert s[0] == 1.0 and s[1] == 1.0 and s[2] == 1.0 and s[3] == 1.0
    # a single pixel: C2(N) = 0
    for p, t in ((0, 0), (-1, 0), (0, -1), (-1, -1)):
        _, s = ref1([p], [t], 1, 1)
        assert s[0] == 1.0
    # both trivial on several pixels
    _, s = ref1([0, 0, 0], [1, 1, 1], 1, 2)
    assert s[0] == 1.0 and s[1] == 1.0


def test_segmentation_ref_without_truth_foreground():
    r, s = ref1([0, 1, -1, 1], [-1, -1, -1, -1], 2, 3)
    assert np.isnan(s[1]) and np.isnan(s[2]) and np.isnan(s[3])
    assert s[4] == 0.0 and r["match"].tolist() == [[-1, -1, -1]] and not r["match_iou"].any()
    assert s[0] == 1.0 or np.isfinite(s[0])
    _, s = ref1([-1, -1], [-1, -1], 2, 3)
    assert s[4] == 1.0 and s[0] == 1.0 and np.isnan(s[1])


def test_segmentation_ref_covering_by_hand():
    # truth: object 0 = pixels 0..3, object 1 = pixels 4..6, object 2 absent, pixels 7..9 background
    # pred:  segment 0 = pixels 0, 1;  segment 1 = pixels 2, 3, 4;  segment 2 = pixels 5, 6, 7;  pixels 8, 9 background
    truth = [0, 0, 0, 0, 1, 1, 1, -1, -1, -1]
    pred = [0, 0, 1, 1, 1, 2, 2, 2, -1, -1]
    r, s = ref1(pred, truth, 3, 3)
    # object 0 (4 px): segment 0: 2 / (2 + 4 - 2) = 1/2, segment 1: 2 / (3 + 4 - 2) = 2/5          -> 1/2 by segment 0
    # object 1 (3 px): segment 1: 1 / (3 + 3 - 1) = 1/5, segment 2: 2 / (3 + 3 - 2) = 1/2          -> 1/2 by segment 2
    assert r["match"].tolist() == [[0, 2, -1]] and r["match_iou"].tolist() == [[0.5, 0.5, 0.0]]
    assert s[2] == 0.5 and s[3] == 0.5
    assert s[4] == 7 / 8                                          # foreground: 8 predicted, 7 true, 7 shared
    assert r["contingency"][0].tolist() == [[2, 0, 0, 0], [0, 2, 0, 0], [0, 2, 1, 0], [1, 0, 2, 0]]
    # an exact tie between unequal fractions, 2/6 = 1/3: the lowest label wins whichever fraction it carries
    truth = [0, 0, 0, -1, -1, -1, -1]
    r, _ = ref1([0, 0, 1, 0, 0, 0, -1], truth, 2, 1)
    assert r["match"].tolist() == [[0]] and r["match_iou"][0, 0] == 1 / 3
    r, _ = ref1([1, 1, 0, 1, 1, 1, -1], truth, 2, 1)
    assert r["match"].tolist() == [[0]] and r["match_iou"][0, 0] == 1 / 3
    # weighting: object 0 (6 px) matched exactly, object 1 (2 px) not met at all
    _, s = ref1([0] * 6 + [-1] * 2, [0] * 6 + [1] * 2, 1, 2)
    assert s[2] == 0.5 and s[3] == 0.75
    # labels outside the range are background
    a = sh.segmentation_ref(np.array([[[3, -7, 2 ** 31 - 1, 1]]]), np.array([[[0, 2, 1, 1]]]), 3, 2)
    b = sh.segmentation_ref(np.array([[[-1, -1, -1, 1]]]), np.array([[[0, -1, 1, 1]]]), 3, 2)
    assert np.array_equal(a["contingency"], b["contingency"]) and np.array_equal(a["scores"], b["scores"], equal_nan=True)


# ---- refusals, before any launch (the non-NULL pointers are never read) ----------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def vp(a):
    return ctypes.c_void_p(a) if a else None


def masks_call(lib, seed=1, first=0, B=2, I=32, K=5, smin=14, smax=28, image=64, bbox=64, count=64, scratch=64, mask=64):
    return lib.spair_scenes_generate_masks(seed, first, B, I, K, smin, smax, vp(image), vp(bbox), vp(count), vp(scratch), vp(mask), None)


@pytest.mark.parametrize("kw", [dict(mask=0), dict(B=0), dict(B=-2), dict(I=0), dict(K=0), dict(K=33), dict(smin=3), dict(smin=20, smax=19),
                                dict(image=0), dict(bbox=0), dict(count=0), dict(scratch=0)])
def test_scenes_generate_masks_refusals(lib, kw):
    assert masks_call(lib, **kw) == ERR_SHAPE


def seg_call(lib, pred=64, truth=64, B=2, HW=64, NP=4, K=3, contingency=64, scores=64, match=64, match_iou=64):
    return lib.spair_segmentation(vp(pred), vp(truth), B, HW, NP, K, vp(contingency), vp(scores), vp(match), vp(match_iou), None)


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(HW=0), dict(HW=-5), dict(HW=2 ** 24 + 1), dict(HW=2 ** 40), dict(NP=0), dict(NP=-1),
                                dict(NP=1025), dict(K=0), dict(K=-1), dict(K=33), dict(pred=0), dict(truth=0), dict(contingency=0),
                                dict(scores=0), dict(pred=0, match=0, match_iou=0)])
def test_segmentation_refusals(lib, kw):
    assert seg_call(lib, **kw) == ERR_SHAPE


def test_surface():
    import spair_pytorch_amd as sp
    from spair_pytorch_amd import _lib, data, metric
    assert sp.segmentation is metric.segmentation and sp.SegmentationResult is metric.SegmentationResult
    assert "segmentation" in sp.__all__ and "SegmentationResult" in sp.__all__
    assert metric.SegmentationResult.__slots__ == ("ari", "ari_fg", "msc", "sc", "fg_iou", "match", "match_iou", "contingency")
    assert callable(metric.SegmentationResult.mean)
    sig = inspect.signature(metric.segmentation)
    assert list(sig.parameters) == ["pred", "truth", "n_pred", "n_truth"]
    assert sig.parameters["n_pred"].default is None and sig.parameters["n_truth"].default is None
    doc = metric.segmentation.__doc__
    for word in ("ParseResult", "owner", "n_pred", "n_truth", "PASS", "synchronisation", "background", "GPU only"):
        assert word in doc, word
    sig = inspect.signature(data.DeviceScatteredDigits.batch)
    assert list(sig.parameters) == ["self", "i", "epoch", "masks"]
    assert sig.parameters["epoch"].default == 0 and sig.parameters["masks"].default is False
    assert "masks=True" in data.DeviceScatteredDigits.__doc__
    header = open(os.path.join(ROOT, "include", "spair_hip.h")).read()
    source = open(_lib.__file__).read()
    for fn in ("spair_scenes_generate_masks", "spair_segmentation"):
        assert "int %s(" % fn in header and fn in source
    assert "#define SPAIR_ABI_VERSION 3" in header and _lib.ABI_VERSION == 3
    assert os.path.exists(os.path.join(ROOT, "spair_pytorch_amd", "csrc", "segmentation.hip"))
    if os.path.exists(_lib.LIB_PATH):
        h = _lib.lib()
        for fn in ("spair_scenes_generate_masks", "spair_segmentation", "spair_scenes_generate"):
            assert hasattr(h, fn)


def test_cpu_tensors_are_refused_not_scored():
    import torch
    from spair_pytorch_amd import _lib, metric
    t = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(_lib.SpairHipError, match="GPU"):
        metric.segmentation(t, t, 1, 1)
    with pytest.raises(_lib.SpairHipError, match="integer"):
        metric.segmentation(t.float(), t, 1, 1)
