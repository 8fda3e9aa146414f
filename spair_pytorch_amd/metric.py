"""Device-side evaluation metrics with the reference's function names (spair/metric.py:5-99).

Differences from the reference, on purpose: nothing is mutated in place, the batch size comes from the
tensors instead of ``cfg.BATCH_SIZE``, results stay on the device (0-dim tensors).  The reference's box convention (z_where taken as
top-left x, y + width, height) is kept so that numbers are comparable with it.
"""
import ctypes

import torch

from . import _lib as L
from . import config as cfg


def _f32(t):
    return t.detach().to(dtype=torch.float32).contiguous()


def _both(z_where, z_pres, ground_truth_bbox, truth_bbox_digit_count, image_side=None):
    if not z_where.is_cuda:
        raise L.SpairHipError("metrics run on the GPU (no CPU fallback)")
    B, _, G, _ = z_where.shape
    K = ground_truth_bbox.shape[1]
    I = int(image_side if image_side is not None else cfg.INPUT_IMAGE_SHAPE[-1])
    zw, zp, bb = _f32(z_where), _f32(z_pres), _f32(ground_truth_bbox)
    cnt = _f32(truth_bbox_digit_count.to(z_where.device)).reshape(-1)
    scratch = torch.empty(2 * B, device=z_where.device, dtype=torch.float32)
    out = torch.empty(2, device=z_where.device, dtype=torch.float32)
    L.check(L.lib().spair_metrics(L.ptr(zw), L.ptr(zp), L.ptr(bb), L.ptr(cnt), B, G, I, K, L.ptr(scratch), L.ptr(out), L.stream()), "spair_metrics")
    return out


def mAP(z_where, z_pres, ground_truth_bbox, truth_bbox_digit_count, image_side=None):
    """Mean average precision @ IoU [0.1:0.1:0.9] of the best predicted box per label box (metric.py:5-47).  Scenes without objects
    (0/0 in the reference) are left out of the batch mean; a batch of only such scenes returns NaN."""
    return _both(z_where, z_pres, ground_truth_bbox, truth_bbox_digit_count, image_side)[0]


def object_count_accuracy(z_pres, truth_bbox_digit_count):
    """Mean of (label count - number of cells with round(z_pres) = 1) (metric.py:49-56)."""
    B, _, G, _ = z_pres.shape
    dummy_w = torch.zeros(B, 4, G, G, device=z_pres.device)
    dummy_b = torch.zeros(B, 1, 4, device=z_pres.device)
    return _both(dummy_w, z_pres, dummy_b, truth_bbox_digit_count, 1)[1]


def batch_jaccard(box_a, box_b):
    """IoU of corner-format boxes: [B,A,4] x [B,Bn,4] -> [B,A,Bn] (metric.py:82-99)."""
    if not box_a.is_cuda:
        raise L.SpairHipError("metrics run on the GPU (no CPU fallback)")
    a, b = _f32(box_a), _f32(box_b)
    out = torch.empty(a.shape[0], a.shape[1], b.shape[1], device=a.device, dtype=torch.float32)
    L.check(L.lib().spair_batch_jaccard(L.ptr(a), L.ptr(b), a.shape[0], a.shape[1], b.shape[1], L.ptr(out), L.stream()), "spair_batch_jaccard")
    return out


class SegmentationResult:
    """What ``segmentation`` returns, all on the device.  Per image: ``ari`` (adjusted Rand index over every pixel), ``ari_fg`` (over the
    pixels of true objects; NaN for an image without one), ``msc`` / ``sc`` (segmentation covering: the mean over the true objects of
    the best IoU with a predicted segment, unweighted / weighted by object size; NaN without an object), ``fg_iou`` (IoU of the two
    foreground masks) -- fp32 [B]; ``match`` int32 [B,K]: the predicted label that covers true object j best (the lowest on a tie, -1 if
    none meets it or it has no pixel) and ``match_iou`` fp32 [B,K] its IoU; ``contingency`` int32 [B,NP+1,K+1]: pixels per (predicted,
    true) label pair, index 0 on either axis being background."""
    __slots__ = ("ari", "ari_fg", "msc", "sc", "fg_iou", "match", "match_iou", "contingency")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __repr__(self):
        return "SegmentationResult(%s)" % ", ".join("%s=%s" % (k, tuple(getattr(self, k).shape)) for k in self.__slots__)

    def mean(self):
        """Batch means of the five scores as a dict of 0-dim device tensors; an image whose score is NaN (no true object) is left out of
        that score's mean, as ``mAP`` leaves out empty scenes, and a batch of only such images gives NaN."""
        return {k: torch.nanmean(getattr(self, k)) for k in ("ari", "ari_fg", "msc", "sc", "fg_iou")}


def _labels(t, what):
    if not torch.is_tensor(t) or t.dim() != 3 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise L.SpairHipError("segmentation: %s must be an integer tensor [B,H,W]" % what)
    if not t.is_cuda:
        raise L.SpairHipError("metrics run on the GPU (no CPU fallback)")
    if t.dtype != torch.int32:
        t = t.detach().clamp(-1, 2 ** 31 - 1).to(torch.int32)       # a label that int32 cannot hold is out of range either way: background
    return t.detach().contiguous()


def segmentation(pred, truth, n_pred=None, n_truth=None):
    """Segmentation quality of a predicted label map against a true one, per image, on the device (csrc/segmentation.hip).

    ``pred``: a ``ParseResult`` (its ``owner`` map is scored and ``n_pred`` is its number of cells) or an integer tensor [B,H,W] with
    labels -1 (background) and 0 .. n_pred-1; ``truth``: an integer tensor [B,H,W] with labels -1 and 0 .. n_truth-1, such as the
    instance mask of ``DeviceScatteredDigits.batch(i, masks=True)``.  A label outside its range counts as background.  n_pred <= 1024,
    n_truth <= 32.  PASS ``n_pred`` and ``n_truth``: left out, each defaults to max(labels) + 1 (at least 1), which costs a device
    reduction and a host synchronisation per call.  Returns a ``SegmentationResult``; every sum is an exact integer and the scores are
    bit-identical from run to run.  Reads no model, no workspace and no status word; GPU only."""
    if hasattr(pred, "owner") and hasattr(pred, "area"):
        if n_pred is None:
            n_pred = int(pred.area.shape[1])
        pred = pred.owner
    p, t = _labels(pred, "pred"), _labels(truth, "truth")
    if p.shape != t.shape or p.device != t.device:
        raise L.SpairHipError("segmentation: pred %s and truth %s differ in shape or device" % (tuple(p.shape), tuple(t.shape)))
    B, HW = int(p.shape[0]), int(p.shape[1]) * int(p.shape[2])
    NP = max(int(p.max().item()) + 1, 1) if n_pred is None else int(n_pred)
    K = max(int(t.max().item()) + 1, 1) if n_truth is None else int(n_truth)
    dev = p.device
    if B < 1 or HW < 1 or not 1 <= NP <= 1024 or not 1 <= K <= 32:
        L.check(-1, "spair_segmentation (B=%d, pixels=%d, n_pred=%d, n_truth=%d)" % (B, HW, NP, K))
    cont = torch.empty(B, NP + 1, K + 1, device=dev, dtype=torch.int32)
    scores = torch.empty(B, 5, device=dev, dtype=torch.float32)
    match = torch.empty(B, K, device=dev, dtype=torch.int32)
    miou = torch.empty(B, K, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        L.check(L.lib().spair_segmentation(L.ptr(p), L.ptr(t), B, HW, NP, K, L.ptr(cont), L.ptr(scores), L.ptr(match), L.ptr(miou),
                                           L.stream()), "spair_segmentation")
    return SegmentationResult(ari=scores[:, 0], ari_fg=scores[:, 1], msc=scores[:, 2], sc=scores[:, 3], fg_iou=scores[:, 4],
                              match=match, match_iou=miou, contingency=cont)
