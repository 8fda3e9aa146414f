"""Detection average precision on the device (csrc/detection.hip; definitions in include/spair_hip.h, "detection metrics").

Predicted boxes are ranked by confidence and matched greedily one-to-one against the true boxes of their image at every IoU threshold
(a second box on an object is a false positive); the precision / recall curve is pooled over every image fed, and AP is the area under
its precision envelope, per threshold and averaged -- the number the SPAIR paper reports, with count accuracy beside it.

Box convention: predictions are true corner boxes (x0, y0, x1, y1) in pixels, as ``parse_boxes`` / ``ParseResult.boxes`` give them (the
footprint of the sprite where the renderer places it); truths are (x, y, w, h) in pixels, as ``DeviceScatteredDigits`` gives them.
This is not ``metric.mAP``'s top-left reading of z_where: ``metric.mAP`` and ``metric.object_count_accuracy`` remain the reference's
functions (best IoU per label box without ranking or false positives, and the mean signed count error), pinned to its outputs.
"""
import torch

from . import _lib as L

COUNTERS = 24            # SPAIR_DET_COUNTERS
MAX_N, MAX_K, MAX_T = 1024, 32, 16


class DetectionBatch:
    """What ``DetectionAP.update`` returns, on the device, per image of the batch in ranked order (score descending, equal scores by
    lower index): ``order`` int32 [B,max_det] the prediction's index (the cell k of a parse; -1 in a dead slot), ``score`` fp32
    [B,max_det] (-inf in a dead slot), ``tp`` int32 [B,max_det] (bit t: a true positive at threshold t), ``n_pred`` int32 [B] live
    predictions before the ``max_det`` cap, ``n_truth`` int32 [B] real truths.  The tensors are views of the accumulator's rows: they
    hold until its ``reset``."""
    __slots__ = ("order", "score", "tp", "n_pred", "n_truth")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __repr__(self):
        return "DetectionBatch(%s)" % ", ".join("%s=%s" % (k, tuple(getattr(self, k).shape)) for k in self.__slots__)


class DetectionResult:
    """What ``DetectionAP.compute`` returns, all device tensors: ``ap`` float64 [T] (NaN without a true box, 0 without a prediction),
    ``mean_ap`` (its mean; NaN if any is NaN), ``recall`` / ``precision`` float64 [T] at the end of the curve, ``thresholds`` fp32 [T];
    ``n_images``, ``n_truth`` (real true boxes), ``n_pred`` (live predictions, before the cap), ``n_records`` (predictions that entered
    the matching) int64; ``count_accuracy`` (share of images with n_pred == count), ``count_mae`` (mean |n_pred - count|),
    ``count_bias`` (mean n_pred - count) float64, NaN without an image."""
    __slots__ = ("ap", "mean_ap", "recall", "precision", "thresholds", "n_images", "n_truth", "n_pred", "n_records", "count_accuracy",
                 "count_mae", "count_bias")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __repr__(self):
        return "DetectionResult(%s)" % ", ".join("%s=%s" % (k, getattr(self, k).tolist()) for k in self.__slots__)


def _gpu(t, what):
    if not torch.is_tensor(t):
        raise L.SpairHipError("detection: %s must be a tensor" % what)
    if not t.is_cuda:
        raise L.SpairHipError("detection metrics run on the GPU (no CPU fallback): %s is on %s" % (what, t.device))
    return t.detach()


def _inputs(pred, bbox, count, scores):
    """(boxes fp32 [B,N,4], scores fp32 [B,N], bbox fp32 [B,K,4], count int32 [B]) on one device, contiguous"""
    if hasattr(pred, "boxes") and hasattr(pred, "z_pres"):
        if scores is not None:
            raise L.SpairHipError("detection: scores come with the ParseResult (its z_pres)")
        pred, scores = pred.boxes, pred.z_pres
    elif scores is None:
        raise L.SpairHipError("detection: a box tensor needs scores [B,N]")
    boxes, scores, bbox, count = _gpu(pred, "pred"), _gpu(scores, "scores"), _gpu(bbox, "bbox"), _gpu(count, "count")
    if boxes.dim() != 3 or boxes.shape[2] != 4 or not boxes.is_floating_point():
        raise L.SpairHipError("detection: pred must be a float tensor [B,N,4] of corner boxes")
    B, N = int(boxes.shape[0]), int(boxes.shape[1])
    if bbox.dim() != 3 or bbox.shape[0] != B or bbox.shape[2] != 4 or scores.numel() != B * N or count.numel() != B:
        raise L.SpairHipError("detection: pred %s, scores %s, bbox %s and count %s do not belong together"
                              % (tuple(boxes.shape), tuple(scores.shape), tuple(bbox.shape), tuple(count.shape)))
    dev = boxes.device
    if scores.device != dev or bbox.device != dev or count.device != dev:
        raise L.SpairHipError("detection: the tensors are on different devices")
    K = int(bbox.shape[1])
    count = count.reshape(B)
    if count.is_floating_point():
        count = count.round()
    count = count.clamp(0, K).to(torch.int32).contiguous()
    f32 = torch.float32
    return boxes.to(f32).contiguous(), scores.reshape(B, N).to(f32).contiguous(), bbox.to(f32).contiguous(), count


def _check_limits(B, N, K, T, max_det):
    if B < 1 or not 1 <= N <= MAX_N or not 1 <= K <= MAX_K or not 1 <= T <= MAX_T or not 1 <= max_det <= N:
        L.check(-1, "spair_det_match (B=%d, N=%d, K=%d, T=%d, max_det=%d)" % (B, N, K, T, max_det))


class DetectionAP:
    """Average precision of predicted boxes and count accuracy over an evaluation set, accumulated on the device.

    ``thresholds``: IoU thresholds (at most 16; default ``torch.arange(0.1, 1.0, 0.1)`` in fp32, the reference's and the paper's nine);
    ``min_score``: a prediction is live at score >= min_score (a NaN score is dead); ``max_det``: only the best-ranked max_det live
    predictions of an image enter the matching (COCO's maxDets; clamped to the number of predictions N at the first update);
    ``capacity``: images the buffers hold before they double (by a device copy); ``device``: default the current GPU.

    Boxes are true corner boxes (x0, y0, x1, y1) in pixels -- ``ParseResult.boxes`` -- against truths (x, y, w, h) in pixels --
    ``DeviceScatteredDigits``'s ``bbox`` -- not ``metric.mAP``'s top-left reading; ``mAP`` and ``object_count_accuracy`` remain the
    reference's functions.  Reads no model, no workspace and no status word; GPU only."""

    def __init__(self, thresholds=None, min_score=0.5, max_det=100, capacity=1024, device=None):
        if thresholds is None:
            thresholds = torch.arange(0.1, 1.0, 0.1)
        thr = torch.as_tensor(thresholds).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
        self.thresholds_host = tuple(thr.tolist())
        self.min_score, self.max_det, self.capacity = float(min_score), int(max_det), max(int(capacity), 1)
        if not 1 <= len(self.thresholds_host) <= MAX_T or self.max_det < 1 or self.min_score - self.min_score != 0.0:
            raise L.SpairHipError("DetectionAP: 1 to %d thresholds, max_det >= 1 and a finite min_score" % MAX_T)
        self.device = None
        self.n_images = 0                        # host-known: images fed (their rows of the buffers are written)
        self._md = None                          # max_det clamped to N: the slots per image
        if device is not None or torch.cuda.is_available():
            self._place(torch.device(device if device is not None else "cuda"))

    def _place(self, dev):
        if dev.type != "cuda":
            raise L.SpairHipError("detection metrics run on the GPU (no CPU fallback): device %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._thr = torch.tensor(self.thresholds_host, dtype=torch.float32).to(dev)          # the one host-to-device copy
        self._counters = torch.zeros(COUNTERS, dtype=torch.int64, device=dev)

    def _alloc(self, cap):
        dev, md = self.device, self._md
        return (torch.empty(cap, md, dtype=torch.float32, device=dev), torch.empty(cap, md, dtype=torch.int32, device=dev),
                torch.empty(cap, md, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                torch.empty(cap, dtype=torch.int32, device=dev))

    def _reserve(self, n_new, N):
        """room for n_new more images of N predictions each; returns the first free row"""
        if self._md is None:
            self._md = min(self.max_det, N)
            self._bufs = self._alloc(self.capacity)
        elif N < self._md:
            raise L.SpairHipError("DetectionAP: %d predictions per image, fewer than the %d slots of the earlier updates" % (N, self._md))
        n = self.n_images
        if n + n_new > self.capacity:
            while n + n_new > self.capacity:
                self.capacity *= 2
            old, self._bufs = self._bufs, self._alloc(self.capacity)
            for o, b in zip(old, self._bufs):
                b[:n].copy_(o[:n])
        return n

    def update(self, pred, bbox, count, scores=None):
        """Rank and match one batch and append it.  ``pred``: a ``ParseResult`` (its ``boxes`` and, as scores, its ``z_pres`` in cell
        order) or a float tensor [B,N,4] of corner boxes with ``scores`` [B,N]; ``bbox`` [B,K,4] (x, y, w, h) and ``count`` [B] (float
        or integer; rounded and clamped to [0, K]): what ``DeviceScatteredDigits.batch`` returns.  N <= 1024, K <= 32.  Returns a
        ``DetectionBatch``.  One launch on the current stream: no ``.item()``, no host copy and no synchronisation, so it can run inside
        a validation loop between training steps (without a GPU at construction and no ``device=``, the first update uploads the
        thresholds).  CPU tensors are refused: GPU only."""
        boxes, scores, bbox, count = _inputs(pred, bbox, count, scores)
        B, N, K, T = int(boxes.shape[0]), int(boxes.shape[1]), int(bbox.shape[1]), len(self.thresholds_host)
        _check_limits(B, N, K, T, min(self.max_det, N) if self._md is None else self._md)
        if self.device is None:
            self._place(boxes.device)
        if boxes.device != self.device:
            raise L.SpairHipError("DetectionAP: the accumulator is on %s, the batch on %s" % (self.device, boxes.device))
        n = self._reserve(B, N)
        score, tp, order, n_pred, n_truth = (b[n:n + B] for b in self._bufs)
        with torch.cuda.device(self.device):
            L.check(L.lib().spair_det_match(L.ptr(boxes), L.ptr(scores), L.ptr(bbox), L.ptr(count), L.ptr(self._thr), B, N, K, T,
                                            self.min_score, self._md, L.ptr(score), L.ptr(tp), L.ptr(order), L.ptr(n_pred),
                                            L.ptr(n_truth), L.ptr(self._counters), None, L.stream()), "spair_det_match")
        self.n_images = n + B
        return DetectionBatch(order=order, score=score, tp=tp, n_pred=n_pred, n_truth=n_truth)

    def compute(self):
        """The pooled curve of everything fed so far, as a ``DetectionResult`` of device tensors: a stable device sort of the records by
        score (``torch.sort``), one launch for the AP of every threshold, and a few element-wise ops for the count statistics.  No
        ``.item()`` and no host copy; bit-identical from run to run.  May be called repeatedly, and more updates may follow."""
        if self.device is None:
            raise L.SpairHipError("DetectionAP.compute: nothing was fed and no GPU device was given")
        T, n = len(self.thresholds_host), self.n_images
        dev = self.device
        if n:
            score, idx = torch.sort(self._bufs[0][:n].reshape(-1), descending=True, stable=True)      # dead slots (-inf) last
            tp = self._bufs[1][:n].reshape(-1)[idx]
        else:
            tp = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.empty(3, T, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().spair_det_ap(L.ptr(tp), int(tp.numel()), T, L.ptr(self._counters), L.ptr(out), L.stream()), "spair_det_ap")
        c = self._counters.clone()
        images = c[5].double()
        return DetectionResult(ap=out[0], mean_ap=out[0].mean(), recall=out[1], precision=out[2], thresholds=self._thr.clone(),
                               n_images=c[5], n_truth=c[0], n_pred=c[0] + c[4], n_records=c[1], count_accuracy=c[2].double() / images,
                               count_mae=c[3].double() / images, count_bias=c[4].double() / images)

    def reset(self):
        """Forget every image fed (the buffers and their capacity stay)."""
        self.n_images = 0
        if self.device is not None:
            self._counters.zero_()

    def merge(self, other):
        """Append the images of ``other`` (a ``DetectionAP`` with the same thresholds, ``min_score`` and ``max_det``) after one's own,
        as if they had been fed here next; ``other`` is left as it is.  A DDP user all-gathers with it."""
        if not isinstance(other, DetectionAP) or other.thresholds_host != self.thresholds_host or other.min_score != self.min_score or \
                other.max_det != self.max_det:
            raise L.SpairHipError("DetectionAP.merge: the accumulators differ in thresholds, min_score or max_det")
        if other.n_images == 0:
            return self
        if self.device is None:
            self._place(other.device)
        if self._md is not None and self._md != other._md:
            raise L.SpairHipError("DetectionAP.merge: %d slots per image here, %d there" % (self._md, other._md))
        n, m = self._reserve(other.n_images, other._md), other.n_images
        for mine, theirs in zip(self._bufs, other._bufs):
            mine[n:n + m].copy_(theirs[:m])
        self._counters += other._counters.to(self.device)
        self.n_images = n + m
        return self


def detection_ap(pred, bbox, count, scores=None, **kw):
    """One ``DetectionAP(**kw).update(pred, bbox, count, scores)`` and its ``compute()``: the ``DetectionResult`` of a single batch.
    True corner boxes against (x, y, w, h) truths, as in ``DetectionAP``; GPU only."""
    first = pred.boxes if hasattr(pred, "boxes") else pred
    dev = _gpu(first, "pred").device
    acc = DetectionAP(device=dev, capacity=int(first.shape[0]), **kw)
    acc.update(pred, bbox, count, scores)
    return acc.compute()


def match_iou(boxes, scores, bbox, count, thresholds, min_score=0.5, max_det=100):
    """spair_det_match alone on one batch, with its IoU matrix: returns (``DetectionBatch``, iou fp32 [B,N,K], counters int64 [24]).
    ``iou[b, n, j]`` is the IoU of prediction n with truth slot j as defined in include/spair_hip.h, for all K slots."""
    boxes, scores, bbox, count = _inputs(boxes, bbox, count, scores)
    dev = boxes.device
    thr = torch.as_tensor(thresholds).detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    B, N, K, T = int(boxes.shape[0]), int(boxes.shape[1]), int(bbox.shape[1]), int(thr.numel())
    md = min(int(max_det), N)
    _check_limits(B, N, K, T, md)
    score = torch.empty(B, md, dtype=torch.float32, device=dev)
    tp, order = (torch.empty(B, md, dtype=torch.int32, device=dev) for _ in range(2))
    n_pred, n_truth = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    counters = torch.zeros(COUNTERS, dtype=torch.int64, device=dev)
    iou = torch.empty(B, N, K, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().spair_det_match(L.ptr(boxes), L.ptr(scores), L.ptr(bbox), L.ptr(count), L.ptr(thr), B, N, K, T, float(min_score), md,
                                        L.ptr(score), L.ptr(tp), L.ptr(order), L.ptr(n_pred), L.ptr(n_truth), L.ptr(counters), L.ptr(iou),
                                        L.stream()), "spair_det_match")
    return DetectionBatch(order=order, score=score, tp=tp, n_pred=n_pred, n_truth=n_truth), iou, counters
