"""Cost of DetectionAP at the BASELINE configs[1] geometry (B = 256, 128 x 128, 16 x 16 cells: N = 256 predictions per image), K = 11
objects: the boxes of DeviceScatteredDigits against the parse() of an untrained bf16 model.
  * update(): at the default min_score (0.5) and max_det (100) -- where the untrained model has no live cell at all --, at the min_score
    that leaves six live cells per image (as many as there are objects: what a trained model's parse looks like), and at min_score = 0
    with max_det = 256 -- every cell live and kept, the worst case for the matching walk; the whole call (input conversions and the launch) and spair_det_match alone on preallocated rows;
  * compute(): at 256, 4,096 and 65,536 images (the same batch fed 1, 16 and 256 times, six records per image); the whole call, and its parts: the stable device
    sort with the gather of the tp words, and spair_det_ap alone;
  * the baseline: a restatement of the same definitions (include/spair_hip.h, "detection metrics") in plain torch ops, which lives here
    and not in the product.  Its matching walks the ranked list with a Python loop of tensor ops over [B, T, K] (the walk is sequential
    by definition); its curve is a cumsum, a reversed cummax and a sum.  Its results are held to the device's before anything is timed.
Device-event times are printed.  For the per-kernel figures (k_det_match, k_det_ap) run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_detection.py --no-baseline` in a run of its own."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


# ---- the restatement in torch ops ------------------------------------------------------------------------------------------------------------
def torch_iou(boxes, bbox):
    a, b = boxes[:, :, None, :], bbox[:, None, :, :]
    bx1, by1 = b[..., 0] + b[..., 2], b[..., 1] + b[..., 3]
    zero = boxes.new_zeros(())
    iw = torch.maximum(torch.minimum(a[..., 2], bx1) - torch.maximum(a[..., 0], b[..., 0]), zero)
    ih = torch.maximum(torch.minimum(a[..., 3], by1) - torch.maximum(a[..., 1], b[..., 1]), zero)
    inter = iw * ih
    un = ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (bx1 - b[..., 0]) * (by1 - b[..., 1])) - inter
    q = inter / un
    ok = torch.isfinite(a).all(-1) & torch.isfinite(b).all(-1) & torch.isfinite(bx1) & torch.isfinite(by1)
    return torch.where(ok & (un > 0) & (q > 0), q, zero)


def torch_update(boxes, scores, bbox, cnt, thr, min_score, max_det):
    """-> score, tp, order [B, max_det], n_pred, n_truth [B]"""
    B, N = scores.shape
    K, T = bbox.shape[1], thr.numel()
    iou = torch_iou(boxes, bbox)                                                         # [B,N,K]
    live = ~torch.isnan(scores) & (scores >= min_score)
    n_pred = live.sum(1).to(torch.int32)
    key = torch.where(live, scores, scores.new_full((), -float("inf")))
    s_sorted, order = torch.sort(key, dim=1, descending=True, stable=True)
    s_sorted, order = s_sorted[:, :max_det], order[:, :max_det]
    on = torch.arange(max_det, device=scores.device)[None] < n_pred[:, None]
    n_truth = cnt.clamp(0, K).to(torch.int32)
    free = (torch.arange(K, device=scores.device)[None] < n_truth[:, None])[:, None, :].expand(B, T, K).clone()      # [B,T,K]
    ranked_iou = torch.gather(iou, 1, order[:, :, None].expand(B, max_det, K))           # [B,max_det,K]
    js = torch.arange(K, device=scores.device)
    tp = torch.zeros(B, max_det, dtype=torch.int32, device=scores.device)
    weights = (1 << torch.arange(T, device=scores.device)).to(torch.int32)
    for r in range(max_det):                                                             # the walk: sequential by definition
        v = torch.where(free, ranked_iou[:, r, None, :], ranked_iou.new_full((), -1.0))  # [B,T,K]
        m = v.max(-1).values                                                             # [B,T]
        first = torch.where((v == m[..., None]) & free, js, K).min(-1).values            # the lowest j at the max
        hit = (first < K) & (m >= thr[None]) & on[:, r, None]
        free &= ~(hit[..., None] & (js == first[..., None]))
        tp[:, r] = (hit.to(torch.int32) * weights).sum(-1)
    neg = s_sorted.new_full((), -float("inf"))
    return torch.where(on, s_sorted, neg), tp, torch.where(on, order, -1).to(torch.int32), n_pred, n_truth


def torch_compute(score, tp, n_truth, T):
    """score, tp [n, max_det], n_truth [n] -> ap, recall, precision float64 [T]"""
    s, idx = torch.sort(score.reshape(-1), descending=True, stable=True)
    w = tp.reshape(-1)[idx]
    valid = (s > -float("inf")).to(torch.float64)
    bits = ((w[None] >> torch.arange(T, device=w.device)[:, None]) & 1).to(torch.float64)       # [T,M]
    tps = bits.cumsum(1)
    prec = tps / torch.arange(1, w.numel() + 1, device=w.device, dtype=torch.float64)[None] * valid[None]
    env = prec.flip(1).cummax(1).values.flip(1)
    NT = n_truth.sum().double()
    return (env * bits).sum(1) / NT, tps[:, -1] / NT, tps[:, -1] / valid.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true", help="leave the torch restatement out (the profiled run)")
    args = ap.parse_args()
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd import detection
    from spair_pytorch_amd.data import DeviceScatteredDigits
    from spair_pytorch_amd.models import SPAIR
    dev = torch.device("cuda")
    I, B, K = 128, 256, 11
    cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(3)
    m = SPAIR([1, I, I], None, dev, compute_dtype="bf16").to(dev)
    ds = DeviceScatteredDigits(10 ** 6, B, image_side=I, max_objects=K, seed=1234)
    x, bbox, cnt = ds.batch(0)
    parse = m.parse(x, 2000, threshold=0.02)
    boxes, scores = parse.boxes.float().contiguous(), parse.z_pres.reshape(B, -1).float().contiguous()
    N = int(scores.shape[1])
    t_parse = timed(lambda: m.parse(x, 2000, threshold=0.02), args.reps, 5)
    print("configs[1]: B = %d, %d x %d, N = %d, K = %d; live cells at 0.5: %.1f per image, true boxes %.1f per image; parse() %.4f ms"
          % (B, I, I, N, K, float((scores >= 0.5).sum()) / B, float(cnt.sum()) / B, t_parse), flush=True)
    lib = L.lib()
    # an untrained model's presences are all below 0.5: the middle case puts min_score where a trained model's would leave about as many
    # live cells as there are objects (six per image), so that the curve has records
    six = float(torch.quantile(scores.reshape(-1)[:65536 * 16].float(), 1 - 6.0 / N))
    for label, min_score, max_det in (("min_score 0.5, max_det 100", 0.5, 100), ("min_score %.6f (6 live per image), max_det 100" % six, six, 100),
                                      ("min_score 0, max_det 256", 0.0, 256)):
        acc = detection.DetectionAP(min_score=min_score, max_det=max_det, capacity=B * (args.reps + 8), device=dev)
        batch = acc.update(parse, bbox, cnt)
        res = acc.compute()
        md = int(batch.score.shape[1])
        print("%s: records %d of %d slots; mean AP %.4f, count accuracy %.4f, count bias %.2f"
              % (label, int(res.n_records), B * md, float(res.mean_ap), float(res.count_accuracy), float(res.count_bias)), flush=True)
        acc.reset()
        t_update = timed(lambda: acc.update(parse, bbox, cnt), args.reps, 3)
        acc.reset()
        cnt32 = cnt.to(torch.int32)
        rows = [b[:B] for b in acc._bufs]

        def run():
            L.check(lib.spair_det_match(L.ptr(boxes), L.ptr(scores), L.ptr(bbox), L.ptr(cnt32), L.ptr(acc._thr), B, N, K, 9, min_score, md,
                                        L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(rows[2]), L.ptr(rows[3]), L.ptr(rows[4]), L.ptr(acc._counters),
                                        None, L.stream()), "spair_det_match")

        t_match = timed(run, args.reps)
        line = "%s: update() %.4f ms, spair_det_match alone %.4f ms" % (label, t_update, t_match)
        if not args.no_baseline:
            ref = torch_update(boxes, scores, bbox, cnt, acc._thr, min_score, md)
            wrong = {name: int((got != exp).sum()) for got, exp, name in
                     zip((batch.score, batch.tp, batch.order, batch.n_pred, batch.n_truth), ref, ("score", "tp", "order", "n_pred", "n_truth"))}
            assert sum(wrong.values()) <= 2, wrong          # (torch's own division may round an IoU on a threshold the other way)
            t_torch = timed(lambda: torch_update(boxes, scores, bbox, cnt, acc._thr, min_score, md), max(args.reps // 4, 3), 1)
            line += "; the torch-ops restatement %.4f ms (%.0f x)" % (t_torch, t_torch / t_update)
        print(line, flush=True)
        if min_score in (0.5, 0.0):
            continue
        for times in (1, 16, 256):
            acc = detection.DetectionAP(min_score=min_score, max_det=max_det, capacity=B * times, device=dev)
            for _ in range(times):
                acc.update(parse, bbox, cnt)
            n = acc.n_images
            res = acc.compute()
            t_compute = timed(acc.compute, args.reps)
            score, tp = acc._bufs[0][:n].reshape(-1), acc._bufs[1][:n].reshape(-1)

            def sort_gather():
                s, idx = torch.sort(score, descending=True, stable=True)
                return tp[idx]

            t_sort = timed(sort_gather, args.reps)
            tps = sort_gather()
            out = torch.empty(3, 9, dtype=torch.float64, device=dev)
            t_ap = timed(lambda: L.check(lib.spair_det_ap(L.ptr(tps), int(tps.numel()), 9, L.ptr(acc._counters), L.ptr(out), L.stream()),
                                         "spair_det_ap"), args.reps)
            assert torch.equal(out[0].view(torch.int64), res.ap.view(torch.int64))
            line = "compute() at %d images (%d slots, %d records): %.4f ms; sort + gather %.4f ms, spair_det_ap alone %.4f ms" \
                % (n, score.numel(), int(res.n_records), t_compute, t_sort, t_ap)
            if not args.no_baseline:
                ref = torch_compute(acc._bufs[0][:n], acc._bufs[1][:n], acc._bufs[4][:n], 9)
                worst = max(float((a - b).abs().max()) for a, b in zip(ref, (res.ap, res.recall, res.precision)))
                assert worst <= 1e-12, worst
                t_torch = timed(lambda: torch_compute(acc._bufs[0][:n], acc._bufs[1][:n], acc._bufs[4][:n], 9), args.reps)
                line += "; the torch-ops restatement %.4f ms (%.1f x), worst difference %.2g" % (t_torch, t_torch / t_compute, worst)
            print(line, flush=True)
            del acc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
