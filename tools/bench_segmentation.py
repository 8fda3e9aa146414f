"""Cost of metric.segmentation at the BASELINE configs[1] (B = 256, 128 x 128, 16 x 16 cells: NP = 256) and configs[3] (B = 64, 256 x 256,
32 x 32 cells: NP = 1024) geometries, K = 11 objects: the instance masks of DeviceScatteredDigits against the owner map of an untrained
bf16 model's parse():
  * the whole segmentation() call (label checks, four result tensors, the memset and the two launches) beside parse() on the same batch
    and beside batch(i) with and without masks, by device events;
  * spair_segmentation alone (the C entry point on preallocated outputs), back to back;
  * the bytes k_seg_count must move -- 8 per pixel (one int of each map) plus the image's table in memory (the memset and the flush's
    atomics: 4 (NP + 1)(K + 1) per image) -- and the time that takes at the copy rate DESIGN.md section 8 records (4.85 TB/s).
Device-event times are printed.  For the per-kernel figures (k_seg_count, k_seg_finish, k_scene_render_mask) run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_segmentation.py` in a run of its own and take the means over the traced launches
(the two geometries differ in grid size)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 4.85e12      # bytes per second


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="launches of the entry point")
    ap.add_argument("--calls", type=int, default=50, help="segmentation() / parse() / batch() calls")
    args = ap.parse_args()
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd import metric
    from spair_pytorch_amd.data import DeviceScatteredDigits
    from spair_pytorch_amd.models import SPAIR
    dev = torch.device("cuda")
    K = 11
    for label, I, B in (("configs[1]", 128, 256), ("configs[3]", 256, 64)):
        cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
        torch.manual_seed(3)
        m = SPAIR([1, I, I], None, dev, compute_dtype="bf16").to(dev)
        ds = DeviceScatteredDigits(10 ** 6, B, image_side=I, max_objects=K, seed=1234)
        x, bbox, cnt, mask = ds.batch(0, masks=True)
        r = m.parse(x, 2000, threshold=0.02)
        NP = int(r.area.shape[1])
        s = metric.segmentation(r, mask, n_truth=K)
        print("%s: B = %d, %d x %d, NP = %d, K = %d; truth foreground %.3f, owned pixels %.3f; means %s"
              % (label, B, I, I, NP, K, float((mask >= 0).float().mean()), float((r.owner >= 0).float().mean()),
                 {k: round(float(v), 4) for k, v in s.mean().items()}), flush=True)
        t_plain, t_mask = timed(lambda: ds.batch(0), args.calls), timed(lambda: ds.batch(0, masks=True), args.calls)
        t_parse = timed(lambda: m.parse(x, 2000, threshold=0.02), args.calls, 5)
        t_seg = timed(lambda: metric.segmentation(r, mask, n_truth=K), args.calls, 5)
        t_auto = timed(lambda: metric.segmentation(r.owner, mask), args.calls, 5)
        print("%s: batch() %.4f ms, batch(masks=True) %.4f ms; parse() %.4f ms; segmentation() %.4f ms, with n_pred / n_truth left out %.4f ms"
              % (label, t_plain, t_mask, t_parse, t_seg, t_auto), flush=True)
        owner = r.owner.contiguous()
        cont = torch.empty(B, NP + 1, K + 1, device=dev, dtype=torch.int32)
        scores, match, miou = torch.empty(B, 5, device=dev), torch.empty(B, K, device=dev, dtype=torch.int32), torch.empty(B, K, device=dev)
        lib = L.lib()

        def run():
            L.check(lib.spair_segmentation(L.ptr(owner), L.ptr(mask), B, I * I, NP, K, L.ptr(cont), L.ptr(scores), L.ptr(match), L.ptr(miou),
                                           L.stream()), "spair_segmentation")

        t_e = timed(run, args.reps)
        assert torch.equal(cont, s.contingency) and int(cont.sum()) == B * I * I
        pixels, table = 8 * B * I * I, 4 * B * (NP + 1) * (K + 1)
        print("%s: spair_segmentation alone %.4f ms; k_seg_count must move %.1f MB of labels + %.1f MB of tables = %.4f ms at %.2f TB/s; "
              "non-zero table entries %d of %d" % (label, t_e, pixels / 1e6, table / 1e6, (pixels + table) / COPY_RATE * 1e3, COPY_RATE / 1e12,
                                                 int((cont != 0).sum()), cont.numel()), flush=True)
        del m, r, s, cont
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
