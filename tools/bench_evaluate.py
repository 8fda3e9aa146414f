"""Cost of SPAIR.evaluate (bf16 model) at the BASELINE configs[1] (B = 256, 128 x 128, 16 x 16 cells) and configs[3] (B = 64, 256 x 256,
32 x 32 cells) geometries:
  * the whole evaluate(samples=1) and evaluate(samples=4) calls against a no_grad forward() in the same run, by device events;
  * spair_eval_terms alone (the C entry point on preallocated outputs) on the workspace the last forward left, with and without the maps;
  * the bytes k_sample_terms must move -- recon and x, the rows' operands (z_pres, p_z, the six means and standard deviations: 2 A + 12
    floats per row), the two maps and the partials -- and the time that takes at the copy rate DESIGN.md section 8 records (4.85 TB/s).
Device-event times are printed.  For the per-kernel figures (k_sample_terms, k_sample_terms_finish) run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_evaluate.py` and take the means over the traced launches."""
import argparse
import ctypes
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
    ap.add_argument("--calls", type=int, default=50, help="evaluate() / forward() calls")
    args = ap.parse_args()
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import SPAIR, STEP_FLAGS
    dev = torch.device("cuda")
    for label, I, B in (("configs[1]", 128, 256), ("configs[3]", 256, 64)):
        cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
        torch.manual_seed(3)
        m = SPAIR([1, I, I], None, dev, compute_dtype="bf16").to(dev)
        x = torch.from_numpy(scattered_digits(1234, B, I, 11)[0]).to(dev)
        r = m.evaluate(x, 2000, seed=1)
        G = r.z_pres.shape[2]
        HW, A = G * G, int(m._engine(B)["dims"].A)
        assert torch.isfinite(r.terms).all()

        def fwd_call():
            with torch.no_grad():
                m(x, 2000)

        t_f = timed(fwd_call, args.calls, 5)
        t_1 = timed(lambda: m.evaluate(x, 2000, seed=1), args.calls, 5)
        t_4 = timed(lambda: m.evaluate(x, 2000, seed=1, samples=4), max(1, args.calls // 4), 2)
        t_b = timed(lambda: m.evaluate(x, 2000, seed=1, maps=False), args.calls, 5)
        print("%s: no_grad forward() %.4f ms, evaluate(samples=1) %.4f ms, without maps %.4f ms, evaluate(samples=4) %.4f ms"
              % (label, t_f, t_1, t_b, t_4), flush=True)
        # the entry point alone, on the workspace of the last forward
        e = m._engine(B)
        d = e["dims"]
        lib = L.lib()
        n = int(lib.spair_sample_terms_scratch_floats(B, HW, I, I))
        scratch = torch.empty(n, device=dev)
        terms, kl_map, bce_map = torch.empty(B, 9, device=dev), torch.empty(B, 7, HW, device=dev), torch.empty(B, I, I, device=dev)
        recon = r.recon

        def run(maps, accumulate=0):
            L.check(lib.spair_eval_terms(ctypes.byref(d), L.ptr(e["workspace"]), int(STEP_FLAGS), L.ptr(x), L.ptr(recon), 1.0, L.ptr(terms),
                                         L.ptr(kl_map) if maps else None, L.ptr(bce_map) if maps else None, L.ptr(scratch), accumulate,
                                         1.0, L.stream()), "spair_eval_terms")

        t_m = timed(lambda: run(True), args.reps)
        t_a = timed(lambda: run(True, 1), args.reps)
        t_n = timed(lambda: run(False), args.reps)
        moved = 4 * (2 * B * I * I + B * HW * (2 * A + 12) + B * I * I + B * 7 * HW + n)
        print("%s: spair_eval_terms (B = %d, HW = %d, %d workgroups per sample) with maps %.4f ms, accumulating %.4f ms, without maps %.4f ms; "
              "%.1f MB to move = %.4f ms at %.2f TB/s" % (label, B, HW, n // (8 * B), t_m, t_a, t_n, moved / 1e6, moved / COPY_RATE * 1e3,
                                                       COPY_RATE / 1e12), flush=True)
        del m, r, scratch, terms, kl_map, bce_map
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
