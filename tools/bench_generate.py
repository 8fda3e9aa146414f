"""Cost of SPAIR.generate (bf16 model) at the BASELINE configs[1] (B = 256, 128 x 128, 16 x 16 cells) and configs[3] (B = 64, 256 x 256,
32 x 32 cells) geometries:
  * the whole generate() call (geometric prior at global_step 0 and 100000, and count = 8) against compose() on the scene it returned and
    against a no_grad forward(), by device events;
  * spair_prior_sample and spair_prior_presence alone (the C entry points on preallocated outputs), the sampler in the dense regime
    (p = 0.999999), late in the schedule (p = 0.0123) and with an exact count.
Device-event times are printed.  The sampler's yardstick is k_count_kl, which runs the same recurrence on a given z_pres inside
forward(): for the per-kernel figures (k_prior_presence, k_prior_gauss, k_count_kl on the same B and G * Gw) run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_generate.py` and take the means over the traced launches."""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="launches per entry point")
    ap.add_argument("--calls", type=int, default=50, help="generate() / compose() / forward() calls")
    args = ap.parse_args()
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import NOISE_MAPS, SPAIR
    dev = torch.device("cuda")
    for label, I, B in (("configs[1]", 128, 256), ("configs[3]", 256, 64)):
        cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
        torch.manual_seed(3)
        m = SPAIR([1, I, I], None, dev, compute_dtype="bf16").to(dev)
        x = torch.from_numpy(scattered_digits(1234, B, I, 11)[0]).to(dev)
        r = m.generate(B, 0, seed=1)
        G = r.z_where.shape[2]
        HW = G * G
        assert torch.equal(m.compose(r).recon, r.recon)

        def fwd_call():
            with torch.no_grad():
                m(x, 2000)

        t_f = timed(fwd_call, args.calls, 5)          # (k_count_kl on the same B and HW: the sampler's yardstick in a kernel trace)
        t_c = timed(lambda: m.compose(r), args.calls, 5)
        t_g0 = timed(lambda: m.generate(B, 0, seed=1), args.calls, 5)
        t_gl = timed(lambda: m.generate(B, 100000, seed=1), args.calls, 5)
        t_gc = timed(lambda: m.generate(B, 0, seed=1, count=8), args.calls, 5)
        noise = {k: torch.empty_like(v) for k, v in m._engine(B)["noise"].items()}
        L.check(L.lib().spair_noise_fill(ctypes.byref(m._engine(B)["dims"]), 1, *(L.ptr(noise[k]) for k in NOISE_MAPS), L.stream()), "noise")
        t_gn = timed(lambda: m.generate(B, 0, noise=noise), args.calls, 5)
        print("%s: no_grad forward() %.4f ms, compose() %.4f ms, generate(seed) at step 0 %.4f ms, at step 100000 %.4f ms, "
              "count = 8 %.4f ms, generate(noise) at step 0 %.4f ms" % (label, t_f, t_c, t_g0, t_gl, t_gc, t_gn), flush=True)
        # the entry points alone, on preallocated outputs
        d = m._engine(B)["dims"]
        outs = [torch.empty_like(v) for v in (r.z_where, r.z_what, r.z_depth, r.z_pres, r.p_z, r.count)]
        cnt = torch.full((B,), 8, device=dev, dtype=torch.int32)
        u = noise["u_pres"].reshape(B, HW)

        def run_sample():
            L.check(L.lib().spair_prior_sample(ctypes.byref(d), 0.999999, None, *(L.ptr(noise[k]) for k in NOISE_MAPS),
                                               *(L.ptr(t) for t in outs), L.stream()), "spair_prior_sample")

        def run_presence(p, count=None):
            L.check(L.lib().spair_prior_presence(L.ptr(u), B, HW, p, L.ptr(count), L.ptr(outs[3]), L.ptr(outs[4]), L.ptr(outs[5]), L.stream()),
                    "spair_prior_presence")

        t_s = timed(run_sample, args.reps)
        t_d = timed(lambda: run_presence(0.999999), args.reps)
        t_l = timed(lambda: run_presence(0.0123), args.reps)
        t_n = timed(lambda: run_presence(0.5, cnt), args.reps)
        print("%s: spair_prior_sample %.4f ms; spair_prior_presence (B = %d, HW = %d) p = 0.999999 %.4f ms, p = 0.0123 %.4f ms, "
              "count = 8 %.4f ms" % (label, t_s, B, HW, t_d, t_l, t_n), flush=True)
        del m, r, outs, noise
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
