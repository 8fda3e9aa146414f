"""Cost of the input-image gradient (x.requires_grad_(); SpairStepIO.grad_x) on the benchmark step: ms per zero_grad + forward + backward + Adam
at BASELINE configs[1] (128x128, 16x16 grid, B=256, bf16) and configs[3] (256x256, 32x32 grid, B=64), without and with x.requires_grad.

    python tools/bench_input_grad.py                       # ms/step of the four runs
    python tools/bench_input_grad.py --trace OUT_DIR       # each run in a child under rocprofv3 --kernel-trace --stats (OUT_DIR/<run>/)
"""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"configs1": (128, 256, (2, 2, 2, 1, 1, 1)), "configs3": (256, 64, (2, 2, 2, 1, 1, 1))}
RUNS = [(c, xg) for c in CONFIGS for xg in (False, True)]


def run_name(cfg_name, xgrad):
    return "%s_%s" % (cfg_name, "xgrad" if xgrad else "default")


def bench(cfg_name, xgrad, steps, warmup):
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import SPAIR
    from spair_pytorch_amd.optim import FusedAdam
    I, B, strides = CONFIGS[cfg_name]
    cfg.set_grid(I, strides)
    dev = torch.device("cuda")
    x = torch.from_numpy(scattered_digits(1234, B, I, 11)[0]).to(dev)
    torch.manual_seed(3)
    m = SPAIR([1, I, I], None, dev, compute_dtype="bf16").to(dev)
    opt = FusedAdam(m, lr=1e-4)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    xx = x.clone().requires_grad_(xgrad)
    for it in range(warmup + steps):
        if it == warmup:
            torch.cuda.synchronize()
            ev[0].record()
        opt.zero_grad()
        xx.grad = None
        loss, recon, z_where, z_pres = m(xx, 2000 + it)
        loss.backward()
        opt.step()
    ev[1].record()
    torch.cuda.synchronize()
    print("%-18s %.4f ms/step" % (run_name(cfg_name, xgrad), ev[0].elapsed_time(ev[1]) / steps), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--run", help="one run: configs1_default, configs1_xgrad, configs3_default or configs3_xgrad")
    ap.add_argument("--trace", help="directory for one rocprofv3 --kernel-trace --stats output per run")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per traced child")
    args = ap.parse_args()
    runs = [r for r in RUNS if args.run in (None, run_name(*r))]
    if not args.trace:
        for c, xg in runs:
            bench(c, xg, args.steps, args.warmup)
        return
    for c, xg in runs:
        out = os.path.join(args.trace, run_name(c, xg))
        os.makedirs(out, exist_ok=True)
        cmd = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--run", run_name(c, xg), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        rc = subprocess.call(cmd)
        if rc != 0:           # a failed or timed-out child ends the measurement: nothing more is started on the GPU
            sys.exit("%s exited with %d" % (run_name(c, xg), rc))


if __name__ == "__main__":
    main()
