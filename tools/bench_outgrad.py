"""Cost of SPAIR(..., differentiable_outputs=True) on the benchmark step (128x128, 16x16 grid, B=256, bf16): ms per zero_grad + forward +
backward + Adam for (a) the default model, (b) the switch on with only loss.backward(), (c) the switch on with a user term on all three
outputs.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_outgrad.py`."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import SPAIR
    from spair_pytorch_amd.optim import FusedAdam
    I, B = 128, args.batch
    cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
    dev = torch.device("cuda")
    x = torch.from_numpy(scattered_digits(1234, B, I, 11)[0]).to(dev)
    for mode in ("default", "switch_on_loss_only", "switch_on_loss_plus_outputs"):
        torch.manual_seed(3)
        m = SPAIR([1, I, I], None, dev, compute_dtype="bf16", differentiable_outputs=mode != "default").to(dev)
        opt = FusedAdam(m, lr=1e-4)
        W = None
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for it in range(args.warmup + args.steps):
            if it == args.warmup:
                torch.cuda.synchronize()
                ev[0].record()
            opt.zero_grad()
            loss, recon, z_where, z_pres = m(x, 2000 + it)
            if mode == "switch_on_loss_plus_outputs":
                if W is None:
                    g = torch.Generator(device=dev).manual_seed(1)
                    W = [torch.rand(t.shape, generator=g, device=dev) for t in (recon, z_where, z_pres)]
                loss = loss + (W[0] * recon).sum() + (W[1] * z_where).sum() + (W[2] * z_pres).sum()
            loss.backward()
            opt.step()
        ev[1].record()
        torch.cuda.synchronize()
        print("%-28s %.4f ms/step" % (mode, ev[0].elapsed_time(ev[1]) / args.steps), flush=True)
        del m, opt


if __name__ == "__main__":
    main()
