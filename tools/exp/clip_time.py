"""What clipping by the global gradient norm costs on the benchmark model (BASELINE configs[1]: 128x128, 16x16 grid, batch 256, bf16):
FusedAdam.step() alone and the whole step (zero_grad + forward + backward + Adam), without max_grad_norm, with it (spair_grad_norm +
spair_adam_clipped) and, for comparison, with torch.nn.utils.clip_grad_norm_ in front of the plain step.  Device events around 200
iterations after 20 warm-up iterations, three repeats per timing, the median reported (all three printed).
usage (GPU box): python tools/exp/clip_time.py [opt-plain|opt-clipped|opt-torch|step-plain|step-clipped|step-torch ...]   (default: all,
the repeats of the chosen timings alternating; one timing per process keeps each under its own time limit)"""
import json
import sys

import torch

sys.path.insert(0, ".")
from spair_pytorch_amd import config as cfg, models                    # noqa: E402
from spair_pytorch_amd.data import scattered_digits                    # noqa: E402
from spair_pytorch_amd.optim import FusedAdam                          # noqa: E402

ITERS, WARMUP, REPEATS = 200, 20, 3
MODES = ("opt-plain", "opt-clipped", "opt-torch", "step-plain", "step-clipped", "step-torch")
modes = sys.argv[1:] or list(MODES)
assert all(m in MODES for m in modes), modes

I, B = 128, 256
cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
torch.manual_seed(3)
model = models.SPAIR([1, I, I], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
x = torch.from_numpy(scattered_digits(1234, B, I, 11)[0]).cuda()
torch.manual_seed(7)
model.flat_gradients().zero_()
model(x, 2000)[0].backward()
norm = model.flat_gradients().double().norm().item()
params = [p for p in model.parameters()]
print("gradient norm of the first step %.4f over %d floats; clipping at half of it" % (norm, model.flat_gradients().numel()), flush=True)


def make(mode):
    what, how = mode.split("-")
    kw = dict(max_grad_norm=0.5 * norm) if how == "clipped" else {}          # lr = 0: every iteration sees the same parameters
    opt = FusedAdam(model, lr=0.0, **kw)

    def adam():
        if how == "torch":
            torch.nn.utils.clip_grad_norm_(params, 0.5 * norm)
        opt.step()

    def step():
        opt.zero_grad()
        model(x, 2000)[0].backward()
        adam()

    return adam if what == "opt" else step


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3                                        # us per iteration


fns = {m: make(m) for m in modes}
for m in modes:
    timed(fns[m], WARMUP)
reps = {m: [] for m in modes}
for _ in range(REPEATS):
    for m in modes:
        reps[m].append(timed(fns[m], ITERS))
for m in modes:
    print(json.dumps(dict(timing=m, us_median=round(sorted(reps[m])[REPEATS // 2], 2), us_repeats=[round(v, 2) for v in reps[m]],
                          iterations=ITERS, warmup=WARMUP)), flush=True)
