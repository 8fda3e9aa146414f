"""Step time of a rectangular image ([1,128,96], reference topology: an 11 x 8 grid) against the square [1,128,128] (11 x 11) on the same
launches -- the per-wavefront per-cell step (SpairStep.flags bit 0), first-generation renderer, implicit-GEMM backbone -- in both dtypes.
The square image is forced onto the rectangular step's kernels too (flags bit 5: no patch-resident convs) so that only the geometry differs;
its records / matrix-core renderer stay, which the rectangular image cannot take.
usage (GPU box): python tools/exp/rect_time.py [batch]"""
import sys, time, torch
sys.path.insert(0, ".")
from spair_pytorch_amd import config as cfg, models
from spair_pytorch_amd.optim import FusedAdam
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
models.STEP_FLAGS = 1 | 32
for dt in ("bf16", "f32"):
    for H, W in ((128, 96), (128, 128)):
        cfg.set_grid(H, (3, 2, 2, 1, 1, 1), image_width=W)
        torch.manual_seed(3)
        m = models.SPAIR([1, H, W], None, torch.device("cuda"), compute_dtype=dt).to("cuda")
        opt = FusedAdam(m, lr=1e-4)
        g = torch.Generator(device="cuda").manual_seed(1)
        x = (torch.rand(B, 1, H, W, device="cuda", generator=g) > 0.9).float() * torch.rand(B, 1, H, W, device="cuda", generator=g)
        def step():
            opt.zero_grad(); loss, *_ = m(x, 2000); loss.backward(); opt.step(); return loss
        for _ in range(3): step()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        n = 10
        for _ in range(n): l = step()
        torch.cuda.synchronize(); ms = (time.perf_counter() - t0) / n * 1e3
        print("%s B=%d %dx%d: %.2f ms/step, loss %.1f" % (dt, B, H, W, ms, float(l.detach())), flush=True)
        del m, opt
