"""Cost of SPAIR.parse (bf16 model) at the BASELINE configs[1] (B = 256, 128 x 128, 16 x 16 cells) and configs[3] (B = 64, 256 x 256,
32 x 32 cells) geometries:
  * the owner kernel (k_render_owner, spair_render_owner) beside the first-generation forward renderer (k_render_fwd: spair_render_fwd16 on
    fp16 sprites, spair_render_fwd on fp32 sprites) ON THE SAME OPERANDS: the sprites, boxes, presences and depths a posterior-mean forward
    left in the workspace.  The sprite copy both kernels read starts 8 bytes off a 16-byte boundary: the unit entry points run the second
    generation on 16-byte-aligned sprites and the first generation otherwise, and the first generation is the yardstick here;
  * the whole parse() call against a no_grad forward() of the same batch.
Device-event times are printed; for the per-kernel figures run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_parse.py`."""
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


def off16(t):
    """A copy of the 2-D tensor t whose first element lies 8 bytes past a 16-byte boundary (same row stride)."""
    es = t.element_size()
    buf = torch.empty(t.numel() + 16 // es, dtype=t.dtype, device=t.device)
    shift = ((8 - buf.data_ptr()) % 16) // es
    out = buf[shift:shift + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel")
    ap.add_argument("--calls", type=int, default=50, help="parse() / forward() calls")
    args = ap.parse_args()
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import SPAIR
    dev = torch.device("cuda")
    for label, I, B in (("configs[1]", 128, 256), ("configs[3]", 256, 64)):
        cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
        torch.manual_seed(3)
        m = SPAIR([1, I, I], None, dev, compute_dtype="bf16").to(dev)
        x = torch.from_numpy(scattered_digits(1234, B, I, 11)[0]).to(dev)
        r = m.parse(x, 2000, threshold=0.25)
        G, P = r.z_where.shape[2], int(cfg.OBJECT_SHAPE[0])
        HW = G * G
        rows = m.cell_rows()
        S16 = m.workspace_view("S", padded=True)
        assert S16.dtype == torch.float16
        ld = S16.shape[1]
        # the rows' operands, in row order r = cprime * B + b (what the renderer reads), from the maps parse returned
        order = torch.argsort(rows.long())                                   # cell k of row block cprime
        to_rows = lambda v: v.permute(2, 3, 0, 1).reshape(HW, B, -1)[order].reshape(HW * B, -1).contiguous()
        nbox, pres, depth = to_rows(r.z_where), to_rows(r.z_pres).reshape(-1), to_rows(r.z_depth).reshape(-1)
        recon, aux = torch.empty(B, 1, I, I, device=dev), torch.empty(B * I * I * 2, device=dev)
        bce = torch.empty(B * ((I + 15) // 16) ** 2, device=dev)
        out = None
        for s16, S in ((1, off16(S16)), (0, off16(S16.float()))):
            fwd = L.lib().spair_render_fwd16 if s16 else L.lib().spair_render_fwd
            fwd.restype = ctypes.c_int

            def run_fwd():
                L.check(fwd(L.ptr(S), ld, L.ptr(nbox), L.ptr(pres), L.ptr(depth), L.ptr(x), L.ptr(recon), L.ptr(aux), L.ptr(bce), B, HW, 1, I,
                            P, 0, L.stream()), "spair_render_fwd")

            def run_owner():
                nonlocal out
                out = L.render_owner(S[:, :P * P * 2], 2, nbox, pres, depth, B, HW, I, I, P, False, 0.25, rows)

            t_fwd, t_own = timed(run_fwd, args.reps), timed(run_owner, args.reps)
            same = s16 and all(torch.equal(a, b) for a, b in zip(out, (r.owner, r.owner_weight, r.coverage, r.area)))
            print("%s %s sprites: k_render_fwd %.4f ms, k_render_owner (+ area memset, 4 output allocations) %.4f ms%s"
                  % (label, "fp16" if s16 else "fp32", t_fwd, t_own, "; equal to parse()'s" if same else ""), flush=True)
            assert not s16 or same
            assert (recon - r.recon).abs().max().item() < 2e-3      # (the step's forward ran the matrix-core renderer)

        def fwd_call():
            with torch.no_grad():
                m(x, 2000)

        t_f, t_p = timed(fwd_call, args.calls, 5), timed(lambda: m.parse(x, 2000, threshold=0.25), args.calls, 5)
        print("%s: no_grad forward() %.4f ms, parse() %.4f ms (+%.4f)" % (label, t_f, t_p, t_p - t_f), flush=True)
        del m, S16, S, r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
