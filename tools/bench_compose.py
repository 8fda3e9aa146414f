"""Cost of SPAIR.compose (bf16 model) at the BASELINE configs[1] (B = 256, 128 x 128, 16 x 16 cells) and configs[3] (B = 64, 256 x 256,
32 x 32 cells) geometries, on the scene a posterior-mean parse of the batch returns:
  * the whole compose() call (no layers, and with K = 8 layers) against a no_grad forward() of the same model, by device events;
  * spair_compose and spair_render_layers alone (the C entry points on preallocated outputs);
  * the layer kernel's yardstick: the first-generation forward renderer k_render_fwd (spair_render_fwd16) on the same sprites and rows,
    scaled by K / (G * Gw) -- the layer kernel visits K cells per pixel where the renderer visits all of them.
Device-event times are printed; for the per-kernel figures (k_latents_import, k_render_layers) run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_compose.py`."""
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
    ap.add_argument("--calls", type=int, default=50, help="compose() / forward() calls")
    ap.add_argument("--layers", type=int, default=8, help="K")
    args = ap.parse_args()
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd import models
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import SPAIR
    dev = torch.device("cuda")
    K = args.layers
    for label, I, B in (("configs[1]", 128, 256), ("configs[3]", 256, 64)):
        cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
        torch.manual_seed(3)
        m = SPAIR([1, I, I], None, dev, compute_dtype="bf16").to(dev)
        x = torch.from_numpy(scattered_digits(1234, B, I, 11)[0]).to(dev)
        p = m.parse(x, 2000, threshold=0.25)
        G, P = p.z_where.shape[2], int(cfg.OBJECT_SHAPE[0])
        HW = G * G
        cells = torch.argsort(p.area, dim=1, descending=True, stable=True)[:, :K].to(torch.int32).contiguous()
        r = m.compose(p, layers=cells)
        assert torch.equal(r.recon, p.recon)

        def fwd_call():
            with torch.no_grad():
                m(x, 2000)

        t_f = timed(fwd_call, args.calls, 5)
        t_c = timed(lambda: m.compose(p), args.calls, 5)
        t_cl = timed(lambda: m.compose(p, layers=cells), args.calls, 5)
        print("%s: no_grad forward() %.4f ms, compose() %.4f ms, compose(layers=[B,%d]) %.4f ms" % (label, t_f, t_c, K, t_cl), flush=True)
        # the entry points alone, on preallocated outputs
        e = m._last_engine()
        d, ws = e["dims"], e["workspace"]
        recon, inv_den = torch.empty(B, 1, I, I, device=dev), torch.empty(B, I, I, device=dev)
        layers, weight = torch.empty(B, K, 1, I, I, device=dev), torch.empty(B, K, I, I, device=dev)
        lat = [t.contiguous() for t in (p.z_where, p.z_what, p.z_depth, p.z_pres)]

        def run_compose():
            L.check(L.lib().spair_compose(ctypes.byref(d), L.ptr(m.flat_parameters()), L.ptr(ws), int(models.STEP_FLAGS), *(L.ptr(t) for t in lat),
                                          L.ptr(recon), L.ptr(inv_den), L.stream()), "spair_compose")

        def run_layers():
            L.check(L.lib().spair_render_layers(ctypes.byref(d), L.ptr(ws), int(models.STEP_FLAGS), L.ptr(cells), K, L.ptr(inv_den), L.ptr(layers),
                                                L.ptr(weight), L.stream()), "spair_render_layers")

        t_sc, t_sl = timed(run_compose, args.reps), timed(run_layers, args.reps)
        assert torch.equal(layers, r.layers) and torch.equal(weight, r.layer_weight)
        # the yardstick: k_render_fwd on the same sprites and rows (a copy 8 bytes off a 16-byte boundary selects the first generation)
        S16 = m.workspace_view("S", padded=True)
        ld, es = S16.shape[1], S16.element_size()
        buf = torch.empty(S16.numel() + 16 // es, dtype=S16.dtype, device=dev)
        shift = ((8 - buf.data_ptr()) % 16) // es
        S = buf[shift:shift + S16.numel()].view(S16.shape)
        S.copy_(S16)
        order = torch.argsort(m.cell_rows().long())
        to_rows = lambda v: v.permute(2, 3, 0, 1).reshape(HW, B, -1)[order].reshape(HW * B, -1).contiguous()
        nbox, pres, depth = to_rows(p.z_where), to_rows(p.z_pres).reshape(-1), to_rows(p.z_depth).reshape(-1)
        aux, bce = torch.empty(B * I * I * 2, device=dev), torch.empty(B * ((I + 15) // 16) ** 2, device=dev)
        fwd = L.lib().spair_render_fwd16
        fwd.restype = ctypes.c_int

        def run_fwd():
            L.check(fwd(L.ptr(S), ld, L.ptr(nbox), L.ptr(pres), L.ptr(depth), L.ptr(x), L.ptr(recon), L.ptr(aux), L.ptr(bce), B, HW, 1, I, P, 0,
                        L.stream()), "spair_render_fwd16")

        t_fwd = timed(run_fwd, args.reps)
        yard = t_fwd * K / HW
        gb = B * K * 2 * I * I * 4 / 1e9
        print("%s: spair_compose %.4f ms, spair_render_layers (K = %d) %.4f ms = %.0f GB/s of its %.3f GB of stores; k_render_fwd %.4f ms, "
              "scaled by K / (G Gw) = %d / %d: %.4f ms, ratio %.1f" % (label, t_sc, K, t_sl, gb / (t_sl * 1e-3), gb, t_fwd, K, HW, yard,
                                                                       t_sl / yard), flush=True)
        del m, S16, S, buf, p, r, layers, weight
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
