"""Shared by test_gradnorm_cpu.py / test_gradnorm_gpu.py: the work-item table restated in Python, float64 references in numpy, and thin
callers of spair_grad_norm / spair_adam_guarded / spair_adam_clipped on torch tensors."""
import ctypes

import numpy as np

ERR_SHAPE = -1
NORM_RTOL = 1e-6         # contract (c): float64 accumulation (< 1e-9 for n <= 2^21 terms) + one fp32 rounding of the result (6e-8), x 10


def i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def items_ref(seg_lo, seg_hi, chunk):
    """include/spair_hip.h: every segment cut into pieces of at most ``chunk`` floats, segments in order, pieces in order."""
    out = []
    for s, (lo, hi) in enumerate(zip(seg_lo, seg_hi)):
        while lo < hi:
            out += [s, lo, min(lo + chunk, hi)]
            lo += chunk
    return out


def items_lib(lib, seg_lo, seg_hi, n):
    """(count, table) from spair_grad_norm_items: the count-only call first, then the filling call; both must agree."""
    nseg = len(seg_lo)
    k = lib.spair_grad_norm_items(i64(seg_lo), i64(seg_hi), nseg, n, None)
    if k < 0:
        return k, None
    table = (ctypes.c_int64 * (3 * k))()
    assert lib.spair_grad_norm_items(i64(seg_lo), i64(seg_hi), nseg, n, table) == k
    return k, list(table)


def norm64(a):
    a = np.asarray(a).astype(np.float64)
    return float(np.sqrt((a * a).sum()))


def layout(lengths, gaps, start=0):
    """Segments of the given lengths, gaps[i] elements in front of segment i, from ``start``: ([(lo, hi)], elements needed)."""
    segs, at = [], start
    for ln, gap in zip(lengths, gaps):
        at += gap
        segs.append((at, at + ln))
        at += ln
    return segs, at


class GradNormCall:
    """spair_grad_norm on a device buffer and a segment list; the outputs stay on the device (``out``, ``seg_sumsq``, ``partial``,
    ``clip`` accumulate over calls of the same object, as the ABI says)."""

    def __init__(self, buf, segs):
        import torch
        from spair_pytorch_amd import _lib as L
        self.L, self.buf, self.nseg = L, buf, len(segs)
        k, table = items_lib(L.lib(), [s[0] for s in segs], [s[1] for s in segs], buf.numel())
        assert k > 0 and table == items_ref([s[0] for s in segs], [s[1] for s in segs], L.lib().spair_grad_chunk())
        dev = buf.device
        self.n_items = k
        self.items = torch.tensor(table, dtype=torch.int64).to(dev)
        self.partial = torch.zeros(k, dtype=torch.float64, device=dev)
        self.seg_sumsq = torch.zeros(self.nseg, dtype=torch.float64, device=dev)
        self.out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.clip = torch.zeros(2, dtype=torch.int32, device=dev)

    def __call__(self, max_norm=0.0, norm_eps=1e-6):
        L = self.L
        L.check(L.lib().spair_grad_norm(L.ptr(self.buf), L.ptr(self.items), self.n_items, self.nseg, L.ptr(self.partial),
                                        L.ptr(self.seg_sumsq), L.ptr(self.out), float(max_norm), float(norm_eps), L.ptr(self.clip),
                                        L.stream()), "spair_grad_norm")
        return self


def adam(p, g, m, v, step, lr=1e-3, skip=None, counters=None, norm_out=None):
    """spair_adam_clipped with ``norm_out`` (a device float[2]), else spair_adam_guarded; torch.optim.Adam's default betas and eps."""
    from spair_pytorch_amd import _lib as L
    args = [L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), ctypes.c_int64(p.numel())] + [ctypes.c_float(f) for f in (lr, 0.9, 0.999, 1e-8)]
    args += [int(step), L.ptr(skip), L.ptr(counters)]
    if norm_out is None:
        L.check(L.lib().spair_adam_guarded(*args, L.stream()), "spair_adam_guarded")
    else:
        L.check(L.lib().spair_adam_clipped(*args, L.ptr(norm_out), L.stream()), "spair_adam_clipped")
