"""What the float64 checks of the HIP kernels share: the derived accumulation bound, the round-to-nearest-even interval check of a bf16
output, the ReLU gate, the sensitivity checks that prove a bound non-vacuous on reference data, and (for the standalone kernel tests) an
output buffer that shows every write outside its block and a set of gate values on which "> 0" can go wrong.

Bound (derived, not measured): an fp32 chain of <= 2048 terms plus a <= 64-way split reduce has a worst-case error of
(2048 + 64) 2^-24 < 2^-12 of the terms' absolute sum; U is that factor.

Used by tests/test_step_operands_gpu.py (whole steps, on the stored operands) and tests/test_gemm16_edges_gpu.py (the C-ABI entry points of
the bf16 matrix kernels at their tile edges)."""
import math

import torch

U = 2.0 ** -12           # the accumulation bound's factor


def rne16(t):
    """float64 -> bf16, round to nearest even (through fp32: the double rounding only moves a value within 2^-24 of its magnitude, far inside
    every bound below)."""
    return t.float().to(torch.bfloat16)


def d64(t):
    return t.double()


class Record:
    def __init__(self, name):
        self.name, self.ratio, self.bad, self.notes = name, {}, [], []
        self.covered = set()          # parameters whose gradient was checked

    def ratio_max(self, key, r):
        self.ratio[key] = max(self.ratio.get(key, 0.0), float(r))
        if not r <= 1.0:
            self.bad.append((key, float(r)))

    def fail(self, key, what):
        self.bad.append((key, what))

    def report(self):
        print("\n[%s]" % self.name)
        for k, r in self.ratio.items():
            print("  %-46s %.3g" % (k, r))
        for n in self.notes:
            print("  " + n)


def _sensitivity(rec, key, ref, bound, drop):
    """The bound must reject the reference with 1/32 of its rows removed (`drop`: their contribution) and with its 8-column blocks shifted by
    one block (column j read from j + 8; a matrix of fewer than 16 columns -- a grey 3x3 stem's 9 -- has no second block: the rows only)."""
    c = ref.shape[1] // 8 * 8 - 8
    r_drop = float((drop.abs() / bound).max())
    r_shift = float(((ref[:, 8:8 + c] - ref[:, 0:c]).abs() / bound[:, 0:c]).max()) if c > 0 else math.inf
    if not (r_drop > 1 and r_shift > 1):
        rec.fail(key, "vacuous bound (drop %.3g, shift %.3g)" % (r_drop, r_shift))


def _bias_sensitivity(rec, key, ref, bound, drop):
    """The same for a bias bound (a vector): the dropped rows always, the shifted 8-element block where the bias has 16 elements or more
    (the heads' 1, 2 and 8 have no second block)."""
    r_drop = float((drop.abs() / bound).max())
    c = ref.numel() // 8 * 8 - 8
    r_shift = float(((ref[8:8 + c] - ref[0:c]).abs() / bound[0:c]).max()) if c > 0 else math.inf
    if not (r_drop > 1 and r_shift > 1):
        rec.fail(key, "vacuous bound (drop %.3g, shift %.3g)" % (r_drop, r_shift))


def lin_wgrad(rec, key, grad_w, grad_b, dY, X, round_ops, chunk=16384):
    """grad_w[out, in] = sum_r dY[r, out] X[r, in], grad_b = sum_r dY[r, :] in float64 (GPU), against the kernel's."""
    R = dY.shape[0]
    rdrop = R // 32          # one row split's worth of rows (1/32), from the middle: rows R/2 ..
    ra = R // 2
    acc = torch.zeros(dY.shape[1], X.shape[1], dtype=torch.float64, device=dY.device)
    absb, drop = torch.zeros_like(acc), torch.zeros_like(acc)
    bsum = torch.zeros(dY.shape[1], dtype=torch.float64, device=dY.device)
    babs, bdrop = torch.zeros_like(bsum), torch.zeros_like(bsum)
    for r0 in range(0, R, chunk):
        a, b = dY[r0:r0 + chunk], X[r0:r0 + chunk]
        a32 = d64(a)            # (the bias gradient sums dY as loaded, before any rounding: gemm.hip's column sums)
        if round_ops:
            a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
        a, b = d64(a), d64(b)
        acc += a.T @ b
        absb += a.abs().T @ b.abs()
        bsum += a32.sum(0)
        babs += a32.abs().sum(0)
        d0, d1 = max(ra - r0, 0), min(ra + rdrop - r0, a.shape[0])
        if d1 > d0:
            drop += a[d0:d1].T @ b[d0:d1]
            bdrop += a32[d0:d1].sum(0)
    bound = U * absb + 1e-30
    rec.ratio_max(key + ".weight", ((d64(grad_w) - acc).abs() / bound).max())
    _sensitivity(rec, key + ".weight", acc, bound, drop)
    bb = U * babs + 1e-30
    rec.ratio_max(key + ".bias", ((d64(grad_b) - bsum).abs() / bb).max())
    _bias_sensitivity(rec, key + ".bias", bsum, bb, bdrop)
    rec.covered |= {key + ".weight", key + ".bias"}


def gate_of(a):
    """The ReLU gate of a data gradient from the stored activation a: a > 0.  -0.0 and +0.0 are off, a positive bf16 denormal is on --
    whether the kernel reads the value or the sign bits its forward left.  Also returns how many of each the data holds."""
    neg0 = int(((a == 0) & torch.signbit(a)).sum())
    den = int(((a != 0) & (a.abs() < 2.0 ** -126)).sum())
    return a > 0, neg0, den


def check_out(rec, key, got, ref, beta, relu=False, gate=None, part=None):
    """A bf16 output must lie in [RNE(f(ref - beta)), RNE(f(ref + beta))] (f: the ReLU where the kernel applies one; RNE is monotone, so
    this is 'RNE of the float64 value, either neighbour only within beta of a rounding boundary'); an fp32 output within beta + 2^-24 |ref|.
    gate: (mask, -0.0 count, denormal count) of gate_of; where the mask is False the output must be exactly 0.  Sensitivity: the accepted
    set must exclude the reference with its channels shifted by one 8-column block (channel j read from j + 8) and, where `part` is given
    (the contribution of one block of 8 summed input channels), the reference without that block."""
    f = (lambda t: t.clamp_min(0)) if relu else (lambda t: t)
    note = ""
    if gate is not None:
        mask, neg0, den = gate
        ref, beta = ref * mask, beta * mask
        part = part * mask if part is not None else None
        off = ~mask
        if bool((got[off] != 0).any()):
            rec.fail(key, "%d gated-off elements are not 0" % int((got[off] != 0).sum()))
        note = "; gate read %d -0.0 and %d bf16-denormal activations" % (neg0, den)
    shifted = ref.clone()
    shifted[..., :-8] = ref[..., 8:]
    wrong = [("shift", shifted)] + ([("drop", ref - part)] if part is not None else [])
    if got.dtype == torch.bfloat16:
        lo, hi = rne16(f(ref - beta)).double(), rne16(f(ref + beta)).double()
        g = d64(got)
        bad = (g < lo) | (g > hi)
        nbad = int(bad.sum())
        near = int((got != rne16(f(ref))).sum())
        if nbad:
            rec.fail(key, "%d bf16 elements outside [RNE(ref - beta), RNE(ref + beta)]" % nbad)
        for what, w in wrong:
            r = rne16(f(w)).double()
            if not bool(((r < lo) | (r > hi)).any()):
                rec.fail(key, "vacuous bound (%s)" % what)
        rec.notes.append("%s: %d of %d elements differ from RNE(ref), all within beta of a rounding boundary%s" % (key, near, got.numel(), note)
                         if not nbad else "%s: %d elements outside" % (key, nbad))
    else:
        bound = beta + 2.0 ** -24 * ref.abs() + 1e-30
        rec.ratio_max(key, ((d64(got) - f(ref)).abs() / bound).max())
        for what, w in wrong:
            if not float(((f(w) - f(ref)).abs() / bound).max()) > 1:
                rec.fail(key, "vacuous bound (%s)" % what)
        if note:
            rec.notes.append(key + note)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# for the standalone kernel tests
# ---------------------------------------------------------------------------------------------------------------------------------------------
def hold(rec, key, got, ref, beta, relu=False, gate=None, part=None):
    """check_out for an output of any width.  check_out always asks its bound to reject the reference shifted by one 8-column block; an
    output of fewer than 16 columns has no second block to shift in (as _sensitivity says of narrow matrices), so for those that one
    finding is dropped -- the interval check itself, the exact zeros of the gate and the dropped block (`part`) hold as they are."""
    n0 = len(rec.bad)
    check_out(rec, key, got, ref, beta, relu=relu, gate=gate, part=part)
    if ref.shape[-1] < 16:
        rec.bad[n0:] = [b for b in rec.bad[n0:] if b != (key, "vacuous bound (shift)")]


SENTINEL = -7.0          # finite, never 0, exact in bf16 and fp32: an element the kernel never wrote does not read as a plausible 0


class Guarded:
    """An output [rows][cols] in rows of leading dimension ld, with one guard row behind the last: everything is filled with SENTINEL
    (the block itself with `inside`, where the kernel accumulates into it).  check() asserts that every byte outside the block still
    holds the fill."""

    def __init__(self, rows, cols, ld, dtype, device="cuda", inside=None):
        assert ld >= cols
        self.rows, self.cols, self.ld = rows, cols, ld
        self.full = torch.full((rows + 1, ld), SENTINEL, dtype=dtype, device=device)
        self.block = self.full[:rows, :cols]
        if inside is not None:
            self.block.fill_(inside)
        self.bits = torch.int16 if dtype == torch.bfloat16 else torch.int32

    def data_ptr(self):
        return self.full.data_ptr()

    def outside_untouched(self):
        want = torch.full_like(self.full, SENTINEL)
        got = self.full.clone()
        got[:self.rows, :self.cols] = SENTINEL
        return torch.equal(got.view(self.bits), want.view(self.bits))

    def check(self, rec, key):
        if not self.outside_untouched():
            rec.fail(key, "wrote outside its [%d][%d] block (guard row or pad columns of ld %d)" % (self.rows, self.cols, self.ld))

    def unwritten(self):
        """How many elements of the block still hold the fill bit for bit."""
        s = torch.full((), SENTINEL, dtype=self.full.dtype, device=self.full.device)
        return int((self.block.contiguous().view(self.bits) == s.view(self.bits)).sum())


def bf16_denormal():
    """The smallest positive bf16 denormal, 2^-133 (bits 0x0001)."""
    return torch.tensor([1], dtype=torch.int16).view(torch.bfloat16)[0]


def plant_special_gates(mask):
    """Plants the values on which a "> 0" test can go wrong into the 2-D gate / mask tensor `mask` (CPU, bf16 or fp32; a view of the valid
    [rows][cols] block): +0.0, -0.0 (off), the smallest positive bf16 denormal (on) and the smallest negative one (off), for fp32 also
    1e-40 (on) and -1e-40 (off).  Positions, fixed: counted back from the last element of the last valid row (so the last valid row and
    the last valid column hold the positive denormal), forward from the first element, and from the start of the middle row.  Returns
    [(row, col, on)]; the expected gate is IEEE value > 0."""
    rows, cols = mask.shape
    den = float(bf16_denormal())
    vals = [(den, True), (0.0, False), (-0.0, False), (-den, False)]
    if mask.dtype == torch.float32:
        vals += [(1e-40, True), (-1e-40, False)]
    n = rows * cols
    assert n >= len(vals), "mask too small for the special values"
    flat = []
    for i, (v, on) in enumerate(vals):
        flat.append((n - 1 - i, v, on))
    if n >= 3 * len(vals) + cols:
        for i, (v, on) in enumerate(vals):
            flat.append((i, v, on))
            flat.append(((rows // 2) * cols + i, v, on) if rows >= 4 else (len(vals) + i, v, on))
    out = []
    for f, v, on in flat:
        r, c = f // cols, f % cols
        mask[r, c] = v
        got = float(mask[r, c])       # (1e-40 is stored as the nearest fp32 denormal: it must not have become 0, nor a zero lost its sign)
        assert (got != 0) == (v != 0) and math.copysign(1.0, got) == math.copysign(1.0, v), "special value lost on the way into the mask"
        out.append((r, c, on))
    return out


def special_gate(mask, planted):
    """gate_of on the CPU copy of `mask` (IEEE comparisons, denormals kept), checked at the planted positions; returned on `mask`'s device."""
    m, neg0, den = gate_of(mask.cpu())
    for r, c, on in planted:
        assert bool(m[r, c]) == on, (r, c, on)
    assert neg0 >= 1 and den >= 2
    return m.to(mask.device), neg0, den
