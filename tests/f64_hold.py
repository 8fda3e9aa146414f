"""What the float64 checks of the HIP kernels share: the derived accumulation bound, the round-to-nearest-even interval check of a bf16
output, the ReLU gate, the sensitivity checks that prove a bound non-vacuous on reference data, and (for the standalone kernel tests) an
output buffer that shows every write outside its block and a set of gate values on which "> 0" can go wrong.

Bound (derived, not measured): an fp32 chain of <= 2048 terms plus a <= 64-way split reduce has a worst-case error of
(2048 + 64) 2^-24 < 2^-12 of the terms' absolute sum; U is that factor.

Used by tests/test_step_operands_gpu.py (whole steps, on the stored operands), tests/test_gemm16_edges_gpu.py (the C-ABI entry points of
the bf16 matrix kernels at their tile edges), tests/test_patch_edges_gpu.py and tests/test_decoder_edges_gpu.py (the patch-resident
convolutions, the stem and the fused decoder kernels; for those also the fp16 interval of a sigmoid output, the float64 convolutions and
the Python mirror of the patch-resident launchers' tiling, which tests/test_patch_tiling_cpu.py holds to the library's own answer)."""
import math

import numpy as np
import torch

U = 2.0 ** -12           # the accumulation bound's factor


def rne16(t):
    """float64 -> bf16, round to nearest even (through fp32: the double rounding only moves a value within 2^-24 of its magnitude, far inside
    every bound below)."""
    return t.float().to(torch.bfloat16)


def rne_f16(t):
    """float64 -> fp16, round to nearest even, fp16 denormals kept (through fp32, as rne16)."""
    return t.float().to(torch.float16)


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


def _cell16(got):
    """The rounding cell of each 16-bit float (bf16 or fp16) in `got`, as float64 (lower edge, upper edge): the midpoints to its two
    neighbours in the format (+-0 is one value; its neighbours are the smallest denormals)."""
    dt = got.dtype
    bits = got.contiguous().view(torch.int16).to(torch.int32) & 0xffff
    mag = bits & 0x7fff
    neg = (bits >= 0x8000) & (mag != 0)

    def val(b):
        return (((b + 0x8000) % 0x10000) - 0x8000).to(torch.int16).view(dt).double()

    up = val(torch.where(neg, (mag - 1) | 0x8000, mag + 1))
    down = val(torch.where(neg, (mag + 1) | 0x8000, torch.where(mag == 0, torch.full_like(mag, 0x8001), mag - 1)))
    g = got.double()
    return (g + down) / 2, (g + up) / 2


def beta_needed(got, ref, relu=False):
    """How far the float64 value `ref` (before the ReLU, where there is one) lies from the nearest value that rounds to the stored 16-bit
    `got`: 0 where got = RNE(f(ref)), else the distance to the edge of got's rounding cell -- the part of beta that element used."""
    lo, hi = _cell16(got)
    if relu:
        lo = torch.where(got == 0, torch.full_like(lo, -math.inf), lo)          # every pre-activation <= 0 is stored as 0
    return torch.maximum(torch.maximum(lo - ref, ref - hi), torch.zeros_like(ref))


def check_out(rec, key, got, ref, beta, relu=False, gate=None, part=None, f32_slack=2.0 ** -24):
    """A bf16 (or fp16) output must lie in [RNE(f(ref - beta)), RNE(f(ref + beta))] (f: the ReLU where the kernel applies one; RNE is monotone, so
    this is 'RNE of the float64 value, either neighbour only within beta of a rounding boundary'); an fp32 output within beta + 2^-24 |ref|
    (f32_slack = 0 where beta already covers the stored value's own rounding).
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
    if got.dtype in (torch.bfloat16, torch.float16):
        rnd = rne16 if got.dtype == torch.bfloat16 else rne_f16
        lo, hi = rnd(f(ref - beta)).double(), rnd(f(ref + beta)).double()
        g = d64(got)
        bad = (g < lo) | (g > hi)
        nbad = int(bad.sum())
        near = int((got != rnd(f(ref))).sum())
        if nbad:
            rec.fail(key, "%d 16-bit elements outside [RNE(ref - beta), RNE(ref + beta)]" % nbad)
        for what, w in wrong:
            r = rnd(f(w)).double()
            if not bool(((r < lo) | (r > hi)).any()):
                rec.fail(key, "vacuous bound (%s)" % what)
        rec.notes.append("%s: %d of %d elements differ from RNE(ref), all within beta of a rounding boundary%s" % (key, near, got.numel(), note)
                         if not nbad else "%s: %d elements outside" % (key, nbad))
        # the figure (a record, not a second threshold): the largest part of its beta an element needed to reach the stored value
        need = beta_needed(got, ref, relu)
        used = need > 0
        k2 = key + ": beta needed / beta"
        rec.ratio[k2] = max(rec.ratio.get(k2, 0.0), float((need[used] / beta[used]).max()) if bool(used.any()) else 0.0)
    else:
        bound = beta + f32_slack * ref.abs() + 1e-30
        rec.ratio_max(key, ((d64(got) - f(ref)).abs() / bound).max())
        for what, w in wrong:
            if not float(((f(w) - f(ref)).abs() / bound).max()) > 1:
                rec.fail(key, "vacuous bound (%s)" % what)
        if note:
            rec.notes.append(key + note)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# for the standalone kernel tests
# ---------------------------------------------------------------------------------------------------------------------------------------------
def hold(rec, key, got, ref, beta, relu=False, gate=None, part=None, f32_slack=2.0 ** -24):
    """check_out for an output of any width.  check_out always asks its bound to reject the reference shifted by one 8-column block; an
    output of fewer than 16 columns has no second block to shift in (as _sensitivity says of narrow matrices), so for those that one
    finding is dropped -- the interval check itself, the exact zeros of the gate and the dropped block (`part`) hold as they are."""
    n0 = len(rec.bad)
    check_out(rec, key, got, ref, beta, relu=relu, gate=gate, part=part, f32_slack=f32_slack)
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
        self.bits = torch.int16 if dtype in (torch.bfloat16, torch.float16) else torch.int32

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


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the fp16 interval of an analytic sigmoid
# ---------------------------------------------------------------------------------------------------------------------------------------------
SIG_REL = 2.0 ** -21     # 8 fp32 ulps: v_exp_f32, the add of 1 and v_rcp_f32 at 1 ulp each, with margin


def sig2(u):
    """1 / (1 + 2^u) in float64 (u = +inf gives 0, u = -inf gives 1)."""
    return 1.0 / (1.0 + torch.exp2(u))


def check_sigmoid16(rec, key, got, u, beta, wrong):
    """An fp16 output s = 1 / (1 + exp2(u)) whose exp2 argument the kernel accumulated in fp32: u is its float64 value, beta the derived
    bound of the accumulation.  The sigmoid is monotone DECREASING in u and RNE is monotone, so the accepted set is
    [RNE16(sig(u + beta) (1 - SIG_REL)), RNE16(sig(u - beta) (1 + SIG_REL))].  `wrong`: [(name, u')] subtly wrong exp2 arguments, each of
    which must put at least one element outside its interval (else the bound is vacuous on this data)."""
    lo = rne_f16(sig2(u + beta) * (1 - SIG_REL)).double()
    hi = rne_f16(sig2(u - beta) * (1 + SIG_REL)).double()
    g = d64(got)
    nbad = int(((g < lo) | (g > hi)).sum())
    if nbad:
        rec.fail(key, "%d fp16 elements outside [RNE(sig(u + beta)(1 - 2^-21)), RNE(sig(u - beta)(1 + 2^-21))]" % nbad)
    for what, w in wrong:
        r = rne_f16(sig2(w)).double()
        if not bool(((r < lo) | (r > hi)).any()):
            rec.fail(key, "vacuous bound (%s)" % what)
    # the figure (a record, not a second threshold): the distance of sig(u) from the stored value's rounding cell over the linearised
    # allowance |sig'(u)| beta + SIG_REL sig(u), sig' = -ln 2 sig (1 - sig)
    s = sig2(u)
    c_lo, c_hi = _cell16(got)
    need = torch.maximum(torch.maximum(c_lo - s, s - c_hi), torch.zeros_like(s))
    allow = math.log(2.0) * s * (1 - s) * beta + SIG_REL * s
    used = need > 0
    k2 = key + ": distance to the stored cell / allowance"
    rec.ratio[k2] = max(rec.ratio.get(k2, 0.0), float((need[used] / allow[used]).max()) if bool(used.any()) else 0.0)
    near = int((got != rne_f16(sig2(u))).sum())
    rec.notes.append("%s: %d of %d elements differ from RNE16(sig(u))%s" % (key, near, got.numel(), "" if not nbad else "; %d outside" % nbad))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 convolutions, one matmul per tap (NHWC)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def conv_s2k4_fwd64(x, w, bias, tap=(1, 2), c0=72):
    """x [B][Hin][Hin][Ci], w [Co][Ci][4][4], bias [Co] in float64 -> the valid 4 x 4 / stride-2 convolution + bias [B][Ho][Ho][Co], the sum
    of its absolute terms (|bias| included) and the contribution of the input channels c0 .. c0 + 7 at tap (ky, kx) = `tap`."""
    B, Hin = x.shape[0], x.shape[1]
    Ho, co = (Hin - 4) // 2 + 1, w.shape[0]
    out = bias.view(1, 1, 1, co).expand(B, Ho, Ho, co).clone()
    ab = bias.abs().view(1, 1, 1, co).expand_as(out).clone()
    part = None
    for ky in range(4):
        for kx in range(4):
            xs = x[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Ho - 1) + 1:2, :]
            wt = w[:, :, ky, kx]
            out += xs @ wt.T
            ab += xs.abs() @ wt.abs().T
            if (ky, kx) == tuple(tap):
                part = xs[..., c0:c0 + 8] @ wt[:, c0:c0 + 8].T
    return out, ab, part


def conv_s2k4_dgrad64(dout, w, tap=(1, 2), c0=72):
    """dout [B][Ho][Ho][Co], w [Co][Ci][4][4] in float64 -> the data gradient of that convolution on its [B][2 Ho + 2][2 Ho + 2][Ci] input:
    input pixel (2 y + ky, 2 x + kx) receives sum_co dout[y][x][co] w[co][ci][ky][kx] -- per output-parity class (ky % 2, kx % 2) the four
    taps of that parity -- with the sum of the absolute terms and the contribution of output channels c0 .. c0 + 7 at tap `tap`."""
    B, Ho = dout.shape[0], dout.shape[1]
    Hi, ci = 2 * Ho + 2, w.shape[1]
    ref = torch.zeros(B, Hi, Hi, ci, dtype=torch.float64, device=dout.device)
    ab, part = torch.zeros_like(ref), torch.zeros_like(ref)
    da = dout.abs()
    for ky in range(4):
        for kx in range(4):
            sl = (slice(None), slice(ky, ky + 2 * (Ho - 1) + 1, 2), slice(kx, kx + 2 * (Ho - 1) + 1, 2))
            wt = w[:, :, ky, kx]
            ref[sl] += dout @ wt
            ab[sl] += da @ wt.abs()
            if (ky, kx) == tuple(tap):
                part[sl] += dout[..., c0:c0 + 8] @ wt[c0:c0 + 8]
    return ref, ab, part


def stem_conv64(x, w, bias, pre, Hin, stride):
    """x [B][I][I] (zero outside [pre, pre + I) of the Hin x Hin frame), w [Co][16] (tap = 4 ky + kx), bias [Co] in float64 -> the 4 x 4
    convolution + bias [B][Ho][Ho][Co] (unfold + one matmul) and the sum of its absolute terms (|bias| included)."""
    B, I = x.shape[0], x.shape[1]
    Ho = (Hin - 4) // stride + 1
    xp = torch.zeros(B, Hin, Hin, dtype=torch.float64, device=x.device)
    xp[:, pre:pre + I, pre:pre + I] = x
    span = stride * (Ho - 1) + 1
    pat = torch.stack([xp[:, ky:ky + span:stride, kx:kx + span:stride] for ky in range(4) for kx in range(4)], -1)      # [B][Ho][Ho][16]
    return pat @ w.T + bias, pat.abs() @ w.abs().T + bias.abs()


def sign_bits(t):
    """The sign-bit form of a ReLU gate, on the CPU (IEEE comparison, denormals kept): t [...][C] -> uint8 [...][C / 8], bit e of byte g =
    t[..., 8 g + e] > 0."""
    t = t.cpu()
    on = (t > 0).reshape(*t.shape[:-1], t.shape[-1] // 8, 8).to(torch.int32)
    return (on * (2 ** torch.arange(8, dtype=torch.int32))).sum(-1).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the tiling of the patch-resident 4 x 4 / stride-2 convolutions: a transcription of cp_plan (conv_s2.hip) and dg_tiling (conv_s2_dgrad.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
CP_BM, CP_PPX = 256, 392         # forward: output pixels per tile, patch capacity in sub-lattice pixels
DG_BM, DG_PPX = 128, 256         # data gradient: class pixels per tile, patch capacity in zero-bordered d-out pixels


def _patch_geometry(dgrad, B, H):
    """(BM, PPX, S, Ws) or None where the launcher's index range (2^31 elements) is exceeded."""
    if B <= 0 or H <= 0:
        return None
    if dgrad:
        side = 2 * (H + 1)
        return (DG_BM, DG_PPX, H + 1, H + 2) if B * side * side * 128 < 1 << 31 else None
    side = 2 * H + 2
    return (CP_BM, CP_PPX, H, H + 1) if B * H * H * 128 < 1 << 31 and B * side * side * 128 < 1 << 31 else None


def patch_windows(dgrad, B, H):
    """(largest window of the whole-batch tiling, or None where its period is not walked; largest window of the per-image tiling)."""
    BM, _, S, Ws = _patch_geometry(dgrad, B, H)

    def window(m0, ml):
        m0, ml = np.asarray(m0, dtype=np.int64), np.asarray(ml, dtype=np.int64)
        g0, g1 = m0 // S, ml // S
        return (g1 + g1 // S + 1) * Ws + (ml - g1 * S) + 1 - ((g0 + g0 // S) * Ws + (m0 - g0 * S)) + 1

    M, HH = B * S * S, S * S
    tiles = -(-M // BM)
    period = HH // math.gcd(BM, HH)
    whole = None
    if min(tiles, period) <= 65536:
        t = np.arange(min(tiles, period), dtype=np.int64)
        whole = int(window(t * BM, np.minimum((t + 1) * BM, M) - 1).max())
        if tiles > period:
            whole = max(whole, int(window((tiles - 1) * BM, M - 1)))          # the batch's partial last tile
    t = np.arange(-(-HH // BM), dtype=np.int64)
    return whole, int(window(t * BM, np.minimum((t + 1) * BM, HH) - 1).max())


def patch_tiling(dgrad, B, H):
    """(tiles, tpi) as the launchers choose them, or None where they refuse.  Forward (dgrad = 0): H = Hout, the tile grid is the
    Hout x Hout output pixels of an image and a sub-lattice row has Hout + 1 pixels.  Data gradient (dgrad = 1): H = Ho, the tile grid is the
    (Ho + 1) x (Ho + 1) pixels of one output-parity class of an image and a zero-bordered d-out row has Ho + 2 pixels.  A tile's patch is the
    LINEAR window from its first pixel's first tap to its last pixel's last tap: with g = m // S the (image, row) index of pixel m on the
    S-wide grid, pixel m sits at extended position (g + g // S) * Ws + m % S (every image owns one extended row more than S), and the window
    is last - first + Ws + 2 pixels.  Tiles of BM consecutive pixels of the whole batch if every distinct one fits the capacity (the pattern
    repeats with period S^2 / gcd(BM, S^2) tiles; the batch's partial last tile is checked besides; a period of more than 65536 tiles is not
    walked), else tiles that restart at every image (tpi = ceil(S^2 / BM) per image, the last one partial), else refused."""
    geo = _patch_geometry(dgrad, B, H)
    if geo is None:
        return None
    BM, PPX, S, _ = geo
    whole, per_image = patch_windows(dgrad, B, H)
    if whole is not None and whole <= PPX:
        return -(-B * S * S // BM), 0
    if per_image <= PPX:
        tpi = -(-S * S // BM)
        return B * tpi, tpi
    return None
