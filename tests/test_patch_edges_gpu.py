"""The patch-resident 4 x 4 / stride-2 convolutions (conv_s2.hip, conv_s2_dgrad.hip) and the stem forward (misc.hip) through their C-ABI entry
points, held to float64 at the edges of their tilings.

spair_conv_s2k4_fwd16 / _fwd16_mask (k_conv_s2k4_patch), spair_conv_s2k4_dgrad16 / _dgrad16_bits (k_conv_s2k4_dgrad, persistent) and
spair_stem_conv_fwd / _fwd_mask (k_conv0_fwd_c1k4_mfma, k_conv0_fwd_c1k4), each at the smallest shapes that reach a decision of its launcher:
whole-batch or per-image tiles, a patch window exactly at the LDS capacity, a tile over dozens of images, a one-row tile, a workgroup that
walks two and three tiles, the last accepted image side; the stem's partial row block and partial 16-pixel column blocks, its last padded
side that fits the LDS limit, and the FMA kernel's strides and channel counts.  The tilings are asserted through spair_conv_s2k4_tiling
and f64_hold.patch_tiling (tests/test_patch_tiling_cpu.py holds the two to each other).

The standard is tests/f64_hold.py's: seeded operands, rounded to bf16 where the kernel reads bf16; the reference is the float64 convolution
of those stored values (one matmul per tap, on the GPU); a bf16 output must lie in [RNE(f(ref - beta)), RNE(f(ref + beta))], a gated-off
element must be exactly 0, and every bound must reject a subtly wrong reference (one block of 8 summed channels at one tap missing; the
channels shifted by 8) on the case's own data.  Outputs start as a sentinel (-7) with a guard row behind the last; masks as 0xAA.  Bounds:
  conv forward    beta = U (sum |x w| + |bias|): 2048 products + the bias in one fp32 accumulator, inside U = 2^-12's derivation (<= 2048 + 64 terms);
  data gradient   beta = U sum |dout w|: 4 taps x 128 channels = 512 terms;
  stem, bf16 out on the matrix cores: see test_stem_conv_fwd_edges;   stem FMA kernel: 16 FMAs from the bias, 2^-19 (sum |w x| + |bias|).

Observed on an MI355X with 256 CUs (-s prints them through Record.report; records, not thresholds -- the thresholds are the derived bounds).
The largest part of its beta that any element needed to reach the stored value, and the elements that differ from RNE(ref):
  conv forward       <= 2.0e-4 of beta (Hout 132, B 1); 0 (Hout 1, B 98) .. 321 of 4,460,544 (Hout 132, B 2) elements differ; every mask bit-equal;
                     the exact +-0 pre-activations (4 per pixel) are all stored as +0.0
  data gradient      <= 1.5e-4 of beta; 709 of 15,745,024 elements differ at Ho 123, B 2, 1,395 of 33,619,968 in the three-tile walk (B 1026,
                     workgroup 0 on tiles 0, 256, 512); the bits launch equal bit for bit
  stem, matrix cores 0 (Hin 4), 0.17 .. 0.43 (Hin 12 .. 36), 0.63 of beta at Hin 614, where 19,247 of 11,985,408 elements differ from RNE(ref): the
                     dropped lo x lo terms are what the bound is made of
  stem, FMA kernel   fp32 out 0.04 .. 0.10 of 2^-19 (sum |w x| + |bias|); bf16 out <= 0.005 of it, at most 1 element differs
"""
import ctypes
import functools

import pytest
import torch

from f64_hold import (U, Guarded, Record, conv_s2k4_dgrad64, conv_s2k4_fwd64, d64, hold, patch_tiling, plant_special_gates, rne16,
                      sign_bits, special_gate, stem_conv64)

pytestmark = pytest.mark.gpu

DEV = "cuda"
OK, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -4
C = 128


def _call(name, *args):
    from spair_pytorch_amd import _lib as L
    return getattr(L.lib(), name)(*args)


def _stream():
    from spair_pytorch_amd import _lib as L
    return L.stream()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    return t.to(torch.bfloat16)


def _done(rec):
    rec.report()
    assert not rec.bad, rec.bad


def _tiling(dgrad, B, H):
    t, p = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _call("spair_conv_s2k4_tiling", dgrad, B, H, ctypes.byref(t), ctypes.byref(p))
    return (t.value, p.value) if rc == OK else None


def _mask_buffer(rows):
    """[rows + 1][16] bytes of 0xAA: the mask of `rows` pixels and a guard row."""
    return torch.full((rows + 1, 16), 0xAA, dtype=torch.uint8, device=DEV)


def _check_mask(rec, key, mask, stored, rows, lo=None, hi=None):
    """The mask must be the sign-bit form of the kernel's own stored bf16 output (bit e of byte g = channel 8 g + e > 0, IEEE on the CPU), its
    guard row untouched; and, where the interval [lo, hi] of that output is given, consistent with it: an on bit needs hi > 0, an off bit
    lo <= 0."""
    if not bool((mask[rows] == 0xAA).all()):
        rec.fail(key, "the mask's guard row was written")
    want = sign_bits(stored.reshape(rows, -1))
    got = mask[:rows].cpu()
    if not torch.equal(got, want):
        rec.fail(key, "%d mask bytes differ from (stored output > 0)" % int((got != want).sum()))
    if lo is not None:
        on = ((mask[:rows, :, None].to(torch.int32) >> torch.arange(8, device=DEV, dtype=torch.int32)) & 1).bool().reshape(rows, -1)
        lo, hi = lo.reshape(rows, -1), hi.reshape(rows, -1)
        n = int((on & (hi <= 0)).sum()) + int((~on & (lo > 0)).sum())
        if n:
            rec.fail(key, "%d mask bits contradict the interval of their element" % n)
        rec.notes.append("%s: %d of %d bits on" % (key, int(on.sum()), on.numel()))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_conv_s2k4_fwd16 / _fwd16_mask
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _tap_parity(w):
    """w [co][ci][4][4] -> [co][2048] in tap-parity K order: column ((class * 2 + half) * 4 + tap) * 64 + c = w[co][half * 64 + c][py + 2 dy][px + 2 dx],
    class = 2 py + px, tap = 2 dy + dx."""
    wf = torch.empty(C, 2048, dtype=w.dtype)
    for py in range(2):
        for px in range(2):
            for half in range(2):
                for dy in range(2):
                    for dx in range(2):
                        blk = ((py * 2 + px) * 2 + half) * 4 + dy * 2 + dx
                        wf[:, blk * 64:(blk + 1) * 64] = w[:, half * 64:(half + 1) * 64, py + 2 * dy, px + 2 * dx]
    return wf


ZERO_W = slice(8, 12)        # output channels whose weights are all +-0.0: their pre-activation is an exact +-0
NEG_W = slice(12, 16)        # output channels whose weights are all negative: on a non-negative input their pre-activation is <= 0


@functools.lru_cache(maxsize=None)
def _fwd_weights():
    """One set of weights for every forward case.  Channels 8 .. 15 have non-positive weights and bias -0.0: 8 .. 11 all zeros of both
    signs, 12 .. 15 all negative; the bias also holds +0.0 and -0.0 elsewhere."""
    g = _gen(1000)
    w = torch.randn(C, C, 4, 4, generator=g) / 45.0
    w[NEG_W] = -w[NEG_W].abs()
    w[ZERO_W] = torch.where(torch.rand(4, C, 4, 4, generator=g) > 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    w = _bf(w)
    bias = torch.randn(C, generator=g) * 0.1
    bias[8:16] = -0.0
    bias[0], bias[1], bias[40], bias[127] = 0.0, -0.0, 0.0, -0.0
    assert int(torch.signbit(bias).logical_and(bias == 0).sum()) == 10 and bool(torch.signbit(w[ZERO_W]).any()) and bool((w[NEG_W] < 0).all())
    return w.to(DEV), _tap_parity(w).to(DEV), bias.to(DEV)


# (Hout, B): the tiling it must get (tiles, tiles per image; 0 = tiles over the whole batch) -- what it crosses
FWD_CASES = {
    (1, 98): (1, 0),           # one tile over 98 images, its patch window exactly the capacity of 392 pixels
    (1, 99): (99, 1),          # one image more: per-image tiles of one row each
    (3, 24): (1, 0),           # 24 images in one tile, window 384
    (3, 25): (25, 1),          # window 400: per-image tiles of 9 rows
    (7, 40): (8, 0),           # tiles spanning 5 - 6 images; the batch's last tile is partial (168 rows)
    (66, 2): (36, 18),         # per-image tiles, 18 per image, the last of 4 rows
    (132, 1): (69, 0),         # the largest accepted side, window exactly 392; the last tile has 16 rows
    (132, 2): (138, 69),       # the same per image
}


@pytest.mark.parametrize("Hout,B", list(FWD_CASES))
def test_conv_s2k4_fwd16_edges(Hout, B):
    """relu(conv + bias) of a non-negative bf16 NHWC input (a stored post-ReLU activation, half of it exact zeros) against float64,
    beta = U (sum |x w| + |bias|).  The launch with the mask must store the same bits and leave the mask of exactly its own stored
    output; channels 8 .. 15 must come out as zeros with their bits off (their pre-activation is an exact +-0 or negative)."""
    rec = Record("conv_s2k4 fwd Hout %d B %d" % (Hout, B))
    assert _tiling(0, B, Hout) == patch_tiling(0, B, Hout) == FWD_CASES[(Hout, B)]
    w, wf, bias = _fwd_weights()
    Hin, M = 2 * Hout + 2, B * Hout * Hout
    x = _bf(torch.relu(torch.randn(B, Hin, Hin, C, generator=_gen(1100 + 7 * Hout + B)))).to(DEV)
    out, outm, mask = Guarded(M, C, C, torch.bfloat16, DEV), Guarded(M, C, C, torch.bfloat16, DEV), _mask_buffer(M)
    rc = _call("spair_conv_s2k4_fwd16", _p(x), _p(wf), _p(bias), _p(out), B, Hin, Hout, _stream())
    assert rc == OK, rc
    rc = _call("spair_conv_s2k4_fwd16_mask", _p(x), _p(wf), _p(bias), _p(outm), _p(mask), B, Hin, Hout, _stream())
    assert rc == OK, rc
    ref, ab, part = conv_s2k4_fwd64(d64(x), d64(w), d64(bias))
    beta = U * ab
    got = out.block.view(B, Hout, Hout, C)
    hold(rec, "Y", got, ref, beta, relu=True, part=part)
    for o, key in ((out, "Y"), (outm, "Y (mask launch)")):
        o.check(rec, key)
        if o.unwritten():
            rec.fail(key, "%d elements were never written" % o.unwritten())
    if not torch.equal(out.full.view(torch.int16), outm.full.view(torch.int16)):
        rec.fail("Y (mask launch)", "the output differs from the launch without a mask")
    _check_mask(rec, "mask", mask, outm.block, M, rne16((ref - beta).clamp_min(0)).double(), rne16((ref + beta).clamp_min(0)).double())
    if bool((got[..., 8:16] != 0).any()):
        rec.fail("Y", "a channel with non-positive weights and bias -0.0 is not 0")
    n0 = int((ref[..., ZERO_W] == 0).sum())
    assert n0 == M * 4 and bool((ref[..., NEG_W] <= 0).all())
    rec.notes.append("%d exact +-0 pre-activations, %d stored as -0.0" % (n0, int(torch.signbit(got[..., ZERO_W].float()).sum())))
    _done(rec)


@pytest.mark.parametrize("B", [1, 2])
def test_conv_s2k4_fwd16_refuses_hout_133(B):
    """One past the largest side: a 256-row tile's window would be 393 pixels.  Refused in front of the launch, nothing written."""
    assert _tiling(0, B, 133) is None and patch_tiling(0, B, 133) is None
    out, mask = Guarded(4, C, C, torch.bfloat16, DEV), _mask_buffer(4)
    assert _call("spair_conv_s2k4_fwd16", None, None, None, _p(out), B, 268, 133, _stream()) == ERR_UNSUPPORTED
    assert _call("spair_conv_s2k4_fwd16_mask", None, None, None, _p(out), _p(mask), B, 268, 133, _stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert out.unwritten() == 4 * C and out.outside_untouched() and bool((mask == 0xAA).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_conv_s2k4_dgrad16 / _dgrad16_bits
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dgrad_weights():
    g = _gen(2000)
    w = _bf(torch.randn(C, C, 4, 4, generator=g) / 23.0)          # [co][ci][ky][kx]
    wd = []
    for py in range(2):
        for px in range(2):                                        # [ci][(ty * 2 + tx) * 128 + co] = w[co][ci][py + 2 ty][px + 2 tx]
            wd.append(torch.cat([w[:, :, py + 2 * ty, px + 2 * tx].t() for ty in range(2) for tx in range(2)], 1).contiguous().to(DEV))
    return w.to(DEV), wd


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# name: (Ho, B or a function of the CU count, tiling or a function of the CU count, extra tiles a workgroup walks)
DGRAD_CASES = {
    "ho1_b28": (1, 28, (1, 0)),                 # one tile over 28 images, window 252
    "ho1_b29": (1, 29, (29, 1)),                # window 261 > 256: per-image tiles of 4 class pixels
    "ho7_b5": (7, 5, (3, 0)),                   # 64 class pixels per image: 2 images per tile, the last tile half full
    "ho123_b1": (123, 1, (121, 0)),             # the largest accepted side: window 255
    "ho123_b2": (123, 2, (242, 121)),           # the same per image (the whole-batch window would be 380)
    "ho7_walk2": (7, lambda cus: 2 * (cus + 4), lambda cus: (cus + 4, 0)),           # persistent: four workgroups walk a second tile
    "ho7_walk3": (7, lambda cus: 2 * (2 * cus + 1), lambda cus: (2 * cus + 1, 0)),   # every workgroup walks two tiles, the first one three
}


@pytest.mark.parametrize("name", list(DGRAD_CASES))
def test_conv_s2k4_dgrad16_edges(name):
    """d x = conv2d_backward_input(d out, W) where gate > 0, else exactly 0, against float64 (per input pixel the four taps of its parity
    class x 128 channels: 512 terms, beta = U sum |dout w|).  The gate holds +0.0, -0.0 and the smallest bf16 denormals of both signs in
    its first image, in its last one and -- in the persistent cases -- at the first pixels of every further tile workgroup 0 walks (tile
    index grid, 2 grid: the patch the loaders fetched under the previous tile's last class epilogue).  The same launch reading the gate
    as sign bits (built on the CPU from IEEE gate > 0) must store the same bits."""
    Ho, B, want = DGRAD_CASES[name]
    cus = _cus()
    if callable(B):
        B, want = B(cus), want(cus)
    Hi = 2 * Ho + 2
    nbytes = 2 * C * B * (Ho * Ho + 3 * Hi * Hi) + 16 * B * Hi * Hi
    if nbytes > 1 << 30:
        pytest.skip("the operands of %d tiles on %d CUs take %d MB (> 1 GB)" % (want[0], cus, nbytes >> 20))
    rec = Record("conv_s2k4 dgrad %s (Ho %d, B %d, %d CUs)" % (name, Ho, B, cus))
    assert _tiling(1, B, Ho) == patch_tiling(1, B, Ho) == want, (_tiling(1, B, Ho), patch_tiling(1, B, Ho), want)
    tiles, tpi = want
    grid = min(tiles, cus)
    w, wd = _dgrad_weights()
    g = _gen(2100 + list(DGRAD_CASES).index(name))
    dout = _bf(torch.randn(B, Ho, Ho, C, generator=g)).to(DEV)
    gate = _bf(torch.randn(B * Hi * Hi, C, generator=g))
    # rows of the gate that get the special values: the first image, the last image, and the first class pixel (classes (0, 0) and (0, 1):
    # two adjacent pixels) of every further tile workgroup 0 walks
    views = {(0, Hi * Hi), ((B - 1) * Hi * Hi, B * Hi * Hi)}
    if name.startswith("ho7_walk"):
        assert tpi == 0 and tiles > grid
        for t in range(grid, tiles, grid):
            img = t * 128 // 64          # 64 class pixels per image: tile t starts at class pixel (0, 0) of image 2 t
            assert 0 < img < B - 1
            views.add((img * Hi * Hi, img * Hi * Hi + 2))
        rec.notes.append("grid %d, workgroup 0 walks tiles %s" % (grid, list(range(0, tiles, grid))))
    planted = []
    for r0, r1 in sorted(views):
        planted += [(r0 + r, c, on) for r, c, on in plant_special_gates(gate[r0:r1])]
    gate_d = gate.to(DEV)
    gm = special_gate(gate_d, planted)
    gbits = sign_bits(gate).to(DEV)
    out, outb = Guarded(B * Hi * Hi, C, C, torch.bfloat16, DEV), Guarded(B * Hi * Hi, C, C, torch.bfloat16, DEV)
    rc = _call("spair_conv_s2k4_dgrad16", _p(dout), _p(wd[0]), _p(wd[1]), _p(wd[2]), _p(wd[3]), _p(gate_d), _p(out), B, Ho, _stream())
    assert rc == OK, rc
    rc = _call("spair_conv_s2k4_dgrad16_bits", _p(dout), _p(wd[0]), _p(wd[1]), _p(wd[2]), _p(wd[3]), _p(gbits), _p(outb), B, Ho, _stream())
    assert rc == OK, rc
    ref, ab, part = conv_s2k4_dgrad64(d64(dout), d64(w))
    shape = (B, Hi, Hi, C)
    hold(rec, "dX", out.block.view(shape), ref, U * ab, gate=(gm[0].view(shape),) + gm[1:], part=part)
    for o, key in ((out, "dX"), (outb, "dX (bits)")):
        o.check(rec, key)
        if o.unwritten():
            rec.fail(key, "%d elements were never written" % o.unwritten())
    if not torch.equal(out.full.view(torch.int16), outb.full.view(torch.int16)):
        rec.fail("dX (bits)", "%d elements differ from the launch reading the bf16 gate"
                 % int((out.full.view(torch.int16) != outb.full.view(torch.int16)).sum()))
    _done(rec)


@pytest.mark.parametrize("B", [1, 2])
def test_conv_s2k4_dgrad16_refuses_ho_124(B):
    """One past the largest side: a 128-pixel tile's window would be 257 pixels.  Refused in front of the launch, nothing written."""
    assert _tiling(1, B, 124) is None and patch_tiling(1, B, 124) is None
    out = Guarded(4, C, C, torch.bfloat16, DEV)
    gate = torch.zeros(16, device=DEV)
    assert _call("spair_conv_s2k4_dgrad16", None, None, None, None, None, _p(gate), _p(out), B, 124, _stream()) == ERR_UNSUPPORTED
    assert _call("spair_conv_s2k4_dgrad16_bits", None, None, None, None, None, _p(gate), _p(out), B, 124, _stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert out.unwritten() == 4 * C and out.outside_untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_stem_conv_fwd / _fwd_mask
# ---------------------------------------------------------------------------------------------------------------------------------------------
C0_ROWS = 5                                                     # output rows per workgroup (misc.hip)
HIN_MAX = 48 * 1024 // ((4 * (C0_ROWS - 1) + 4) * 4) // 2 * 2   # misc_conv0_reads_unpadded: (4 (C0_ROWS - 1) + 4) Hin floats <= 48 KB, even: 614

# (B, I, pre, post): even padded side Hin = I + pre + post -> the matrix-core kernel (stride 2, 128 channels, bf16 out)
STEM_MFMA = {
    "hout1": (2, 2, 1, 1),             # Hin 4: one pixel, one partial 16-pixel block
    "hout5_pre0": (3, 12, 0, 0),       # Hin 12: exactly one row block (C0_ROWS); no padding at all
    "hout6": (2, 9, 2, 3),             # Hin 14: a second row block of one row
    "hout15": (2, 25, 3, 4),           # Hin 32: 15 of a 16-pixel column block
    "hout16": (1, 28, 3, 3),           # Hin 34: exactly one column block
    "hout17_pre0": (2, 30, 0, 6),      # Hin 36: a second column block of one pixel; rows 15, 16 in a partial row block
    "hin_max": (1, HIN_MAX - 14, 7, 7),     # Hin 614: the last even side inside the 48-KB limit (Hout 306: 20 column blocks, the last of 2)
}
# (B, I, pre, post, stride, Cout): the FMA kernel (k_conv0_fwd_c1k4) -- an odd padded side at stride 2 / 128 channels, and the other strides
STEM_FMA = {
    "odd_hin_s2_c128": (2, 29, 1, 1, 2, 128),     # Hin 31, Hout 14
    "s1_c32": (2, 10, 1, 2, 1, 32),               # Hin 13, Hout 10
    "s3_c64": (2, 17, 2, 1, 3, 64),               # Hin 20, Hout 6
    "s4_c128": (1, 21, 0, 4, 4, 128),             # Hin 25, Hout 6
}


def _stem_operands(seed, B, I, Cout):
    g = _gen(seed)
    x = (torch.rand(B, I, I, generator=g) * (torch.rand(B, I, I, generator=g) > 0.5)).to(DEV)
    w = (torch.randn(Cout, 16, generator=g) * 0.3).to(DEV)
    bias = torch.randn(Cout, generator=g) * 0.1
    bias[3], bias[5] = 0.0, -0.0
    return x, w, bias.to(DEV)


def _stem_run(x, w, bias, B, I, pre, Hin, Hout, Cout, stride, out_bf16):
    out = Guarded(B * Hout * Hout, Cout, Cout, torch.bfloat16 if out_bf16 else torch.float32, DEV)
    rc = _call("spair_stem_conv_fwd", _p(x), _p(w), _p(bias), _p(out), B, I, pre, Hin, Hout, Cout, stride, out_bf16, _stream())
    return rc, out


def _stem_fma_checks(rec, x, w, bias, B, I, pre, Hin, Hout, Cout, stride, ref, ab, outs=(0, 1)):
    """The FMA kernel, fp32 and bf16 output: 16 FMAs on top of the bias in fp32, each rounding within 2^-24 of a partial sum that the
    absolute sum bounds: 16 x 2^-24 = 2^-20 < 2^-19 of (sum |w x| + |bias|).  The fp32 output carries no further rounding (f32_slack 0)."""
    w5 = torch.zeros_like(w)
    w5[:, 5] = w[:, 5]
    part = stem_conv64(d64(x), d64(w5), torch.zeros_like(d64(bias)), pre, Hin, stride)[0]          # tap (1, 1) alone
    beta = 2.0 ** -19 * ab
    for out_bf16 in outs:
        rc, out = _stem_run(x, w, bias, B, I, pre, Hin, Hout, Cout, stride, out_bf16)
        assert rc == OK, rc
        key = "Y fma %s" % ("bf16" if out_bf16 else "fp32")
        hold(rec, key, out.block.view(B, Hout, Hout, Cout), ref, beta, relu=True, part=part, f32_slack=0.0)
        out.check(rec, key)
        if out.unwritten():
            rec.fail(key, "%d elements were never written" % out.unwritten())


@pytest.mark.parametrize("name", list(STEM_MFMA))
def test_stem_conv_fwd_edges(name):
    """The stem on the matrix cores against the float64 convolution of the fp32 operands.  The kernel splits every operand v into bf16
    parts hi = bf16(v), lo = bf16(v - hi): |v - hi| <= 2^-9 |v|, so |v - hi - lo| <= 2^-18 |v|.  Of (wh + wl + ew)(xh + xl + ex) it sums
    wh xh + wl xh + wh xl and drops wl xl, ew x and w ex: at most 3 x 2^-18 |w x| each product, plus terms of 2^-27 and below.  The 48
    partial products and the bias accumulate in fp32: at most 49 x 2^-24 < 2^-18 of the absolute sum.  Together below
    beta = (2^-16 + 2^-19) (sum |w x| + |bias|) = 4.5 x 2^-18 (...).  The accepted set must reject the reference with w rounded to bf16 once
    -- a kernel that lost its lo parts, 2^-9 relative -- and the reference with its channels shifted by 8.  With the mask: same output
    bits, the mask bit-equal to (stored > 0), its 0xAA guard row untouched.  The fp32 output of the same shape takes the FMA kernel."""
    B, I, pre, post = STEM_MFMA[name]
    Hin = I + pre + post
    Hout = (Hin - 4) // 2 + 1
    assert Hin % 2 == 0 and Hin <= HIN_MAX
    rec = Record("stem fwd %s (B %d, Hin %d, Hout %d)" % (name, B, Hin, Hout))
    x, w, bias = _stem_operands(3000 + Hin, B, I, 128)
    ref, ab = stem_conv64(d64(x), d64(w), d64(bias), pre, Hin, 2)
    lost_lo = stem_conv64(d64(x), d64(_bf(w)), d64(bias), pre, Hin, 2)[0]
    beta = (2.0 ** -16 + 2.0 ** -19) * ab
    rc, out = _stem_run(x, w, bias, B, I, pre, Hin, Hout, 128, 2, 1)
    assert rc == OK, rc
    M = B * Hout * Hout
    outm, mask = Guarded(M, 128, 128, torch.bfloat16, DEV), _mask_buffer(M)
    rc = _call("spair_stem_conv_fwd_mask", _p(x), _p(w), _p(bias), _p(outm), _p(mask), B, I, pre, Hin, Hout, _stream())
    assert rc == OK, rc
    hold(rec, "Y mfma bf16", out.block.view(B, Hout, Hout, 128), ref, beta, relu=True, part=ref - lost_lo)
    for o, key in ((out, "Y mfma bf16"), (outm, "Y mfma bf16 (mask launch)")):
        o.check(rec, key)
        if o.unwritten():
            rec.fail(key, "%d elements were never written" % o.unwritten())
    if not torch.equal(out.full.view(torch.int16), outm.full.view(torch.int16)):
        rec.fail("Y mfma bf16 (mask launch)", "the output differs from the launch without a mask")
    _check_mask(rec, "mask", mask, outm.block, M, rne16((ref - beta).clamp_min(0)).double(), rne16((ref + beta).clamp_min(0)).double())
    if name != "hin_max":           # (the fp32 rows of that one are 48 MB: the FMA kernel's own cases below are enough)
        _stem_fma_checks(rec, x, w, bias, B, I, pre, Hin, Hout, 128, 2, ref, ab, outs=(0,))
    _done(rec)


def test_stem_conv_fwd_refuses_the_next_even_side():
    """HIN_MAX + 2 = 616: (4 (C0_ROWS - 1) + 4) x 616 floats are 49,280 B > 48 KB.  Refused in front of the launch by both entry points."""
    Hin = HIN_MAX + 2
    assert (4 * (C0_ROWS - 1) + 4) * HIN_MAX * 4 <= 48 * 1024 < (4 * (C0_ROWS - 1) + 4) * Hin * 4
    B, I, pre = 1, Hin - 14, 7
    Hout = (Hin - 4) // 2 + 1
    x, w, bias = _stem_operands(3999, B, I, 128)
    out, mask = Guarded(4, 128, 128, torch.bfloat16, DEV), _mask_buffer(4)
    for bf16_out in (0, 1):
        assert _call("spair_stem_conv_fwd", _p(x), _p(w), _p(bias), _p(out), B, I, pre, Hin, Hout, 128, 2, bf16_out, _stream()) == ERR_UNSUPPORTED
    assert _call("spair_stem_conv_fwd_mask", _p(x), _p(w), _p(bias), _p(out), _p(mask), B, I, pre, Hin, Hout, _stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert out.unwritten() == 4 * 128 and out.outside_untouched() and bool((mask == 0xAA).all())


@pytest.mark.parametrize("name", list(STEM_FMA))
def test_stem_conv_fwd_fma_edges(name):
    """The FMA kernel at an odd padded side (stride 2, 128 channels: the matrix-core kernel needs an even one, and the mask call is
    refused) and at strides 1, 3, 4 with 32, 64 and 128 channels, fp32 and bf16 output; bound in _stem_fma_checks."""
    B, I, pre, post, stride, Cout = STEM_FMA[name]
    Hin = I + pre + post
    Hout = (Hin - 4) // stride + 1
    rec = Record("stem fwd fma %s (B %d, Hin %d, Hout %d)" % (name, B, Hin, Hout))
    x, w, bias = _stem_operands(3500 + Hin, B, I, Cout)
    ref, ab = stem_conv64(d64(x), d64(w), d64(bias), pre, Hin, stride)
    _stem_fma_checks(rec, x, w, bias, B, I, pre, Hin, Hout, Cout, stride, ref, ab)
    if stride == 2 and Cout == 128:
        assert Hin % 2 == 1
        out, mask = Guarded(B * Hout * Hout, 128, 128, torch.bfloat16, DEV), _mask_buffer(B * Hout * Hout)
        rc = _call("spair_stem_conv_fwd_mask", _p(x), _p(w), _p(bias), _p(out), _p(mask), B, I, pre, Hin, Hout, _stream())
        assert rc == ERR_UNSUPPORTED, rc
        torch.cuda.synchronize()
        assert out.unwritten() == out.block.numel() and out.outside_untouched() and bool((mask == 0xAA).all())
    _done(rec)

