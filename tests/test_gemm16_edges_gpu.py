"""The bf16 matrix kernels through their C-ABI entry points, held to float64 at their tile edges and dispatch branches.

spair_gemm_nt16 (gemm_nt16_kernel, every variant), spair_gemm_tn16 (gemm_tn16_kernel, k_tn_ring, k_tn_reduce), spair_conv1x1_stack_fwd16 /
_bwd16 (k_pw_stack), spair_stem_wgrad16 and spair_cast_bf16, each at the smallest shapes that cross a tile edge (128 x 128 tiles: M = 1, 127,
128, 129), a K-tile switch (nt16: K tile 32 below K = 1024, 64 from there on), a store path (vector / scalar), a gate path (vector / scalar,
bf16 / fp32 mask) or a launch decision (XCD-remapped grid, ring / per-tile kernel + reduce / atomics).

The standard is tests/f64_hold.py's: inputs are seeded draws rounded to bf16 where the kernel reads bf16, the reference is the float64
product of those same stored values, an fp32 output must lie within U sum|terms| + 2^-24 |ref| (U = 2^-12, derived there: every shape here
keeps K <= 1032 and the rows of one split <= 2048, the splits <= 64 -- tn_split() below mirrors the launch code and asserts it), a bf16
output inside [RNE(ref - beta), RNE(ref + beta)], a gated-off element exactly 0.  Every bound is proved non-vacuous on reference data: it
must reject the reference without one 8-wide block of the summed dimension (tn: without one row split's rows) and, from 16 columns on, the
reference shifted by 8 columns.  Outputs are never zero-filled: they hold a sentinel (-7), with a guard row behind the last row and pad
columns that must come back untouched; pad columns of inputs that a kernel's contract says it does not read, or that cannot matter, hold 3.0.

Contracts the cases state: the 1x1 stack's backward reads dY and the top layer's weights in whole 8-column chunks, so of the columns
kd .. ldd - 1 one operand must be zero -- here dY holds 3.0 there and the weight copy zeros, as the step's prepared copies do; gemm_tn16's
fp32 B (plain rows) is rounded to bf16 on its way into LDS, and the reference does the same.

Observed figures (per case, the largest error / bound of the fp32 outputs and the bf16 elements that differ from RNE(ref)) are printed
by -s (Record.report); they are records, not thresholds -- the thresholds are the derived bounds.  None is tabulated here yet: this file
has not had a run on an MI355X.
"""
import ctypes

import pytest
import torch

from f64_hold import SENTINEL, U, Guarded, Record, _bias_sensitivity, _sensitivity, d64, hold, plant_special_gates, special_gate

pytestmark = pytest.mark.gpu

DEV = "cuda"
OK, ERR_UNSUPPORTED = 0, -4


def _call(name, *args):
    from spair_pytorch_amd import _lib as L
    return getattr(L.lib(), name)(*args)


def _stream():
    from spair_pytorch_amd import _lib as L
    return L.stream()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _i(*a):
    return (ctypes.c_int * len(a))(*a)


def _parr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else 0 for t in ts])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    return t.to(torch.bfloat16)


def _padded(vals, ld, fill=3.0):
    """vals [R][C] in rows of leading dimension ld, the pad columns holding finite garbage."""
    t = torch.full((vals.shape[0], ld), fill, dtype=vals.dtype)
    t[:, :vals.shape[1]] = vals
    return t.to(DEV)


def _done(rec):
    rec.report()
    assert not rec.bad, rec.bad


def _accumulated(rec, key, got, init, prod, absprod, drop):
    """An fp32 output that is accumulated into: got = init + prod within U (sum|terms| + |init|) + 2^-24 |ref|, the bound sensitive to `drop`
    (the contribution of the rows of one split) and, from 16 columns on, to a shift by 8 columns."""
    ref = init + prod
    bound = U * (absprod + abs(init)) + 2.0 ** -24 * ref.abs() + 1e-30
    rec.ratio_max(key, ((d64(got) - ref).abs() / bound).max())
    (_sensitivity if ref.dim() == 2 else _bias_sensitivity)(rec, key, ref, bound, drop)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_gemm_nt16, plain rows
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (M, N, K, lda, ldb, ldc, bf16 out, bias, relu, mask, ldmask): what it crosses
NT16_PLAIN = {
    "m1_n1_k8": (1, 1, 8, 8, 8, 4, 0, 1, 1, None, 0),                    # smallest everything; K below one K tile; scalar fp32 stores
    "m127_n100_k24": (127, 100, 24, 24, 24, 104, 1, 1, 0, "bf16", 100),  # partial row tile; partial 8-chunk at columns 96..99; scalar gate path
    "m129_n128_k128": (129, 128, 128, 128, 128, 128, 1, 0, 0, "bf16", 128),   # a second row tile of one row; no bias; vector gate path
    # two column tiles: the XCD-remapped grid, 2 row tiles padded to 8 = 6 surplus blocks per column tile; K tile 32 with a tail; fp32 mask
    "m129_n136_k40": (129, 136, 40, 40, 40, 136, 0, 1, 1, "f32", 136),
    "m1153_n264_k32": (1153, 264, 32, 32, 32, 264, 1, 1, 1, None, 0),    # 10 row tiles padded to 16, three column tiles; no mask
    "m300_n100_k1024": (300, 100, 1024, 1024, 1024, 100, 0, 1, 0, None, 0),   # K tile 64, fp32 output
    # K tile 64 with a tail of 8; lda > K with garbage behind K; odd ldc and ldmask: scalar stores and gates at odd 2-byte offsets
    "m129_n136_k1032": (129, 136, 1032, 1040, 1032, 137, 1, 1, 1, "bf16", 137),
}


def _mask(g, rows, cols, ld, kind):
    """A gate tensor [rows][ld] (bf16 or fp32 draws, 3.0 behind `cols`) holding the special values; returns it on DEV with its expected gate."""
    m = torch.full((rows, ld), 3.0, dtype=torch.bfloat16 if kind == "bf16" else torch.float32)
    m[:, :cols] = torch.randn(rows, cols, generator=g).to(m.dtype)
    planted = plant_special_gates(m[:, :cols])
    md = m.to(DEV)
    return md, special_gate(md[:, :cols], planted)


@pytest.mark.parametrize("name", list(NT16_PLAIN))
def test_gemm_nt16_plain_edges(name):
    M, N, K, lda, ldb, ldc, c16, has_bias, relu, mk, ldmask = NT16_PLAIN[name]
    g = _gen(100 + list(NT16_PLAIN).index(name))
    rec = Record("nt16 plain " + name)
    A = _padded(_bf(torch.randn(M, K, generator=g)), lda)
    W = _padded(_bf(torch.randn(N, K, generator=g) / K ** 0.5), ldb)
    bias = torch.randn(N, generator=g).to(DEV) if has_bias else None
    mask, gate = _mask(g, M, N, ldmask, mk) if mk else (None, None)
    out = Guarded(M, N, ldc, torch.bfloat16 if c16 else torch.float32, DEV)
    rc = _call("spair_gemm_nt16", _p(A), lda, _p(W), ldb, _p(out), ldc, M, N, K, _p(bias), _p(mask), ldmask, int(mk == "bf16"), relu, c16,
               None, None, _stream())
    assert rc == OK, rc
    a, w = d64(A[:, :K]), d64(W[:, :K])
    ref, ab = a @ w.T, a.abs() @ w.abs().T
    if has_bias:
        ref, ab = ref + d64(bias), ab + d64(bias).abs()
    k0 = K // 2 // 8 * 8           # one 8-wide block of K (the only one at K = 8)
    hold(rec, "C", out.block, ref, U * ab, relu=bool(relu), gate=gate, part=a[:, k0:k0 + 8] @ w[:, k0:k0 + 8].T)
    out.check(rec, "C")
    _done(rec)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_gemm_nt16, conv gather
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _conv_fwd64(x, w, bias, k, s, ho, wo):
    """x [B][H][W][Ci], w [Co][k][k][Ci] in float64: the valid convolution, the sum of its absolute terms and the part of the 8 input
    channels from Ci / 2 on."""
    co, ci = w.shape[0], w.shape[3]
    out = bias.view(1, 1, 1, co).expand(x.shape[0], ho, wo, co).clone()
    ab = bias.abs().view(1, 1, 1, co).expand_as(out).clone()
    pt = torch.zeros_like(out)
    h = ci // 2 // 8 * 8
    for ky in range(k):
        for kx in range(k):
            xs = x[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s, :]
            wt = w[:, ky, kx, :]
            out += xs @ wt.T
            ab += xs.abs() @ wt.abs().T
            pt += xs[..., h:h + 8] @ wt[:, h:h + 8].T
    return out, ab, pt


# (B, Hin, Win, Cin, Cout, k, s): rectangular inputs; Cin = 8 (a tap is one 16-byte chunk) at three kernel / stride pairs; Cin = 64, Cout = 136
# (two column tiles: the XCD-remapped grid with a gathered A) as a 1x1 layer -- batch 6 there, so that its weight gradient below has the
# four 64-row stages the ring kernel asks for
CONV_LAYERS = {
    "c8_k3s1": (2, 11, 14, 8, 24, 3, 1),
    "c8_k2s2": (2, 11, 14, 8, 24, 2, 2),
    "c8_k6s2": (2, 11, 14, 8, 24, 6, 2),
    "c64_k1s1": (6, 5, 7, 64, 136, 1, 1),
}


def _conv_layer(name):
    B, Hin, Win, Cin, Cout, k, s = CONV_LAYERS[name]
    g = _gen(200 + list(CONV_LAYERS).index(name))
    x = _bf(torch.randn(B, Hin, Win, Cin, generator=g)).to(DEV)
    w = _bf(torch.randn(Cout, k, k, Cin, generator=g) / (k * k * Cin) ** 0.5).to(DEV)
    bias = torch.randn(Cout, generator=g).to(DEV)
    return g, x, w, bias, (Hin - k) // s + 1, (Win - k) // s + 1


@pytest.mark.parametrize("cmap,c16", [(0, 1), (1, 0)])
@pytest.mark.parametrize("name", list(CONV_LAYERS))
def test_gemm_nt16_conv_forward_edges(name, cmap, c16):
    """Forward conv as an implicit GEMM (bias, relu).  Without cmap8: bf16 rows [M][Cout].  With cmap8: fp32 rows of leading dimension
    Cout + 8 written into the interior (offset 1, 2) of a [B][Hout + 2][Wout + 3] row grid whose border must stay untouched."""
    B, Hin, Win, Cin, Cout, k, s = CONV_LAYERS[name]
    g, x, w, bias, Ho, Wo = _conv_layer(name)
    rec = Record("nt16 conv fwd %s cmap %d" % (name, cmap))
    K, M = k * k * Cin, B * Ho * Wo
    Hc, Wc, oy, ox = (Ho + 2, Wo + 3, 1, 2) if cmap else (Ho, Wo, 0, 0)
    ldc = Cout + 8 if cmap else Cout
    out = Guarded(B * Hc * Wc, Cout, ldc, torch.bfloat16 if c16 else torch.float32, DEV)
    rc = _call("spair_gemm_nt16", _p(x), 0, _p(w), K, _p(out), ldc, M, Cout, K, _p(bias), None, 0, 0, 1, c16,
               _i(Hin, Win, Cin, Ho, Wo, k, k, s, s, 1, 1, 0, 0), _i(Ho, Wo, Hc, Wc, 1, 1, oy, ox) if cmap else None, _stream())
    assert rc == OK, rc
    ref, ab, pt = _conv_fwd64(d64(x), d64(w), d64(bias), k, s, Ho, Wo)
    grid = out.block.reshape(B, Hc, Wc, Cout)
    hold(rec, "C", grid[:, oy:oy + Ho, ox:ox + Wo], ref, U * ab, relu=True, part=pt)
    out.check(rec, "C")
    border = grid.clone()
    border[:, oy:oy + Ho, ox:ox + Wo] = SENTINEL
    if not bool((border == SENTINEL).all()):
        rec.fail("C", "rows outside the mapped interior were written")
    _done(rec)


def test_gemm_nt16_conv_dgrad_by_parity_class_edges():
    """The k4 s2 data gradient as four stride-1 2x2 gathers over d out, one per output-parity class, each row-mapped into dX (the recipe of
    test_conv16_fwd_dgrad_wgrad) on an input with odd sides 13 x 11: the classes have 7x6, 7x5, 6x6 and 6x5 rows, row 12 and column 10 are read
    by no window (their gradient is an exact 0 sum), the bf16 gate holds the special values.  dX starts as the sentinel: the classes' rows
    tile it (their counts add up to every row) and none may be left."""
    B, Hin, Win, Cin, Cout, k, s = 3, 13, 11, 16, 24, 4, 2
    g = _gen(300)
    rec = Record("nt16 conv dgrad k4s2 13x11")
    Ho, Wo = (Hin - k) // s + 1, (Win - k) // s + 1
    w = _bf(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5)
    go = _bf(torch.randn(B, Ho, Wo, Cout, generator=g)).to(DEV)
    mask, gate = _mask(g, B * Hin * Win, Cin, Cin, "bf16")
    dX = Guarded(B * Hin * Win, Cin, Cin, torch.bfloat16, DEV)
    rows = 0
    for py in range(2):
        for px in range(2):
            wc = w[:, :, py::2, px::2].permute(1, 2, 3, 0).reshape(Cin, 4 * Cout).contiguous().to(DEV)      # [ci][(ty, tx, co)] = w[co, ci, py + 2 ty, px + 2 tx]
            Hc, Wc = (Hin - py + 1) // 2, (Win - px + 1) // 2
            rows += B * Hc * Wc
            rc = _call("spair_gemm_nt16", _p(go), 0, _p(wc), 4 * Cout, _p(dX), Cin, B * Hc * Wc, Cin, 4 * Cout, None, _p(mask), Cin, 1, 0, 1,
                       _i(Ho, Wo, Cout, Hc, Wc, 2, 2, 1, 1, -1, -1, 0, 0), _i(Hc, Wc, Hin, Win, 2, 2, py, px), _stream())
            assert rc == OK, rc
    assert rows == B * Hin * Win          # written exactly once: the four classes' rows are disjoint by parity and add up to every row of dX
    wd, god = d64(w.to(DEV)), d64(go)
    ref = torch.zeros(B, Hin, Win, Cin, dtype=torch.float64, device=DEV)
    ab, pt = torch.zeros_like(ref), torch.zeros_like(ref)
    h = Cout // 2 // 8 * 8
    for ky in range(k):
        for kx in range(k):
            sl = (slice(None), slice(ky, ky + s * (Ho - 1) + 1, s), slice(kx, kx + s * (Wo - 1) + 1, s))
            wt = wd[:, :, ky, kx]
            ref[sl] += god @ wt
            ab[sl] += god.abs() @ wt.abs()
            pt[sl] += god[..., h:h + 8] @ wt[h:h + 8]
    gm = (gate[0].reshape(B, Hin, Win, Cin),) + gate[1:]
    hold(rec, "dX", dX.block.reshape(B, Hin, Win, Cin), ref, U * ab, gate=gm, part=pt)
    dX.check(rec, "dX")
    if dX.unwritten():
        rec.fail("dX", "%d elements were never written" % dX.unwritten())
    _done(rec)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_gemm_tn16
# ---------------------------------------------------------------------------------------------------------------------------------------------
_SCRATCH = {}
AMPLE = 4 << 20           # floats; the largest launch here asks for 66 x (128 x 256 + 128) = 2.2 M


def _scratch(n):
    """NaN-filled split-K scratch: a partial tile read before it was written shows."""
    if n not in _SCRATCH:
        _SCRATCH[n] = torch.full((n,), float("nan"), device=DEV)
    return _SCRATCH[n]


def _cd(a, b):
    return -(-a // b)


def tn_split(R, Mr, Nr, scratch_floats, b_bf16=True, conv_cin=None):
    """(kernel, row splits, rows per split) as spair_gemm_tn_ring (tn_ring.hip) and spair_gemm_tn16_impl (gemm16.hip) choose them for R
    summed rows and loaded extents Mr x Nr (M and N rounded up to 8; 4 for an fp32 B)."""
    if scratch_floats and b_bf16 and (conv_cin is None or conv_cin % 64 == 0):
        BN = 256 if Nr > 128 else 128
        tiles, stages = _cd(Mr, 128) * _cd(Nr, BN), _cd(R, 64)
        if stages >= 4:
            ns = max(1, min(stages // 2, 256 // tiles))
            ns = ns // 8 * 8 if ns >= 8 else ns
            sps = _cd(stages, ns)
            ns = _cd(stages, sps)
            if tiles * ns * (128 * BN + 128) <= scratch_floats:
                return "ring%d" % BN, ns, sps * 64
    tiles = _cd(Mr, 128) * _cd(Nr, 128)
    ns = max(1, min(_cd(R, 256), 768 // tiles))
    ns = ns // 8 * 8 if ns >= 8 else ns
    rps = _cd(_cd(R, ns), 32) * 32
    ns = _cd(R, rps)
    if scratch_floats and tiles * ns * (128 * 128 + 128) <= scratch_floats:
        return "tn16+reduce", ns, rps
    return "tn16 atomics", ns, rps


def _split_rows(R, ns, rps):
    """The rows the sensitivity check removes: those of the middle split (at most half of all rows, at least one; one split: the first half)."""
    r0 = (ns // 2) * rps
    return r0, min(R, r0 + min(rps, max(1, R // 2)))


# (R, M, N, lda, ldb, ldc, B bf16, scratch floats): the launch tn_split() must find, what it crosses
TN16_PLAIN = {
    "r1_m8_n8": ((1, 8, 8, 8, 8, 8, 1, 0), ("tn16 atomics", 1, 32)),                     # smallest; atomics
    # the step's F = 100 in rows of 104: Mstore, Nstore below the loaded extent, 3.0 in the pad columns of A and B, C's columns 100..103 and its guard row stay
    "r63_m100_n100": ((63, 100, 100, 104, 104, 104, 1, 0), ("tn16 atomics", 1, 64)),
    "r200_m100_n56": ((200, 100, 56, 104, 56, 56, 1, AMPLE), ("ring128", 2, 128)),        # ceil(R / 64) = 4 stages: the ring's minimum
    "r191_m136_n128": ((191, 136, 128, 136, 128, 128, 1, AMPLE), ("tn16+reduce", 1, 192)),  # 3 stages: refused by the ring -> gemm_tn16_kernel + k_tn_reduce
    "r257_m128_n264": ((257, 128, 264, 128, 264, 264, 1, AMPLE), ("ring256", 2, 192)),    # BN = 256 with an 8-column second tile; R one past a stage
    "r4100_m264_n136": ((4100, 264, 136, 264, 136, 136, 1, AMPLE), ("ring256", 22, 192)),  # three row tiles of A's columns; R no multiple of 64
    "r4100_m264_n136_small_scratch": ((4100, 264, 136, 264, 136, 136, 1, 1000), ("tn16 atomics", 15, 288)),   # scratch too small for either: atomics, SPAIR_OK
    "r300_m104_n100_f32b": ((300, 104, 100, 104, 100, 100, 0, 0), ("tn16 atomics", 2, 160)),   # fp32 B in plain rows, N a multiple of 4 only
}


def _run_tn16(rec, A, lda, Bm, ldb, b16, M, N, R, ldc, conv, cw, scratch_floats, a64, b64, bitwise, split):
    """Launches spair_gemm_tn16 (twice where `bitwise`) into sentinel-guarded, non-zero C (0.25) and column sums (0.125) and checks both
    against a64^T b64 (a64 [R][M], b64 [R][N] float64, N in C's column order)."""
    kernel, ns, rps = split
    assert rps <= 2048 and ns <= 64            # what U is derived for
    outs = []
    for _ in range(2 if bitwise else 1):
        C = Guarded(M, N, ldc, torch.float32, DEV, inside=0.25)
        cs = Guarded(1, M, M + 3, torch.float32, DEV, inside=0.125)
        sc = _scratch(scratch_floats) if scratch_floats else None
        rc = _call("spair_gemm_tn16", _p(A), lda, _p(Bm), ldb, b16, _p(C), ldc, M, N, R, conv, cw[0], cw[1], _p(cs), _p(sc),
                   ctypes.c_longlong(scratch_floats), _stream())
        assert rc == OK, rc
        outs.append((C, cs))
    C, cs = outs[0]
    r0, r1 = _split_rows(R, ns, rps)
    _accumulated(rec, "C", C.block, 0.25, a64.T @ b64, a64.abs().T @ b64.abs(), a64[r0:r1].T @ b64[r0:r1])
    _accumulated(rec, "colsum", cs.block[0], 0.125, a64.sum(0), a64.abs().sum(0), a64[r0:r1].sum(0))
    C.check(rec, "C")
    cs.check(rec, "colsum")
    if bitwise and not (torch.equal(outs[0][0].full, outs[1][0].full) and torch.equal(outs[0][1].full, outs[1][1].full)):
        rec.fail("C", "two runs through the split-K scratch differ")
    rec.notes.append("%s, %d split(s) of %d rows; sensitivity drops rows %d..%d" % (kernel, ns, rps, r0, r1 - 1))


@pytest.mark.parametrize("name", list(TN16_PLAIN))
def test_gemm_tn16_plain_edges(name):
    (R, M, N, lda, ldb, ldc, b16, scratch_floats), want = TN16_PLAIN[name]
    g = _gen(400 + list(TN16_PLAIN).index(name))
    rec = Record("tn16 plain " + name)
    split = tn_split(R, _cd(M, 8) * 8, _cd(N, 8 if b16 else 4) * (8 if b16 else 4), scratch_floats, bool(b16))
    assert split == want, split
    A = _padded(_bf(torch.randn(R, M, generator=g)), lda)
    Bv = torch.randn(R, N, generator=g)
    Bm = _padded(_bf(Bv) if b16 else Bv, ldb)
    b64 = d64(Bm[:, :N]) if b16 else d64(_bf(Bm[:, :N]))          # an fp32 B is rounded to bf16 by the kernel on its way into LDS -- and here
    # bit for bit only through the scratch (the ring's contract, and k_tn_reduce's fixed order); atomics may add in any order
    _run_tn16(rec, A, lda, Bm, ldb, b16, M, N, R, ldc, None, (0, 0), scratch_floats, d64(A[:, :M]), b64, split[0] != "tn16 atomics", split)
    _done(rec)


# the weight gradients of CONV_LAYERS: A = d out [R][Cout], B = the conv gather of x, C = dW in OIHW order (cw_cin / cw_taps), fused bias
# gradient.  Cin = 8 without scratch (atomics) and with (the ring refuses Cin % 64 != 0: gemm_tn16_kernel + k_tn_reduce); Cin = 64 with
# scratch: the ring's conv variant
TN16_CONV = {
    "c8_k3s1": ("c8_k3s1", 0, ("tn16 atomics", 1, 224)),
    "c8_k3s1_scratch": ("c8_k3s1", AMPLE, ("tn16+reduce", 1, 224)),
    "c8_k2s2": ("c8_k2s2", 0, ("tn16 atomics", 1, 96)),
    "c8_k2s2_scratch": ("c8_k2s2", AMPLE, ("tn16+reduce", 1, 96)),
    "c8_k6s2": ("c8_k6s2", 0, ("tn16 atomics", 1, 32)),
    "c8_k6s2_scratch": ("c8_k6s2", AMPLE, ("tn16+reduce", 1, 32)),
    "c64_k1s1_scratch": ("c64_k1s1", AMPLE, ("ring128", 2, 128)),
}


@pytest.mark.parametrize("name", list(TN16_CONV))
def test_gemm_tn16_conv_wgrad_edges(name):
    layer, scratch_floats, want = TN16_CONV[name]
    B, Hin, Win, Cin, Cout, k, s = CONV_LAYERS[layer]
    g, x, _, _, Ho, Wo = _conv_layer(layer)
    rec = Record("tn16 conv wgrad " + name)
    R, K = B * Ho * Wo, k * k * Cin
    split = tn_split(R, Cout, K, scratch_floats, True, Cin)
    assert split == want, split
    go = _bf(torch.randn(R, Cout, generator=g)).to(DEV)
    # b64[r][ci * taps + tap] = x[b, s y + ky, s x + kx, ci]: the gathered rows, in C's (OIHW) column order
    xd = d64(x)
    cols = torch.stack([xd[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, :] for ky in range(k) for kx in range(k)], -1)
    b64 = cols.reshape(R, Cin * k * k)
    _run_tn16(rec, go, Cout, x, 0, 1, Cout, K, R, K, _i(Hin, Win, Cin, Ho, Wo, k, k, s, s, 1, 1, 0, 0), (Cin, k * k), scratch_floats,
              d64(go), b64, split[0] != "tn16 atomics", split)
    _done(rec)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_conv1x1_stack_fwd16 / _bwd16
# ---------------------------------------------------------------------------------------------------------------------------------------------
PW_FWD = [(1, 1, 4, 4), (127, 2, 100, 104), (128, 3, 128, 128), (129, 4, 100, 104), (1000, 4, 8, 12)]       # (M, L, last cout, ldlast)


@pytest.mark.parametrize("ldw", [128, 136])
@pytest.mark.parametrize("M,L,nlast,ldlast", PW_FWD)
def test_conv1x1_stack_fwd16_edges(M, L, nlast, ldlast, ldw):
    """Each layer against float64 on the kernel's own stored input of that layer (X, then Y[l - 1]): a rounding flipped upstream does not
    leak into the next layer's bound.  Bias on every layer; weights in rows of ldw with 3.0 behind column 128 (never read)."""
    g = _gen(500 + M + L)
    rec = Record("1x1 stack fwd M %d L %d last %d ldw %d" % (M, L, nlast, ldw))
    couts = [128] * (L - 1) + [nlast]
    X = _bf(torch.relu(torch.randn(M, 128, generator=g))).to(DEV)
    Ws = [_padded(_bf(torch.randn(co, 128, generator=g) / 128 ** 0.5), ldw) for co in couts]
    bs = [(torch.randn(co, generator=g) * 0.1).to(DEV) for co in couts]
    Y = [Guarded(M, 128, 128, torch.bfloat16, DEV) for _ in range(L - 1)]
    last = Guarded(M, nlast, ldlast, torch.float32, DEV)
    rc = _call("spair_conv1x1_stack_fwd16", _p(X), _parr(Ws), _i(*[ldw] * L), _i(*couts), _parr(bs), _parr(Y + [None]), _p(last), ldlast, M, L,
               _stream())
    assert rc == OK, rc
    for l in range(L):
        xin = d64(X if l == 0 else Y[l - 1].block)
        w, b = d64(Ws[l][:, :128]), d64(bs[l])
        ref, ab = xin @ w.T + b, xin.abs() @ w.abs().T + b.abs()
        out = last if l == L - 1 else Y[l]
        hold(rec, "Y%d" % l, out.block, ref, U * ab, relu=l < L - 1, part=xin[:, 64:72] @ w[:, 64:72].T)
        out.check(rec, "Y%d" % l)
    _done(rec)


PW_BWD = [(1, 1, 4, 8, 4), (127, 2, 100, 104, 100), (129, 4, 100, 104, 100), (128, 3, 128, 128, 128), (1000, 4, 8, 8, 8)]   # (M, L, kd, ldd, top cout)


@pytest.mark.parametrize("M,L,kd,ldd,ctop", PW_BWD)
def test_conv1x1_stack_bwd16_edges(M, L, kd, ldd, ctop):
    """Layers in backward order; dX[l] = (dX[l - 1] Wd[l]^T) gated by gate[l] > 0, each against float64 on the stored dX[l - 1] (dY for the
    top layer) -- so a gated-off element, exactly 0 in dX[l], must also be the 0 the next layer summed.  dY holds 3.0 in its columns
    kd .. ldd - 1; the top layer's transposed weights are [128][cout rounded up to 8] with zeros behind cout (see the module docstring),
    the inner ones [128][128 or 136] with 3.0 behind column 128 (never read)."""
    g = _gen(600 + M + L)
    rec = Record("1x1 stack bwd M %d L %d kd %d ldd %d" % (M, L, kd, ldd))
    assert ctop == kd
    couts = [ctop] + [128] * (L - 1)
    ldws = [_cd(ctop, 8) * 8] + [128 + 8 * (l % 2) for l in range(1, L)]
    dY = _padded(_bf(torch.randn(M, kd, generator=g)), ldd)
    Wd = [_padded(_bf(torch.randn(128, couts[l], generator=g) / 128 ** 0.5), ldws[l], fill=0.0 if l == 0 else 3.0) for l in range(L)]
    gates, expect = [], []
    for l in range(L):
        m = _bf(torch.relu(torch.randn(M, 128, generator=g)))
        planted = plant_special_gates(m)
        md = m.to(DEV)
        gates.append(md)
        expect.append(special_gate(md, planted))
    dX = [Guarded(M, 128, 128, torch.bfloat16, DEV) for _ in range(L)]
    rc = _call("spair_conv1x1_stack_bwd16", _p(dY), ldd, kd, _parr(Wd), _i(*ldws), _i(*couts), _parr(gates), _parr(dX), M, L, _stream())
    assert rc == OK, rc
    for l in range(L):
        gin = d64(dY[:, :kd] if l == 0 else dX[l - 1].block)
        w = d64(Wd[l][:, :couts[l]])                # [128 cin][cout]
        n = gin.shape[1]
        c0 = n // 2 // 8 * 8 if n >= 16 else 0      # one 8-wide block of the summed columns (kd = 4, 8: all of them)
        hold(rec, "dX%d" % l, dX[l].block, gin @ w.T, U * (gin.abs() @ w.abs().T), gate=expect[l], part=gin[:, c0:c0 + 8] @ w[:, c0:c0 + 8].T)
        dX[l].check(rec, "dX%d" % l)
    _done(rec)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_stem_wgrad16
# ---------------------------------------------------------------------------------------------------------------------------------------------
STEM_SCRATCH = 512 * 128 * 32


def _stem_case(B, Hin):
    g = _gen(700 + Hin)
    s, k = 2, 4
    Ho = (Hin - k) // s + 1
    M = B * Ho * Ho
    x = torch.rand(B, Hin, Hin, generator=g).to(DEV)
    dY = _bf(torch.randn(M, 128, generator=g)).to(DEV)
    return x, dY, Ho, M


def _stem_launch(x, dY, B, Hin, Ho, scratch_floats):
    dW = Guarded(128, 16, 16, torch.float32, DEV, inside=0.5)          # accumulated into
    db = Guarded(1, 128, 131, torch.float32, DEV, inside=0.25)
    sc = _scratch(STEM_SCRATCH)
    rc = _call("spair_stem_wgrad16", _p(dY), _p(x), _p(dW), _p(db), _p(sc), ctypes.c_longlong(scratch_floats), B, Hin, 2, Ho, _stream())
    return rc, dW, db


# M = 16 rows, less than one 32-row chunk; an odd Hin whose last row and column no window reads; several workgroups with a partial last chunk
@pytest.mark.parametrize("B,Hin", [(1, 10), (2, 55), (3, 130)])
def test_stem_wgrad16_edges(B, Hin):
    """dW[co][tap] += sum_m dY[m][co] patch(m)[tap], db[co] += sum_m dY[m][co]; the kernel rounds the padded fp32 image to bf16 -- and so does
    the reference.  One workgroup sums chunks of 32 rows: ceil(M / 32) chunks over at most 512 workgroups (here 1, 43 and 384 workgroups of
    one chunk), k_stem_wgrad_reduce adds them in 8 chains: inside what U is derived for."""
    x, dY, Ho, M = _stem_case(B, Hin)
    rec = Record("stem wgrad B %d Hin %d" % (B, Hin))
    runs = []
    for _ in range(2):
        rc, dW, db = _stem_launch(x, dY, B, Hin, Ho, STEM_SCRATCH)
        assert rc == OK, rc
        runs.append((dW, db))
    dW, db = runs[0]
    xq = d64(_bf(x))
    a = d64(dY)
    pat = torch.stack([xq[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Ho - 1) + 1:2] for ky in range(4) for kx in range(4)], -1).reshape(M, 16)
    chunks = _cd(M, 32)
    rows = _cd(chunks, min(512, chunks)) * 32
    r0, r1 = _split_rows(M, _cd(M, rows), rows)
    _accumulated(rec, "dW", dW.block, 0.5, a.T @ pat, a.abs().T @ pat.abs(), a[r0:r1].T @ pat[r0:r1])
    _accumulated(rec, "db", db.block[0], 0.25, a.sum(0), a.abs().sum(0), a[r0:r1].sum(0))
    dW.check(rec, "dW")
    db.check(rec, "db")
    if not (torch.equal(runs[0][0].full, runs[1][0].full) and torch.equal(runs[0][1].full, runs[1][1].full)):
        rec.fail("dW", "two runs differ")
    _done(rec)


def test_stem_wgrad16_refuses_a_short_scratch():
    x, dY, Ho, _ = _stem_case(1, 10)
    rc, dW, db = _stem_launch(x, dY, 1, 10, Ho, STEM_SCRATCH - 1)
    assert rc == ERR_UNSUPPORTED, rc
    torch.cuda.synchronize()
    assert dW.outside_untouched() and db.outside_untouched()
    assert bool((dW.block == 0.5).all()) and bool((db.block == 0.25).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_cast_bf16
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _cast_specials():
    """+-0, +-inf, fp32 denormals, the largest finite fp32 (rounds to inf), and for two bf16 neighbours (one with an even, one with an odd
    last bit) the value exactly on the rounding tie and one fp32 ulp either side of it."""
    bits = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x7f7fffff, 0xff7fffff]
    for base in (0x3f800000, 0x3f810000, 0xc2f60000):
        bits += [base + 0x7fff, base + 0x8000, base + 0x8001]
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(1, 1, 1, 1), (37, 100, 104, 112), (300, 128, 128, 128)])
def test_cast_bf16_is_rne_bit_for_bit(rows, cols, ld_src, ld_dst):
    g = _gen(800 + rows)
    v = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-20, 20, (rows, cols), generator=g).float())
    sp = _cast_specials()
    flat = v.reshape(-1)
    n = min(flat.numel(), sp.numel())
    flat[flat.numel() - n:] = sp[sp.numel() - n:] if flat.numel() < sp.numel() else sp      # the last element of the last row is a tie case
    if flat.numel() >= 2 * sp.numel():
        flat[:sp.numel()] = sp
    src = _padded(v, ld_src)
    dst = Guarded(rows, cols, ld_dst, torch.bfloat16, DEV)
    rc = _call("spair_cast_bf16", _p(src), ld_src, _p(dst), ld_dst, ctypes.c_longlong(rows), cols, _stream())
    assert rc == OK, rc
    want = v.to(torch.bfloat16)                 # torch on the CPU: round to nearest even, denormals kept
    got = dst.block.cpu()
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), \
        "%d elements differ from RNE" % int((got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)).sum())
    assert dst.outside_untouched()
