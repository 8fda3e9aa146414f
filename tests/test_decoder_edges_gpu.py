"""The fused object-decoder kernels (dec_fused.hip, dec_fused_bwd.hip) through their C-ABI entry points, held to float64 over the shapes
the entry points accept -- not only the benchmark's A = 50, n_out = 1568.

spair_decoder_fwd16 (k_dec_pack + k_dec_fwd): A from 1 to 64 (the k padding of z_attr to 64, chunks of 8 read only inside ld_za),
n_out = 64 .. 2048 with an even and an odd number of 32-column pairs (the two workgroups of a pair then take ceil and floor of them:
n_out = 96 -> 2 + 1, 160 -> 3 + 2), leading dimensions above the width, N = 1 and N one off a multiple of the 256-row block.
spair_decoder_bwd16 (k_dec_bwd): n_out % 64 = 0, 8 and 32 (the last 64-wide K stage full, 8 and 32 columns wide), a number of stages that
is 0, 1 and 2 above a multiple of the three-stage rotation (1152 -> 18, 64 and 1568 -> 1 and 25, 72 and 2048 -> 2 and 32), ld_s / ld2 /
ld_dza above the width, N one off a multiple of the 128-row block.

The standard is tests/f64_hold.py's.  Every layer is checked against float64 on the kernel's OWN stored input of that layer and the
bf16-rounded weights the kernel multiplies (for decoder.out: rounded AFTER the fp32 scaling by -scale log2(e), as k_dec_pack does):
  hidden layers   bf16, [RNE(relu(ref - beta)), RNE(relu(ref + beta))], beta = U (sum |terms| + |bias|) (<= 256 terms + the bias in fp32);
  sprites         fp16 = 1 / (1 + exp2(u)), u = the accumulator (its bias term folded as dec_fused.hip does, in fp32):
                  [RNE16(sig(u + beta)(1 - 2^-21)), RNE16(sig(u - beta)(1 + 2^-21))] -- the sigmoid decreases in u; 2^-21 = 8 fp32 ulps
                  covers v_exp_f32, the add and v_rcp_f32 at 1 ulp each with margin (no accuracy figures of the two transcendental
                  instructions were at hand: 1 ulp is the usual statement for them, and the margin is 2.7 x);
  dH2, dH1        bf16, RNE interval with beta = U sum |terms| (<= 2048 terms), exactly 0 where the stored activation is not > 0 -- the
                  gates hold +0.0, -0.0 and the smallest bf16 denormals of both signs;
  d z_attr        fp32, within U sum |terms| + 2^-24 |ref|.
Every bound must reject, on the case's own data, the reference without one block of 8 summed channels and the reference with its
columns shifted by 8 (from 16 columns on); the sprites besides the reference with the grey and alpha scales swapped.  Outputs start as a
sentinel (-7) with a guard row and, where the leading dimension is larger than the width, pad columns that must stay; pad columns of the
inputs hold 3.0; the packed-weight scratch starts as bf16 NaNs.

Observed on an MI355X (-s prints them through Record.report; records, not thresholds -- the thresholds are the derived bounds):
  H1, H2      at most 4 elements of a case differ from RNE(ref); the largest part of beta an element needed: 3.0e-5
  sprites     0 (N 1; N 33) .. 49 of 522,240 (N 255, n_out 2048) elements differ from RNE16(sig(u)); sig(u) lies at most 0.0061 of the
              linearised allowance (ln 2 sig (1 - sig) beta + 2^-21 sig) outside the stored value's rounding cell
  dH2, dH1    at most 6 / 1 elements differ from RNE(ref); 2.1e-5 / 0 of beta needed; every gate read 1 - 3 stored -0.0 and 2 - 6 bf16 denormals
  d z_attr    4.8e-5 (N 1) .. 3.7e-4 of U sum |terms| + 2^-24 |ref|
"""
import ctypes

import pytest
import torch

from f64_hold import U, Guarded, Record, check_sigmoid16, d64, hold, plant_special_gates, special_gate

pytestmark = pytest.mark.gpu

DEV = "cuda"
OK = 0
H1, H2 = 128, 256
L2E = 1.4426950408889634


def _lib():
    from spair_pytorch_amd import _lib as L
    return L


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


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


def _whole(rec, key, out):
    out.check(rec, key)
    if out.unwritten():
        rec.fail(key, "%d elements were never written" % out.unwritten())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_decoder_fwd16
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (N, A, n_out, ld_za, ld_s), (obj_scale, alpha_scale, alpha_bias): what it crosses
FWD_CASES = [
    ((257, 50, 1568, 56, 1568), (2.0, 0.1, 5.0)),      # the benchmark's widths; a second row block of one row; z_attr chunk 48 .. 55 partly pad
    ((1, 1, 64, 8, 64), (1.0, 1.0, 0.0)),              # smallest everything: one row, one input column, one column pair per half
    ((33, 33, 96, 40, 104), (0.5, 3.0, -2.0)),         # 3 column pairs: 2 + 1; A one past a k chunk; pad columns behind the sprites
    ((255, 64, 2048, 64, 2056), (2.0, 0.1, 5.0)),      # the largest A and n_out (32 pairs per half); one row short of a block
    ((65, 59, 1152, 64, 1152), (1.5, 0.25, 1.0)),      # A = 59 (the step's other width); one row past a wave's 64
    ((256, 16, 160, 16, 168), (3.0, 0.5, -0.5)),       # A = 16, ld_za = A; 5 column pairs: 3 + 2; exactly one row block
]


@pytest.mark.parametrize("shape,scales", FWD_CASES, ids=["n%d_a%d_o%d" % c[0][:3] for c in FWD_CASES])
def test_decoder_fwd16_edges(shape, scales):
    N, A, n_out, ld_za, ld_s = shape
    obj_s, al_s, al_b = scales
    L = _lib()
    lib = L.lib()
    lib.spair_decoder_fwd16_scratch_bytes.restype = ctypes.c_int64
    rec = Record("decoder fwd N %d A %d n_out %d ld_za %d ld_s %d" % shape)
    g = _gen(4000 + N + A)
    za = _padded(_bf(torch.randn(N, A, generator=g)), ld_za)
    W0, b0 = (torch.randn(H1, A, generator=g) * 0.2).to(DEV), (torch.randn(H1, generator=g) * 0.1).to(DEV)
    W1, b1 = (torch.randn(H2, H1, generator=g) * 0.1).to(DEV), (torch.randn(H2, generator=g) * 0.1).to(DEV)
    W2, b2 = (torch.randn(n_out, H2, generator=g) * 0.08).to(DEV), (torch.randn(n_out, generator=g) * 0.1).to(DEV)
    h1, h2 = Guarded(N, H1, H1, torch.bfloat16, DEV), Guarded(N, H2, H2, torch.bfloat16, DEV)
    S = Guarded(N, n_out, ld_s, torch.float16, DEV)
    scratch = torch.full((int(lib.spair_decoder_fwd16_scratch_bytes(n_out)) // 2,), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = lib.spair_decoder_fwd16(_p(za), ld_za, _p(W0), _p(b0), _p(W1), _p(b1), _p(W2), _p(b2), _p(h1), _p(h2), _p(S), ld_s, ctypes.c_longlong(N),
                                 A, n_out, ctypes.c_float(obj_s), ctypes.c_float(al_s), ctypes.c_float(al_b), _p(scratch), L.stream())
    assert rc == OK, rc
    # hidden layers, each on the kernel's own stored input; the summed block: 8 input columns from the middle (A < 16: the first ones)
    x0, w0 = d64(za[:, :A]), d64(_bf(W0))
    c0 = A // 2 // 8 * 8
    hold(rec, "H1", h1.block, x0 @ w0.T + d64(b0), U * (x0.abs() @ w0.abs().T + d64(b0).abs()), relu=True, part=x0[:, c0:c0 + 8] @ w0[:, c0:c0 + 8].T)
    x1, w1 = d64(h1.block), d64(_bf(W1))
    hold(rec, "H2", h2.block, x1 @ w1.T + d64(b1), U * (x1.abs() @ w1.abs().T + d64(b1).abs()), relu=True, part=x1[:, 64:72] @ w1[:, 64:72].T)

    # decoder.out: the exp2 argument of the analytic sigmoid.  Weights: W2[n] * (-scale_n * log2(e)) in fp32 (the factor itself an fp32
    # product), THEN bf16.  Bias term: even columns -(b obj_scale) log2(e), odd -(b alpha_scale + alpha_bias) log2(e), in fp32 (the kernel
    # may contract the multiply-add: within an ulp of the term, which beta's |bias term| covers 2^12 times over).
    def exp2_arg(grey_scale, alpha_scale):
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)
        odd = (torch.arange(n_out, device=DEV) % 2 == 1)
        sc = torch.where(odd, -f32(alpha_scale) * f32(L2E), -f32(grey_scale) * f32(L2E))
        w2 = d64(_bf(W2 * sc[:, None]))
        bt = d64(torch.where(odd, -(b2 * f32(alpha_scale) + f32(al_b)) * f32(L2E), -(b2 * f32(grey_scale)) * f32(L2E)))
        return w2, bt

    x2 = d64(h2.block)
    w2, bt = exp2_arg(obj_s, al_s)
    u = x2 @ w2.T + bt
    beta = U * (x2.abs() @ w2.abs().T + bt.abs())
    w2s, bts = exp2_arg(al_s, obj_s)
    wrong = [("scales swapped", x2 @ w2s.T + bts), ("drop", u - x2[:, 128:136] @ w2[:, 128:136].T)]
    if obj_s == al_s:
        wrong = wrong[1:]           # (nothing to swap)
    check_sigmoid16(rec, "S", S.block, u, beta, wrong)
    for key, o in (("H1", h1), ("H2", h2), ("S", S)):
        _whole(rec, key, o)
    _done(rec)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spair_decoder_bwd16
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (N, A, n_out, ld_s, ld2, ld_dza): what it crosses
BWD_CASES = [
    (129, 50, 1568, 1568, 1568, 56),       # the benchmark's widths: 25 stages, the last 32 columns wide; a second row block of one row
    (1, 1, 64, 64, 64, 8),                 # smallest everything: one stage, one row, one output column
    (127, 33, 72, 80, 72, 40),             # two stages, the last 8 columns wide; d-logit rows wider than n_out
    (128, 64, 2048, 2048, 2056, 64),       # the largest A and n_out: 32 stages; W2^T rows wider than n_out; exactly one row block
    (130, 59, 1152, 1160, 1152, 64),       # 18 stages (no remainder of the three-stage rotation); A = 59
]


def _gate_rows(g, N, width):
    """A stored post-ReLU activation [N][width] holding the special gate values; on DEV with its expected gate."""
    m = _bf(torch.relu(torch.randn(N, width, generator=g)))
    planted = plant_special_gates(m)
    md = m.to(DEV)
    return md, special_gate(md, planted)


@pytest.mark.parametrize("shape", BWD_CASES, ids=["n%d_a%d_o%d" % c[:3] for c in BWD_CASES])
def test_decoder_bwd16_edges(shape):
    """dH2 = (dL W2) [H2 > 0], dH1 = (dH2 W1) [H1 > 0], d z_attr = dH1 W0 from the transposed bf16 weights, each on the kernel's own stored
    input: a gated-off element, exactly 0 in dH2, must also be the 0 the next layer summed."""
    N, A, n_out, ld_s, ld2, ld_dza = shape
    L = _lib()
    rec = Record("decoder bwd N %d A %d n_out %d ld_s %d ld2 %d ld_dza %d" % shape)
    g = _gen(5000 + N + A)
    dL = _padded(_bf(torch.randn(N, n_out, generator=g) * 0.05), ld_s)
    W2t = _padded(_bf(torch.randn(H2, n_out, generator=g) * 0.08), ld2)
    W1t = _bf(torch.randn(H1, H2, generator=g) * 0.1).to(DEV)
    W0t = _bf(torch.randn(A, H1, generator=g) * 0.2).to(DEV)
    h2, gate2 = _gate_rows(g, N, H2)
    h1, gate1 = _gate_rows(g, N, H1)
    dH2, dH1 = Guarded(N, H2, H2, torch.bfloat16, DEV), Guarded(N, H1, H1, torch.bfloat16, DEV)
    dza = Guarded(N, A, ld_dza, torch.float32, DEV)
    rc = L.lib().spair_decoder_bwd16(_p(dL), ld_s, _p(W2t), ld2, _p(W1t), _p(W0t), _p(h2), _p(h1), _p(dH2), _p(dH1), _p(dza), ld_dza,
                                     ctypes.c_longlong(N), A, n_out, L.stream())
    assert rc == OK, rc
    x, w = d64(dL[:, :n_out]), d64(W2t[:, :n_out])
    c0 = n_out // 2 // 8 * 8
    hold(rec, "dH2", dH2.block, x @ w.T, U * (x.abs() @ w.abs().T), gate=gate2, part=x[:, c0:c0 + 8] @ w[:, c0:c0 + 8].T)
    x, w = d64(dH2.block), d64(W1t)
    hold(rec, "dH1", dH1.block, x @ w.T, U * (x.abs() @ w.abs().T), gate=gate1, part=x[:, 128:136] @ w[:, 128:136].T)
    x, w = d64(dH1.block), d64(W0t)
    hold(rec, "dza", dza.block, x @ w.T, U * (x.abs() @ w.abs().T), part=x[:, 64:72] @ w[:, 64:72].T)
    for key, o in (("dH2", dH2), ("dH1", dH1), ("dza", dza)):
        _whole(rec, key, o)
    _done(rec)
