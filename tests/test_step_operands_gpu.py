"""Teacher-forced checks of the training step's kernels on the operands they actually read.

Every activation, gradient row buffer and prepared weight copy of a step has its own region of the workspace (carve(), engine.hip: nothing
is aliased), so after one real step each kernel's stored bf16 / fp32 inputs can be read back through ``SPAIR.workspace_view`` and the same
operation recomputed in float64.  The difference is then fp32 accumulation noise alone, not the percent-level chaos of whole-step
comparisons (every bf16 rounding in the 3G - 2 dependent chain steps re-rolls everything downstream).

(a) every parameter gradient is the float64 product of its stored operands: p.grad = sum over rows of dY^T X, bias = column sums of dY;
(b) backbone and decoder activations and data gradients, for samples 0, 1, B/2 and B - 1: a bf16 output is the round-to-nearest-even of the
    float64 value, either neighbour accepted only where that value lies within the accumulation bound of a rounding boundary; a gated-off
    element is exactly 0 (the gate: the stored activation > 0);
(c) the prepared weight copies of plain layout are bit-equal to the RNE bf16 (fp32 step: the fp32) parameters, zero padding included.

Bound (derived, not measured): |got - ref| <= 2^-12 sum_r |dY_r X_r| per element -- the worst-case fp32 accumulation error of a chain of
<= 2048 terms plus a split-K reduce is (2048 + 64) 2^-24 < 2^-12 of the terms' absolute sum.  Every bound is checked for sensitivity on the
reference data (no kernel is mutated): a weight or bias bound must reject the reference with one row split's worth of rows (1/32 of the
rows) removed and with its 8-column blocks shifted by one block (biases of fewer than 16 elements: the rows only); an activation or data-
gradient bound must reject the reference without one block of 8 summed input channels and with its channels shifted by one block.

Where a kernel rounds an operand itself, the reference does the same and says so: the bf16 step's per-wavefront weight gradients (wgrad_lin)
read fp32 rows and round both operands to bf16 on their way into LDS (their bias gradients sum the fp32 rows as loaded); the stem's weight-gradient kernels round the padded fp32 image to bf16.

Not such products, so not checked here: virtual_edge_element (the context rows of edge cells: per-sample partial sums of the chain's
context gradients, chain_edge_reduce) and attn.* (dead in the reference: no gradient).  Out of scope: the fused chain's per-cell forward math
(its split-bf16 box network is not a plain product; tests/test_chain_gpu.py holds it cell by cell) and the renderer (already held to float64).

Observed maxima per tensor, largest error as a fraction of its bound over configurations A - F (in brackets: where; -s prints every
configuration):
  box_network.body.dense0.weight                   0.00076 (E)
  box_network.body.dense0.bias                     0.00028 (E)
  box_network.body.dense1.weight                   0.00075 (E)
  box_network.body.dense1.bias                     0.00026 (E)
  box_network.output_layers.1.weight               0.00052 (E)
  box_network.output_layers.1.bias                 0.00014 (E)
  box_network.output_layers.0.weight               0.00053 (E)
  box_network.output_layers.0.bias                 0.00016 (E)
  object_encoder.dense0.weight                     0.00099 (D)
  object_encoder.dense0.bias                       0.00027 (E)
  object_encoder.dense1.weight                     0.00093 (B)
  object_encoder.dense1.bias                       0.00027 (E)
  object_encoder.out.weight                        0.00067 (E)
  object_encoder.out.bias                          0.00023 (D)
  z_network.body.dense0.weight                     0.00061 (E)
  z_network.body.dense0.bias                       0.00019 (E)
  z_network.body.dense1.weight                     0.00065 (A)
  z_network.body.dense1.bias                       0.00026 (E)
  z_network.output_layers.1.weight                 0.0019 (B)
  z_network.output_layers.1.bias                   0.001 (B)
  z_network.output_layers.0.weight                 0.00018 (E)
  z_network.output_layers.0.bias                   6.3e-05 (E)
  obj_network.dense0.weight                        0.0023 (A)
  obj_network.dense0.bias                          0.00086 (B)
  obj_network.dense1.weight                        0.0021 (A)
  obj_network.dense1.bias                          0.00091 (B)
  obj_network.out.weight                           0.0013 (B)
  obj_network.out.bias                             0.00057 (A)
  object_decoder.out.weight                        0.0017 (B)
  object_decoder.out.bias                          0.0013 (B)
  object_decoder.dense1.weight                     0.0014 (D)
  object_decoder.dense1.bias                       0.00081 (D)
  object_decoder.dense0.weight                     0.00049 (E)
  object_decoder.dense0.bias                       0.00087 (B)
  backbone.net.conv_1.weight                       0.0008 (D)
  backbone.net.conv_1.bias                         0.00015 (D)
  backbone.net.conv_2.weight                       0.00095 (D)
  backbone.net.conv_2.bias                         0.00047 (D)
  backbone.net.conv_3.weight                       0.00068 (D)
  backbone.net.conv_3.bias                         0.00027 (D)
  backbone.net.conv_4.weight                       0.00062 (C)
  backbone.net.conv_4.bias                         0.00022 (B)
  backbone.net.conv_5.weight                       0.00072 (D)
  backbone.net.conv_5.bias                         0.00028 (B)
  backbone.net.conv_out.weight                     0.00063 (D)
  backbone.net.conv_out.bias                       0.00039 (D)
  backbone.net.conv_0.weight (d act0 recomputed)   0.41 (C)
  backbone.net.conv_0.bias (d act0 recomputed)     0.13 (B)
  feat                                             0.0008 (D)
  backbone.net.conv_0.weight                       0.00067 (D)
  backbone.net.conv_0.bias                         0.00019 (D)
  act1                                             0.00091 (D)
  dact0                                            0.0016 (D)
  act2                                             0.00091 (D)
  dact1                                            0.0022 (D)
  act3                                             0.00069 (D)
  dact2                                            0.001 (D)
  act4                                             0.00051 (D)
  dact3                                            0.001 (D)
  act5                                             0.00051 (D)
  dact4                                            0.0012 (D)
  dact5                                            0.00084 (D)
  Hd1                                              0.0011 (D)
  Hd2                                              0.001 (D)
  dHd2                                             0.0019 (D)
  dHd1                                             0.0011 (D)
(the recomputed stem bound carries the bf16 rounding of the intermediate d act0, which dominates it; per configuration 0.32 - 0.41,
every other weight gradient <= 2.3e-3).  bf16 round-to-nearest: no element outside its interval; a few per million checked differ
from RNE(ref), each within its bound of a rounding boundary.  Gates: F stores 12,433 bf16-denormal act0 values (5,587 in the checked
samples), and conv_1's data gradient, gated by the stem kernel's sign bits, passes them as the stored value does; no kernel stored a
-0.0 activation, F's channels 32 - 39 (bias -0.0, non-positive weights) included, so that case cannot arise in the step.

The T_* configurations (other backbone topologies and network sizes, batch 4) stay inside the same figures: every weight gradient, activation
and data gradient <= 1.1e-3 of its bound in the bf16 ones (T_k6_fp32: 2.8e-3, obj_network.dense0.weight), the recomputed stem 0.46 - 0.56
(T_k6, whose d act0 comes out of a 6x6 conv_1's class-batched data gradient, T_stack5, T_feat64, T_attr59)."""
import math

import pytest
import torch

from f64_hold import U, Record, _bias_sensitivity, _sensitivity, check_out, d64, gate_of, lin_wgrad, rne16

pytestmark = pytest.mark.gpu

STEP = 3000              # past the training wheel
S2 = (2, 2, 2, 1, 1, 1)

# name -> (dtype, image [C, H, W], batch, SpairStep.flags[, a case of golden_inputs whose backbone topology and F / NP / A the step runs on])
CONFIGS = {
    "A_bench": ("bf16", [1, 128, 128], 256, 0),
    "A_bench_stem_stored": ("bf16", [1, 128, 128], 256, 8),      # flags bit 3: the stem's weight gradient from a stored d act0
    "B_configs3": ("bf16", [1, 256, 256], 64, 0),
    "C_b37": ("bf16", [1, 128, 128], 37, 0),
    "C_b37_per_wavefront": ("bf16", [1, 128, 128], 37, 1),
    "C_b37_implicit_gemm": ("bf16", [1, 128, 128], 37, 16 | 32 | 64),
    "D_fp32": ("f32", [1, 128, 128], 32, 0),
    "E_colour": ("bf16", [3, 48, 48], 4, 0),
    # directed: stem channels whose outputs are bf16 denormals, underflow to 0 or come out of negative-only sums (see edge_stem); flags bit 3
    # stores d act0, so conv_1's data gradient -- gated by the stem kernel's sign bits -- is compared element by element with the stored act0 > 0
    "F_edge_act0": ("bf16", [1, 128, 128], 8, 8),
    # other topologies and network sizes (tests/test_topology_cpu.py pins the kernels each runs; tests/test_topology_gpu.py holds the same
    # steps to the reference's fixtures): the T = 3 and T = 1 weight packs; the stem's weight gradient inside a k = 6 conv_1's data gradient
    # and a patch data gradient gated by the stored activation; a 1x1 stack of 3 behind 32 / 64 / 72-channel layers; a 1x1 layer outside a
    # stack of 4; cin = 64 in tap-parity order; the per-wavefront chain at F = 64, NP = 36; A = 59
    # (batch 4 throughout: the scenes' sample 1 is empty, and at batch 2 or 3 the rows the stem's sensitivity check drops -- the middle of
    # sample B / 2 -- would all be black pixels, which no weight-gradient bound can miss)
    "T_k3": ("bf16", [1, 48, 48], 4, 0, "t_k3"),
    "T_k6": ("bf16", [1, 48, 48], 4, 0, "t_k6"),
    "T_k6_fp32": ("f32", [1, 48, 48], 4, 0, "t_k6"),
    "T_deep8": ("bf16", [1, 48, 48], 4, 0, "t_deep8"),
    "T_stack5": ("bf16", [1, 32, 32], 4, 0, "t_stack5"),
    "T_shallow64": ("bf16", [1, 32, 32], 4, 0, "t_shallow64"),
    "T_feat64": ("bf16", [1, 48, 48], 4, 0, "t_feat64"),
    "T_attr59": ("bf16", [1, 48, 48], 4, 0, "o_attr59"),
}


def edge_stem(m):
    """Stem channels 0..31: weights scaled by 2^-(112 + c) and bias 0, so their ReLU outputs run from normal through bf16 denormal
    (below 2^-126) to underflow; channels 32..39: bias -0.0 and non-positive weights, so the background's sums are -0.0 or +0.0."""
    w, b = m.backbone.net.conv_0.weight, m.backbone.net.conv_0.bias
    with torch.no_grad():
        for c in range(32):
            w[c] *= 2.0 ** -(112 + c)
            b[c] = 0.0
        w[32:40] = -w[32:40].abs()
        b[32:40] = -0.0


TWEAKS = {"F_edge_act0": edge_stem}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------------------------------
def run_step(name):
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd import models
    from spair_pytorch_amd.data import scattered_digits
    import golden_inputs as gi
    from helpers import engine_config
    dtype, shape, B, flags = CONFIGS[name][:4]
    case = dict(gi.TOPO_CASES, **gi.ORACLE_CASES)[CONFIGS[name][4]] if len(CONFIGS[name]) > 4 else dict(I=shape[1], strides=S2)
    assert case["I"] == shape[1]
    # (engine_config puts the topology, F / NP / A, the image shape and STEP_FLAGS back afterwards)
    with engine_config(case):
        cfg.INPUT_IMAGE_SHAPE[0] = shape[0]
        torch.manual_seed(3)
        m = models.SPAIR(shape, None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
        if name in TWEAKS:
            TWEAKS[name](m)
        models.STEP_FLAGS = flags
        x = torch.from_numpy(scattered_digits(1234, B, shape[1], 11, channels=shape[0])[0]).cuda()
        g = torch.Generator().manual_seed(5)
        G = m._dims(B).G
        noise = dict(eps_box=torch.randn(B, 4, G, G, generator=g), eps_attr=torch.randn(B, cfg.N_ATTRIBUTES, G, G, generator=g),
                     eps_depth=torch.randn(B, 1, G, G, generator=g), u_pres=torch.rand(B, 1, G, G, generator=g))
        m.zero_grad()
        loss = m(x, STEP, noise=noise)[0]
        loss.backward()
        torch.cuda.synchronize()
        assert math.isfinite(loss.item())
        from spair_pytorch_amd import _lib as L
        e = m._last_engine()
        plan = dict(L.step_plan(e["dims"], e["workspace"].data_ptr(), flags), **L.step_plan_n(e["dims"], e["workspace"].data_ptr(), flags))
        views = {nm: L.workspace_view(e["dims"], e["workspace"].data_ptr(), nm, flags) for nm in L.workspace_view_names(e["dims"])}
        V = {nm: m.workspace_view(nm) for nm in views}
        # (padded: whole rows of the leading dimension -- not for a head's second transposed layer, whose columns start inside its rows)
        Vp = {nm: m.workspace_view(nm, padded=True) for nm in views
              if nm.startswith(("conv_w", "lin_w")) and not (nm.startswith("lin_wt.") and nm.endswith("output_layers.0"))}
    return m, e["dims"], plan, views, V, Vp


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) weight gradients
# ---------------------------------------------------------------------------------------------------------------------------------------------
def conv_taps(X, k, s, ho, wo):
    """The (ky, kx) tap views of NHWC input X for a k x k / stride-s valid convolution with an ho x wo output."""
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, X[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s, :]


def conv_wgrad(rec, key, grad_w, grad_b, dY, X, k, s, round_x, samples_per_chunk=8):
    """grad_w[co, ci, ky, kx] = sum over (b, y, x) of dY[b, y, x, co] X[b, s y + ky, s x + kx, ci] (NHWC operands, valid convolution)."""
    B, ho, wo, co = dY.shape
    ci = X.shape[3]
    dev = dY.device
    acc = torch.zeros(co, ci, k, k, dtype=torch.float64, device=dev)
    absb, drop = torch.zeros_like(acc), torch.zeros_like(acc)
    # one row split's worth of (b, y, x) rows (1/32), centred on the middle pixel of sample B/2 (the image border is padding: zero rows)
    rdrop = B * ho * wo // 32
    ra = max(0, (B // 2) * ho * wo + (ho * wo) // 2 - rdrop // 2)
    bsum = torch.zeros(co, dtype=torch.float64, device=dev)
    babs, bdrop = torch.zeros_like(bsum), torch.zeros_like(bsum)
    for b0 in range(0, B, samples_per_chunk):
        a = d64(dY[b0:b0 + samples_per_chunk])
        xx = X[b0:b0 + samples_per_chunk]
        xx = d64(xx.to(torch.bfloat16) if round_x else xx)
        nb = a.shape[0]
        a2 = a.reshape(-1, co)
        row0 = b0 * ho * wo
        d0, d1 = max(ra - row0, 0), min(ra + rdrop - row0, a2.shape[0])
        for ky, kx, xs in conv_taps(xx, k, s, ho, wo):
            x2 = xs.reshape(nb * ho * wo, ci)
            acc[:, :, ky, kx] += a2.T @ x2
            absb[:, :, ky, kx] += a2.abs().T @ x2.abs()
            if d1 > d0:
                drop[:, :, ky, kx] += a2[d0:d1].T @ x2[d0:d1]
        bsum += a2.sum(0)
        babs += a2.abs().sum(0)
        if d1 > d0:
            bdrop += a2[d0:d1].sum(0)
    bound = U * absb.reshape(co, -1) + 1e-30
    ref = acc.reshape(co, -1)
    rec.ratio_max(key + ".weight", ((d64(grad_w).reshape(co, -1) - ref).abs() / bound).max())
    _sensitivity(rec, key + ".weight", ref, bound, drop.reshape(co, -1))
    bb = U * babs + 1e-30
    rec.ratio_max(key + ".bias", ((d64(grad_b) - bsum).abs() / bb).max())
    _bias_sensitivity(rec, key + ".bias", bsum, bb, bdrop)
    rec.covered |= {key + ".weight", key + ".bias"}


def dgrad64(dY, W, k, s, hi, wi, part=False):
    """d X[b, s y + ky, s x + kx, ci] += sum_co dY[b, y, x, co] W[co, ci, ky, kx] in float64, and the same sum of absolute terms (part: and the
    contribution of the 8 output channels from co / 2 on)."""
    B, ho, wo, co = dY.shape
    ci = W.shape[1]
    out = torch.zeros(B, hi, wi, ci, dtype=torch.float64, device=dY.device)
    ab = torch.zeros_like(out)
    pt = torch.zeros_like(out) if part else None
    for ky in range(k):
        for kx in range(k):
            w = W[:, :, ky, kx]
            sl = (slice(None), slice(ky, ky + s * (ho - 1) + 1, s), slice(kx, kx + s * (wo - 1) + 1, s))
            out[sl] += dY @ w
            ab[sl] += dY.abs() @ w.abs()
            if part:
                h = co // 2
                pt[sl] += dY[..., h:h + 8] @ w[h:h + 8]
    return (out, ab, pt) if part else (out, ab)


def stem_wgrad_from_recomputed_dact0(rec, key, grad_w, grad_b, dact1, act0, W1, xpad, k1, s1, k0, s0, samples_per_chunk=8):
    """The default plan takes the stem's weight gradient inside conv_1's data-gradient tile: d act0 is never stored.  Recompute it in
    float64 from the stored d act1, the bf16 conv_1 weights and the act0 gate, and bound the product by the accumulation bound plus the error
    of that intermediate: the kernel's d act0 element is an fp32 sum of <= 2048 terms (error <= 2^-12 A, A its absolute terms), rounded to
    bf16 for the stem product (8 significant bits: a further <= 2^-8 of its magnitude, the bf16 unit roundoff): e = 2^-8 (|d| + 2^-12 A)
    + 2^-12 A.  The padded image is rounded to bf16 by the kernel, and here.  The bound is checked for sensitivity as the others are."""
    B, h0, w0, c0 = act0.shape
    _, h1, w1, _ = dact1.shape
    dev = dact1.device
    acc = torch.zeros(c0, k0 * k0, dtype=torch.float64, device=dev)
    absb, err = torch.zeros_like(acc), torch.zeros_like(acc)
    drop = torch.zeros_like(acc)
    bsum = torch.zeros(c0, dtype=torch.float64, device=dev)
    babs, berr, bdrop = torch.zeros_like(bsum), torch.zeros_like(bsum), torch.zeros_like(bsum)
    rdrop = B * h0 * w0 // 32          # one row split's worth of (b, y, x) rows, centred on the middle pixel of sample B/2 (as conv_wgrad)
    ra = max(0, (B // 2) * h0 * w0 + (h0 * w0) // 2 - rdrop // 2)
    for b0 in range(0, B, samples_per_chunk):
        dd, A = dgrad64(d64(dact1[b0:b0 + samples_per_chunk]), W1, k1, s1, h0, w0)
        gate = act0[b0:b0 + samples_per_chunk] > 0
        dd, A = dd * gate, A * gate
        e = 2.0 ** -8 * (dd.abs() + U * A) + U * A
        xx = d64(xpad[b0:b0 + samples_per_chunk].to(torch.bfloat16))
        a2, e2 = dd.reshape(-1, c0), e.reshape(-1, c0)
        row0 = b0 * h0 * w0
        d0, d1 = max(ra - row0, 0), min(ra + rdrop - row0, a2.shape[0])
        for ky, kx, xs in conv_taps(xx, k0, s0, h0, w0):
            x2 = xs.reshape(-1)
            t = ky * k0 + kx
            acc[:, t] += a2.T @ x2
            absb[:, t] += a2.abs().T @ x2.abs()
            err[:, t] += e2.T @ x2.abs()
            if d1 > d0:
                drop[:, t] += a2[d0:d1].T @ x2[d0:d1]
        bsum += a2.sum(0)
        babs += a2.abs().sum(0)
        berr += e2.sum(0)
        if d1 > d0:
            bdrop += a2[d0:d1].sum(0)
    bound = U * absb + err + 1e-30
    rec.ratio_max(key + ".weight (d act0 recomputed)", ((d64(grad_w).reshape(c0, -1) - acc).abs() / bound).max())
    _sensitivity(rec, key + ".weight (d act0 recomputed)", acc, bound, drop)
    bb = U * babs + berr + 1e-30
    rec.ratio_max(key + ".bias (d act0 recomputed)", ((d64(grad_b) - bsum).abs() / bb).max())
    _bias_sensitivity(rec, key + ".bias (d act0 recomputed)", bsum, bb, bdrop)
    rec.covered |= {key + ".weight", key + ".bias"}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (b) activations and data gradients
# ---------------------------------------------------------------------------------------------------------------------------------------------
def conv_fwd64(X, W, bias, k, s, ho, wo):
    """The valid convolution in float64, the sum of its absolute terms, and the contribution of the 8 input channels from ci / 2 on."""
    co = W.shape[0]
    out = bias.view(1, 1, 1, co).expand(X.shape[0], ho, wo, co).clone()
    ab = bias.abs().view(1, 1, 1, co).expand_as(out).clone()
    pt = torch.zeros_like(out)
    for ky, kx, xs in conv_taps(X, k, s, ho, wo):
        w = W[:, :, ky, kx]
        out += xs @ w.T
        ab += xs.abs() @ w.abs().T
        h = xs.shape[-1] // 2
        pt += xs[..., h:h + 8] @ w[:, h:h + 8].T
    return out, ab, pt


def tap_parity_columns(ci, k, s):
    """(ci, ky, kx) of each column of a bf16 strided conv's forward matrix in tap-parity K order (gemm16.hip GemmNT::ktab, misc.hip mode 2):
    64-column blocks = (parity class, channel block, tap of the class)."""
    T, nh = k // s, ci // 64
    c = torch.arange(k * k * ci)
    blk = c // 64
    tq, rr = blk % (T * T), blk // (T * T)
    h, cls = rr % nh, rr // nh
    return h * 64 + c % 64, cls // s + s * (tq // T), cls % s + s * (tq % T)


# ---------------------------------------------------------------------------------------------------------------------------------------------
def check_config(name):
    m, d, plan, views, V, Vp = run_step(name)
    rec = Record(name)
    B, b16 = d.B, d.dtype == 1
    wq = (lambda p: d64(rne16(p.detach()))) if b16 else (lambda p: d64(p.detach()))      # the step's weights as its kernels read them
    P = dict(m.named_parameters())
    n = d.n_conv
    F, A, NP = d.F, d.A, d.NP
    chain = plan["chain"]
    # ---- the model's wiring (reference concatenation order): [features F | context 4 (4 + A + 2) | passthrough NP | box 4 | attr A | depth]
    nfc = F + 4 * (4 + A + 2)
    zin = nfc + NP + 4 + A
    sprite = d.P * d.P * (d.C + 1)

    def first_layer_input(rows):      # the z / obj nets' first layers: the fused chain keeps [features | context] once, in Xb
        if chain:
            return torch.cat([V["Xb"][:, :nfc].contiguous(), V[rows][:, nfc:].contiguous()], 1)
        return V[rows].contiguous()
    cells = [
        ("box_network.body.dense0", V["dHb1"], V["Xb"]),
        ("box_network.body.dense1", V["dHb2"], V["Hb1"]),
        ("box_network.output_layers.1", V["dOb"][:, :NP], V["Hb2"]),
        ("box_network.output_layers.0", V["dOb"][:, NP:NP + 8], V["Hb2"]),
        ("object_encoder.dense0", V["dHe1"], V["glimpse"]),
        ("object_encoder.dense1", V["dHe2"], V["He1"]),
        ("object_encoder.out", V["dOe"], V["He2"]),
        ("z_network.body.dense0", V["dHz1"], first_layer_input("Xz")),
        ("z_network.body.dense1", V["dHz2"], V["Hz1"]),
        ("z_network.output_layers.1", V["dOz"][:, :NP], V["Hz2"]),
        ("z_network.output_layers.0", V["dOz"][:, NP:NP + 2], V["Hz2"]),
        ("obj_network.dense0", V["dHo1"], first_layer_input("Xo")),
        ("obj_network.dense1", V["dHo2"], V["Ho1"]),
        ("obj_network.out", V["dOo"], V["Ho2"]),
    ]
    assert views["Xz"]["cols"] == zin and views["Xo"]["cols"] == zin + 1
    # per-wavefront launches in the bf16 step: fp32 rows, rounded to bf16 by the weight-gradient kernel (gemm.hip) -- and here
    round_rows = b16 and not chain
    for key, dY, X in cells:
        lin_wgrad(rec, key, P[key + ".weight"].grad, P[key + ".bias"].grad, dY, X, round_rows)
    # decoder: d logits (bf16 step: as its weight gradient reads them -- the bf16 copy of fp32 ones), hidden layers, the z_attr rows
    dL = V["dLog16"] if "dLog16" in V else V["dLog"]
    Za = V["Za16"] if b16 else V["Za"]
    dec = [("object_decoder.out", dL, V["Hd2"]), ("object_decoder.dense1", V["dHd2"], V["Hd1"]), ("object_decoder.dense0", V["dHd1"], Za)]
    for key, dY, X in dec:
        lin_wgrad(rec, key, P[key + ".weight"].grad, P[key + ".bias"].grad, dY, X, False)
    # backbone: layer i reads act<i-1> (NHWC), its output gradient is d act<i> (d feat for conv_out)
    layers = []
    for i in range(n + 1):
        conv = "backbone.net.conv_%d" % i if i < n else "backbone.net.conv_out"
        w = P[conv + ".weight"]
        co, ci, k, _ = w.shape
        s = d.conv_s[i] if i < n else 1
        layers.append((conv, co, ci, k, s))
    shapes = {}
    Ip = d.I + d.pad_pre + d.pad_post
    shapes[-1] = (Ip, Ip)
    for i in range(n + 1):
        hi = shapes[i - 1][0]
        ho = (hi - layers[i][3]) // layers[i][4] + 1
        shapes[i] = (ho, ho)

    def act(i):
        if i == -1:
            return V["xpad"].reshape(B, Ip, Ip, d.C)
        if i == n:
            return V["feat"].reshape(B, d.G, d.G, F)
        return V["act%d" % i].reshape(B, *shapes[i], layers[i][1])

    def dact(i):
        if i == n:
            return (V["dfeat16"] if b16 else V["dfeat"]).reshape(B, d.G, d.G, F)
        return V["dact%d" % i].reshape(B, *shapes[i], layers[i][1])
    for i in range(1, n + 1):
        conv, co, ci, k, s = layers[i]
        conv_wgrad(rec, conv, P[conv + ".weight"].grad, P[conv + ".bias"].grad, dact(i), act(i - 1), k, s, False)
    conv, co, ci, k0, s0 = layers[0]
    if views["dact0"]["written"]:
        # the padded fp32 image: rounded to bf16 by the bf16 step's stem weight-gradient kernels (gemm16.hip, conv_s2_dgrad.hip) -- and here
        conv_wgrad(rec, conv, P[conv + ".weight"].grad, P[conv + ".bias"].grad, dact(0), act(-1), k0, s0, b16)
    else:
        _, _, _, k1, s1 = layers[1]
        stem_wgrad_from_recomputed_dact0(rec, conv, P[conv + ".weight"].grad, P[conv + ".bias"].grad, dact(1), act(0),
                                         wq(P["backbone.net.conv_1.weight"]), act(-1), k1, s1, k0, s0)

    # ---- (b) four samples
    smp = sorted({0, 1, B // 2, B - 1})
    idx = torch.tensor(smp, device="cuda")
    for i in range(1, n + 1):
        conv, co, ci, k, s = layers[i]
        X = d64(act(i - 1)[idx])
        ho, wo = shapes[i]
        ref, ab, pt = conv_fwd64(X, wq(P[conv + ".weight"]), d64(P[conv + ".bias"].detach()), k, s, ho, wo)
        check_out(rec, "act%d" % i if i < n else "feat", act(i)[idx], ref, U * ab, relu=i < n, part=pt)
        # data gradient into act<i-1>, gated by the stored act<i-1> > 0
        if i > 1 or views["dact0"]["written"]:
            dref, dab, dpt = dgrad64(d64(dact(i)[idx]), wq(P[conv + ".weight"]), k, s, *shapes[i - 1], part=True)
            check_out(rec, "dact%d" % (i - 1), dact(i - 1)[idx], dref, U * dab, gate=gate_of(act(i - 1)[idx]), part=dpt)
    if name in TWEAKS:      # the directed configuration must actually hold the edge values it is there for
        _, neg0, den = gate_of(act(0))
        rec.notes.append("act0 (whole batch): %d -0.0, %d bf16 denormals" % (neg0, den))
        if not den:
            rec.fail("act0", "no bf16-denormal activation to gate")
    if b16 and views["dfeat"]["written"]:
        check_out(rec, "dfeat16 = RNE(dfeat)", V["dfeat16"], d64(V["dfeat"]), torch.zeros_like(d64(V["dfeat"])))
    if "dLog16" in V:
        check_out(rec, "dLog16 = RNE(dLog)", V["dLog16"], d64(V["dLog"]), torch.zeros_like(d64(V["dLog"])))
    rows = torch.cat([torch.arange(b, views["Hd1"]["rows"], B, device="cuda") for b in smp])      # rows r = cprime B + b
    W0, W1, W2 = (wq(P["object_decoder.%s.weight" % k]) for k in ("dense0", "dense1", "out"))
    b0, b1 = (d64(P["object_decoder.%s.bias" % k].detach()) for k in ("dense0", "dense1"))
    z = d64(Za[rows])
    h1 = d64(V["Hd1"][rows])
    a0 = A // 2 // 8 * 8      # one block of 8 of the A summed attributes (24 at A = 50)
    check_out(rec, "Hd1", V["Hd1"][rows], z @ W0.T + b0, U * (z.abs() @ W0.abs().T + b0.abs()), relu=True, part=z[:, a0:a0 + 8] @ W0[:, a0:a0 + 8].T)
    check_out(rec, "Hd2", V["Hd2"][rows], h1 @ W1.T + b1, U * (h1.abs() @ W1.abs().T + b1.abs()), relu=True, part=h1[:, 64:72] @ W1[:, 64:72].T)
    g = d64(dL[rows])
    check_out(rec, "dHd2", V["dHd2"][rows], g @ W2, U * (g.abs() @ W2.abs()), gate=gate_of(V["Hd2"][rows]), part=g[:, 400:408] @ W2[400:408])
    g2 = d64(V["dHd2"][rows])
    check_out(rec, "dHd1", V["dHd1"][rows], g2 @ W1, U * (g2.abs() @ W1.abs()), gate=gate_of(V["Hd1"][rows]), part=g2[:, 128:136] @ W1[128:136])
    assert sprite == views["dLog"]["cols"]

    # ---- (c) prepared weight copies: bit-equal, zero padding included
    def prepared(p):
        return p.detach().to(torch.bfloat16) if b16 else p.detach()

    def same(key, got_padded, want, cols):
        full = torch.zeros_like(got_padded)
        full[:, :cols] = want
        if not torch.equal(got_padded.view(torch.int16 if b16 else torch.int32), full.view(torch.int16 if b16 else torch.int32)):
            rec.fail(key, "prepared copy differs from the parameters")
    for i in range(1, n + 1):
        conv, co, ci, k, s = layers[i]
        w = prepared(P[conv + ".weight"])                       # [co][ci][k][k]
        if b16 and k > 1 and s > 1 and k % s == 0 and ci % 64 == 0 and k * k * ci // 64 <= 64:      # engine.hip conv_kperm
            cc, ky, kx = tap_parity_columns(ci, k, s)
            same("conv_wf%d" % i, Vp["conv_wf%d" % i], w[:, cc, ky, kx], k * k * ci)
        else:       # [co][(ky k + kx) ci + ci']
            same("conv_wf%d" % i, Vp["conv_wf%d" % i], w.permute(0, 2, 3, 1).reshape(co, -1), k * k * ci)
        if k == 1:
            same("conv_wd%d_0" % i, Vp["conv_wd%d_0" % i], w.reshape(co, ci).T, co)
        else:
            T = k // s
            for py in range(s):
                for px in range(s):
                    sub = w[:, :, py::s, px::s][:, :, :T, :T]          # [co][ci][ty][tx] -> [ci][(ty T + tx) co + co']
                    same("conv_wd%d_%d" % (i, py * s + px), Vp["conv_wd%d_%d" % (i, py * s + px)], sub.permute(1, 2, 3, 0).reshape(ci, -1),
                         T * T * co)
    for key in [c[0] for c in cells] + [c[0] for c in dec]:
        w = prepared(P[key + ".weight"])
        if key.endswith("output_layers.0"):
            continue        # (with its head's first layer below)
        if key.endswith("output_layers.1"):
            # a head's two layers share one matrix: [out1 + out0][in] forward rows (out0's rows behind out1's), [in][out1 | out0] transposed
            w0 = prepared(P[key[:-1] + "0.weight"])
            same("lin_wf." + key, Vp["lin_wf." + key], w, w.shape[1])
            same("lin_wf." + key[:-1] + "0", Vp["lin_wf." + key[:-1] + "0"], w0, w0.shape[1])
            same("lin_wt." + key, Vp["lin_wt." + key], torch.cat([w.T, w0.T], 1), w.shape[0] + w0.shape[0])
            continue
        same("lin_wf." + key, Vp["lin_wf." + key], w, w.shape[1])
        same("lin_wt." + key, Vp["lin_wt." + key], w.T, w.shape[0])
    # every parameter gradient is checked above, or is one of the stated exclusions
    unchecked = {k for k, p in P.items() if p.grad is not None} - rec.covered
    if unchecked != {"virtual_edge_element"}:
        rec.fail("coverage", "parameter gradients neither checked nor excluded: %s" % sorted(unchecked - {"virtual_edge_element"}))
    if any(p.grad is not None for k, p in P.items() if k.startswith("attn.")):
        rec.fail("coverage", "attn.* received a gradient")
    del m, V, Vp
    torch.cuda.empty_cache()
    rec.report()
    return rec


@pytest.mark.parametrize("name", list(CONFIGS))
def test_step_kernels_hold_to_float64_on_their_stored_operands(name):
    rec = check_config(name)
    assert not rec.bad, rec.bad
