"""Directed inputs that drive the per-cell latent transforms into their +-10 clamps, and the checks both test_latent_edges_cpu.py (on the
oracle alone) and test_latent_edges_gpu.py (on the HIP step) apply.  Plain module: no test lives here.

Base: strides (2,2,2,1,1,1), global_step 2500 (training wheel 0), make_weights(21, 1.0), scattered_digits(7 + B, B, I, 9),
make_noise(3 + B, B, G).  Regimes ("L" moves latents, "N" moves noise; cells are classed by (h + w) % 3):
  L-std   box log-std biases += (12, -12, 8, -8), depth log-std bias += 12, encoder log-std biases [0:10] += 12, [10:20] -= 12, [20:30] += 8
  L-pres  obj_network.out.weight *= 120: presence logits on both sides of the clamp, cell by cell
  N-eps   eps_box = +60 / -60 and eps_depth = -60 / +60 on classes 0 / 1; class 2 keeps its draws
  N-u     u_pres = 2^-25 / 1.0 on classes 0 / 1 (the generator's extremes, misc.hip u01), one class-2 cell at 1 - 2^-24
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import golden_inputs as gi
from oracle import spair_oracle as orc

S2 = (2, 2, 2, 1, 1, 1)
GS = 2500
A = gi.N_ATTR
DELTA = 0.05                 # the kernel's own fp32 latents decide the masks: nothing within DELTA of +-10 is asserted either way
PRES_BAND = 0.5              # the reference-side conditioning band of L-pres (CPU test)
MIN_COUNT = 20               # every zero / non-zero assertion covers at least this many elements on each side
MAX_BAND_SHARE = 0.10
NAMES = ["box_lat", "enc_out", "depth_lat", "pres_logit"]
ALL = ("L-std", "L-pres", "N-eps")
TARGETS = ("loss", "z_where", "recon", "z_pres")

# The reference's own fp32-versus-float64 spread (largest absolute difference of the fp32 and the float64 oracle), re-measured and held by
# test_latent_edges_cpu.py (measured 1.35e-7, 3.45e-7, 7.0e-8; the constants leave headroom inside its <= 3 x window): forward values
# under L-std + N-eps and under N-u; the loss under N-u (relative).
SPREAD = {"z_where": 2.0e-7, "z_depth": 5.0e-7, "z_pres": 1.2e-7, "loss_nu": 1.2e-6}
FWD_FACTOR = 10.0            # a forward value may differ from the fp32 oracle by FWD_FACTOR * SPREAD
# Bounds of tests/test_chain_gpu.py::test_per_cell_latent_gradients_vs_oracle, unchanged: (cell, floor, whole map, loss)
F32_BOUNDS = (2e-3, 1e-4, 1e-3, 2e-5)
BF16_BOUNDS = (0.15, 5e-3, 0.03, 2.5e-4)


def cell_class(G):
    h, w = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    return (h + w) % 3


def inputs(regimes, I=48, B=4, pres_scale=120.0):
    """(weights {key: ndarray}, image ndarray, noise {key: ndarray}, G) of the base geometry with ``regimes`` applied."""
    from spair_pytorch_amd.data import scattered_digits
    G = gi.grid_side(I, S2)
    w = {k: v.copy() for k, v in gi.make_weights(21, 1.0).items()}
    x = scattered_digits(7 + B, B, I, 9)[0]
    noise = {k: v.copy() for k, v in gi.make_noise(3 + B, B, G).items()}
    cls = cell_class(G)
    c0, c1 = cls == 0, cls == 1
    for r in regimes:
        if r == "L-std":
            w["box_network.output_layers.0.bias"][4:8] += np.float32([12, -12, 8, -8])
            w["z_network.output_layers.0.bias"][1] += 12
            b = w["object_encoder.out.bias"]
            b[A:A + 10] += 12
            b[A + 10:A + 20] -= 12
            b[A + 20:A + 30] += 8
        elif r == "L-pres":
            w["obj_network.out.weight"] *= np.float32(pres_scale)
        elif r == "N-eps":
            noise["eps_box"][:, :, c0], noise["eps_box"][:, :, c1] = 60.0, -60.0
            noise["eps_depth"][:, :, c0], noise["eps_depth"][:, :, c1] = -60.0, 60.0
        elif r == "N-u":
            noise["u_pres"][:, :, c0], noise["u_pres"][:, :, c1] = 2.0 ** -25, 1.0
            noise["u_pres"][0, 0, 0, 2] = 1.0 - 2.0 ** -24
        else:
            raise KeyError(r)
    return w, x, noise, G


def aux(B, I, G):
    from test_output_grads_gpu import aux_weights
    return aux_weights((B, 1, I, I), (B, 4, G, G), (B, 1, G, G))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
class _TorchWithoutPresenceClamp:
    """``torch`` as the oracle sees it, with the presence logit's clamp -- the one call with float literals, clamp(x, -10.0, 10.0) -- removed."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def clamp(x, *a, **k):
        if len(a) == 2 and isinstance(a[0], float) and a == (-10.0, 10.0):
            return x
        return torch.clamp(x, *a, **k)


class _RoundGrad(torch.autograd.Function):
    """Identity whose gradient is rounded to bf16: a gradient row buffer of the bf16 step."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class _LinearBwd16(torch.autograd.Function):
    """x W^T + b on the parameters as given; the data gradient from the bf16 copy of W (the step's prepared transposed weights)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return g @ w.to(torch.bfloat16).to(w.dtype), g.t() @ x, g.sum(0)


_round_grad, _linear_bwd16 = _RoundGrad.apply, _LinearBwd16.apply


def _mutated(mutation):
    """name -> replacement of the oracle module's attributes for one mutated reference."""
    if mutation == "no_sigmoid_clamps":
        def latent_to_mean_std(lat):
            mean, log_std = torch.chunk(lat, 2, dim=-1)
            return mean, torch.sigmoid(log_std) * 2

        def clamped_sigmoid(x, analytical=False):
            return 1 / ((-x).exp() + 1) if analytical else torch.sigmoid(x)
        return dict(latent_to_mean_std=latent_to_mean_std, clamped_sigmoid=clamped_sigmoid)
    if mutation == "no_presence_clamp":
        return dict(torch=_TorchWithoutPresenceClamp())
    if mutation == "sigmoid_clamps_at_5":
        def latent_to_mean_std(lat):
            mean, log_std = torch.chunk(lat, 2, dim=-1)
            return mean, torch.sigmoid(log_std.clamp(-5, 5)) * 2

        def clamped_sigmoid(x, analytical=False):
            return 1 / ((-x).exp() + 1) if analytical else torch.sigmoid(torch.clamp(x, -5, 5))
        return dict(latent_to_mean_std=latent_to_mean_std, clamped_sigmoid=clamped_sigmoid)
    raise KeyError(mutation)


TIE_MARGIN = 5e-4


def _tie_patch(box_sides, overrides):
    """Replacement of the oracle's _mlp that resolves the box network's ReLU ties: a hidden unit whose pre-activation lies within TIE_MARGIN of
    zero takes the side ``box_sides`` gives (two bool tensors [B, G * G, units], one per layer); every other unit keeps its own.
    overrides[0] counts the units whose side this changed."""
    inner, calls = orc._mlp, [0]

    def mlp_sides(p_, prefix, x_, n_hidden=2, multi=False):
        if prefix != "box_network":
            return inner(p_, prefix, x_, n_hidden, multi)
        cell = calls[0]
        calls[0] += 1
        for i in range(n_hidden):
            pre = F.linear(x_, p_[f"{prefix}.body.dense{i}.weight"], p_[f"{prefix}.body.dense{i}.bias"])
            side = pre.detach() > 0
            flip = (pre.detach().abs() < TIE_MARGIN) & (box_sides[i][:, cell, :pre.shape[1]] != side)
            overrides[0] += int(flip.sum())
            x_ = pre * (side ^ flip).to(pre.dtype)
        return [F.linear(x_, p_[f"{prefix}.output_layers.{i}.weight"], p_[f"{prefix}.output_layers.{i}.bias"]) for i in range(2)]
    return dict(_mlp=mlp_sides)


def _bf16_weights(w):
    """Every weight matrix / filter bank rounded to bf16 (nearest even), as the bf16 step's kernels read them; not the box network's, which
    the fused kernel runs as split-bf16 products (fp32 to 1e-5); biases stay fp32."""
    return {k: (torch.from_numpy(v).to(torch.bfloat16).float().numpy() if v.ndim >= 2 and not k.startswith("box_network.") else v)
            for k, v in w.items()}


def _q16(t):
    """t rounded to bf16, straight through."""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


def _bf16_patch():
    """Replacements of the oracle's backbone_forward and _mlp that round what the bf16 step rounds: backbone activations, every layer input
    of the encoder, depth, presence and decoder networks, every gradient row; the box network exact forward, its data gradients from the bf16
    weight copies."""
    def backbone16(p_, x_, cfg_):
        pre, post, _, _, _ = orc.backbone_geometry(cfg_.image_shape[1], cfg_.conv_kernels, cfg_.conv_strides)
        h = F.pad(x_, (pre, post, pre, post))
        for i, s_ in enumerate(cfg_.conv_strides):
            h = _q16(F.relu(F.conv2d(h, p_[f"backbone.net.conv_{i}.weight"], p_[f"backbone.net.conv_{i}.bias"], stride=s_)))
        return F.conv2d(h, p_["backbone.net.conv_out.weight"], p_["backbone.net.conv_out.bias"])

    def mlp16(p_, prefix, x_, n_hidden=2, multi=False):
        box = prefix == "box_network"
        lin = _linear_bwd16 if box else (lambda x, w, b: F.linear(_q16(x), w, b))
        body = prefix + (".body" if multi else "")
        for i in range(n_hidden):
            x_ = F.relu(_round_grad(lin(x_, p_[f"{body}.dense{i}.weight"], p_[f"{body}.dense{i}.bias"])))
        heads = [f"{prefix}.output_layers.{i}" for i in range(2)] if multi else [f"{prefix}.out"]
        outs = [lin(x_, p_[h + ".weight"], p_[h + ".bias"]) for h in heads]
        outs = outs if box else [_round_grad(o) for o in outs]
        return outs if multi else outs[0]
    return dict(backbone_forward=backbone16, _mlp=mlp16)


@functools.lru_cache(maxsize=None)
def oracle_run(regimes, dtype="f32", targets=("loss",), mutation=None, I=48, B=4, bf16_operands=False):
    """oracle_step, computed once per process and never modified."""
    return oracle_step(regimes, dtype, targets, mutation, I, B, bf16_operands)


def oracle_step(regimes, dtype="f32", targets=("loss",), mutation=None, I=48, B=4, bf16_operands=False, box_sides=None):
    """One oracle step on ``inputs(regimes)`` in fp32 or float64.  Returns loss, z_where, z_pres, z_depth, recon, ``latents`` (the four
    networks' raw outputs per cell as [B, ch, G, G] maps) and ``grads[target][name]``: d target / d those, float64.  Targets: the loss, or
    (W * output).sum() with test_output_grads_gpu.aux_weights.  At most one of: ``mutation``, a reference with clamps missing or moved
    (_mutated); ``bf16_operands``, the reference on the operands the bf16 step reads (_bf16_weights, _bf16_patch), for
    bf16_operand_spread; ``box_sides``, the sides of the box network's two ReLU layers as a HIP step stored them, which the reference's
    ties take (_tie_patch).  The reference's gradient jumps across a ReLU kink, and which side a unit within rounding of zero lands on
    is an accident of that rounding (a bf16 step reads bf16 features: 2^-9 relative on the 324 inputs of the first layer is a
    pre-activation noise of about 2e-4, TIE_MARGIN is 2.5 of that).  Unlike test_output_grads_gpu.untie_decoder, which moves ties away in
    the weights both sides use, this reads the step's stored sides, for the tied units only; ``tie_overrides`` counts them."""
    assert (mutation is not None) + bool(bf16_operands) + (box_sides is not None) <= 1
    w, x, noise, G = inputs(regimes, I, B)
    dt = torch.float64 if dtype == "f64" else torch.float32
    overrides = [0]
    patch = {}
    if mutation:
        patch = _mutated(mutation)
    elif box_sides is not None:
        patch = _tie_patch(box_sides, overrides)
    elif bf16_operands:
        w, patch = _bf16_weights(w), _bf16_patch()
    p = {k: torch.from_numpy(v).to(dt).requires_grad_(not k.startswith("attn.")) for k, v in w.items()}
    ocfg = orc.OracleConfig(image_shape=(1, I, I), conv_strides=S2, inverse_mode="closed")
    taps = {}
    old = {}
    try:
        for k, v in patch.items():
            old[k] = getattr(orc, k)
            setattr(orc, k, v)
        out = orc.forward(p, torch.from_numpy(x).to(dt), GS, {k: torch.from_numpy(v).to(dt) for k, v in noise.items()}, ocfg, fast=mutation is None, taps=taps)
    finally:
        for k, v in old.items():
            setattr(orc, k, v)
    W = aux(B, I, G)
    outs = {"recon": out["recon_x"], "z_where": out["z_where"], "z_pres": out["z_pres"]}
    leaves = [t for n in NAMES for t in taps[n]]
    HW = G * G

    def maps(ts):
        return {n: torch.stack(ts[i * HW:(i + 1) * HW], dim=-1).reshape(B, -1, G, G).detach().double() for i, n in enumerate(NAMES)}
    grads = {}
    for t in targets:
        obj = out["loss"] if t == "loss" else (W[t].to(dt) * outs[t]).sum()
        g = torch.autograd.grad(obj, leaves, retain_graph=True, allow_unused=True)
        grads[t] = maps([torch.zeros_like(l) if gi_ is None else gi_ for l, gi_ in zip(leaves, g)])
    res = dict(loss=float(out["loss"].detach().double()), latents=maps(leaves), grads=grads, G=G, tie_overrides=overrides[0],
               noise={k: torch.from_numpy(v) for k, v in noise.items()})
    for k, v in (("z_where", out["z_where"]), ("z_pres", out["z_pres"]), ("z_depth", out["z_depth"]), ("recon", out["recon_x"])):
        res[k] = v.detach().double()
    return res


# ---------------------------------------------------------------------------------------------------------------------------------------------
# clamp inputs and the structural-zero assertions
# ---------------------------------------------------------------------------------------------------------------------------------------------
def clamp_inputs(lat, noise):
    """Every clamp input of a step (61 per cell) in float64 from the networks' raw outputs ``lat`` ([B, ch, G, G] maps) and the noise maps,
    at training wheel 0: z = mu + sd * eps with sd = 2 sigmoid(clamp(log-std))."""
    lat = {k: v.double().cpu() for k, v in lat.items()}
    n = {k: torch.as_tensor(v).double().cpu() for k, v in noise.items()}

    def sd(ls):
        return 2 * torch.sigmoid(ls.clamp(-10, 10))
    box, dep = lat["box_lat"], lat["depth_lat"]
    return dict(z_box=box[:, :4] + sd(box[:, 4:]) * n["eps_box"], ls_box=box[:, 4:], ls_enc=lat["enc_out"][:, A:],
                dl=dep[:, 0:1] + sd(dep[:, 1:2]) * n["eps_depth"], ls_depth=dep[:, 1:2], logit=lat["pres_logit"])


def off(v, delta=DELTA):
    return v.abs() > 10 + delta


def opn(v, delta=DELTA):
    return v.abs() < 10 - delta


def band_share(ci, delta=DELTA, keys=None):
    tot = bad = 0
    for k, v in ci.items():
        if keys is None or k in keys:
            tot += v.numel()
            bad += int((~off(v, delta) & ~opn(v, delta)).sum())
    return bad / tot


def zero_mask_report(grads, ci, mode, delta=DELTA):
    """The structural zeros of a backward whose per-cell latent gradients are ``grads`` (name -> [B, ch, G, G]) given its clamp inputs ``ci``.
    mode 'loss': the whole loss backpropagated; 'z_where' / 'recon': that output term alone (no KL reaches the latents).
    Returns (failures, counts): failures is a list of strings (empty = every assertion holds, on enough elements), counts maps an
    assertion's name to (gated-off elements, open elements)."""
    g = {k: v.double().cpu() for k, v in grads.items()}
    G = ci["logit"].shape[-1]
    c2 = torch.from_numpy(cell_class(G) == 2)[None, None]
    o, f = (lambda v: opn(v, delta)), (lambda v: off(v, delta))
    box, dep, pres = g["box_lat"], g["depth_lat"], g["pres_logit"]
    checks = []          # (name, gradient, must be exactly 0, must be non-zero, the open side must be populated)
    if mode == "loss":
        # d log-std = g_sd * 2 s (1 - s) * in10(log-std), g_sd carrying the KL's sd / ps^2 - 1 / sd: non-zero wherever the gate is open
        checks += [("box log-std", box[:, 4:], f(ci["ls_box"]), o(ci["ls_box"]), True),
                   ("encoder log-std", g["enc_out"][:, A:], f(ci["ls_enc"]), o(ci["ls_enc"]), True),
                   # (L-std moves the one depth log-std bias by +12: no open element there; N-eps alone has them all open)
                   ("depth log-std", dep[:, 1:2], f(ci["ls_depth"]), o(ci["ls_depth"]), False),
                   ("presence logit", pres, f(ci["logit"]), o(ci["logit"]), True)]
    else:
        # no KL: the box mean's gradient is g_z = gq s (1 - s) in10(z), the log-std's g_z eps 2 sl (1 - sl) in10(log-std).  Non-zero is
        # asserted on class-2 cells only (a class-1 box is 2e-3 pixels wide: the renderer may not touch it at all)
        zo = o(ci["z_box"]) & c2
        checks += [("box mean", box[:, :4], f(ci["z_box"]), zo, True),
                   ("box log-std", box[:, 4:], f(ci["z_box"]) | f(ci["ls_box"]), zo & o(ci["ls_box"]), True)]
        if mode == "recon":
            d_off, d_open = f(ci["dl"]), o(ci["dl"]) & c2
            checks += [("depth latents", dep, d_off.expand_as(dep), torch.cat([d_open, d_open & o(ci["ls_depth"])], 1), True),
                       ("presence logit", pres, f(ci["logit"]), o(ci["logit"]) & c2, True)]
        else:       # (under the z_where term a cell's presence matters only to the cells after it: the last has no gradient at all)
            checks += [("presence logit", pres, f(ci["logit"]), torch.zeros_like(f(ci["logit"])), False)]
    failures, counts = [], {}
    share = band_share(ci, delta)
    if share > MAX_BAND_SHARE:
        failures.append("%.1f %% of the clamp inputs lie within %g of +-10" % (100 * share, delta))
    for name, grad, zero, nonzero, need_open in checks:
        n0, n1 = int(zero.sum()), int(nonzero.sum())
        counts[name] = (n0, n1)
        if n0 < MIN_COUNT or (need_open and n1 < MIN_COUNT):
            failures.append("%s (%s): only %d gated-off and %d open elements" % (name, mode, n0, n1))
        bad0, bad1 = int((grad[zero] != 0).sum()), int((grad[nonzero] == 0).sum())
        if bad0:
            failures.append("%s (%s): %d of %d gated-off elements are not exactly 0 (largest %.3g)" % (name, mode, bad0, n0, float(grad[zero].abs().max())))
        if bad1:
            failures.append("%s (%s): %d of %d open elements are 0" % (name, mode, bad1, n1))
        if not bool(torch.isfinite(grad).all()):
            failures.append("%s (%s): non-finite gradient" % (name, mode))
    return failures, counts


def cell_errors(got, ref, cell_tol, floor_tol):
    """(worst cell's error as a fraction of cell_tol * its norm + floor_tol * the largest cell's norm, whole-map relative error)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    err, rn = (got - ref).norm(dim=1), ref.norm(dim=1)
    return float((err / (cell_tol * rn + floor_tol * rn.max())).max()), float((got - ref).norm() / ref.norm())


@functools.lru_cache(maxsize=None)
def bf16_operand_spread(regimes):
    """How far the reference itself moves when its operands are rounded as the bf16 step rounds them (float64 oracle on bf16 operands against
    the float64 oracle, see oracle_run): {"loss": relative difference, (target, name): (worst cell in units of the bf16 cell bound, whole-map
    relative difference)}.  The reference's own spread under bf16 operands, measured on the reference alone."""
    a, b = oracle_run(regimes, "f64", TARGETS), oracle_run(regimes, "f64", TARGETS, bf16_operands=True)
    cell_tol, floor_tol, _, _ = BF16_BOUNDS
    out = {"loss": abs(a["loss"] - b["loss"]) / abs(a["loss"])}
    for t in TARGETS:
        for n in NAMES:
            out[t, n] = cell_errors(b["grads"][t][n], a["grads"][t][n], (2 if n == "enc_out" else 1) * cell_tol, floor_tol)
    return out


SPREAD_MARGIN = 4.0
# The bf16 step holds every undirected bf16 bound in these regimes except the ones below (test_latent_edges_gpu.py's docstring has its
# figures).  For those alone the bound is SPREAD_MARGIN x the reference's own spread under bf16 operands, stated here: regime -> "loss":
# relative spread, (target, latent): (worst cell in units of the undirected cell bound or None, whole-map relative spread or None); None =
# that bound is held and stays.  test_latent_edges_cpu.py re-measures every figure: it must not exceed the one stated, nor lie below 2/3 of it.
BF16_WIDENED = {
    ALL: {"loss": 1.6e-3,
          ("loss", "depth_lat"): (2.1, 4.0e-2), ("loss", "pres_logit"): (None, 4.1e-2),
          ("z_where", "pres_logit"): (1.1, 3.6e-2),
          ("recon", "depth_lat"): (1.3, None), ("recon", "pres_logit"): (None, 4.2e-2),
          ("z_pres", "box_lat"): (5.1, 6.6e-2), ("z_pres", "depth_lat"): (None, 4.9e-2)},
    ("N-eps",): {("z_pres", "box_lat"): (1.3, 5.7e-2), ("z_pres", "depth_lat"): (3.3, 4.5e-2)},
}


def bf16_bounds(regimes, target, name):
    """(worst-cell limit in units of the undirected cell bound, whole-map limit) of the bf16 step for d target / d name."""
    k = 2 if name == "enc_out" else 1
    sw, sm = BF16_WIDENED[regimes].get((target, name), (None, None))
    return (1.0 if sw is None else SPREAD_MARGIN * sw), (k * BF16_BOUNDS[2] if sm is None else SPREAD_MARGIN * sm)


def bf16_loss_bound(regimes):
    s_ = BF16_WIDENED[regimes].get("loss")
    return BF16_BOUNDS[3] if s_ is None else SPREAD_MARGIN * s_


def missing_clamp_effect(I):
    """What a missing clamp on a saturated logit moves, from the config constants: 1 - sigmoid(10) of the range of cell_y / cell_x, in
    z_where's (xt, yt) units, and of the depth's 4."""
    from spair_pytorch_amd import config as cfg
    t = 1.0 - 1.0 / (1.0 + np.exp(-10.0))
    cell_px = int(np.prod(S2))
    return {"z_where": (cfg.MAX_YX - cfg.MIN_YX) * t * cell_px / I, "z_depth": 4.0 * t}
