"""Differentiable recon / z_where / z_pres outputs (SPAIR(..., differentiable_outputs=True); SpairStepIO.inv_den and grad_*,
csrc/outgrad.hip) against the oracle's autograd, which returns the three as live tensors of the same graph (models.py:35-131).

A user term  aux = (Wr * recon).sum() + (Ww * z_where).sum() + (Wp * z_pres).sum()  with fixed non-symmetric random weights (a wrong
row -> (b, h, w) mapping shows up) is backpropagated alone, term by term and together with the loss; every parameter gradient must match
the oracle's.  With only the loss reaching backward the switch changes nothing: bit for bit on the bf16 step (no atomics); the fp32 step
sums a few reductions with float atomics (split-K GEMMs, the edge element), so there it agrees to that rounding.

The fixtures' weights are used as they are except where a decoder ReLU of some object sits within rounding of zero (11 x 11 fixture:
one pre-activation of 7e-8): which side it lands on is an accident of summation order -- the oracle on two CPUs disagrees -- and a
user term on recon weighs every pixel, so the flipped unit shows.  Such a unit's bias is moved by a few 1e-3 in the weights BOTH sides
use (`untie_decoder`); nothing else changes."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from helpers import case_noise, case_weights, load_case, oracle_cfg
from oracle import spair_oracle as orc
from test_engine_gpu import BF16_BOUNDS

pytestmark = pytest.mark.gpu

FP32_CASES = ["c2_b2_step1001", "ref_default_b2_step1001", "rgb_c1_b4_step1001", "lb2_c1_b4_step1001"]
TARGETS = ["aux", "recon", "z_where", "z_pres", "loss+aux"]


@pytest.fixture
def spair_cfg():
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd import models
    old = list(cfg.INPUT_IMAGE_SHAPE), cfg.N_LOOKBACK, models.STEP_FLAGS
    yield cfg
    cfg.INPUT_IMAGE_SHAPE[:] = old[0]
    cfg.N_LOOKBACK = old[1]
    models.STEP_FLAGS = old[2]


def build(case, dtype, cfg, differentiable=True, weights=None):
    from spair_pytorch_amd.models import SPAIR
    C = case.get("in_chan", 1)
    cfg.set_grid(case["I"], case["strides"])
    cfg.INPUT_IMAGE_SHAPE[0] = C
    cfg.N_LOOKBACK = case.get("lookback", 1)
    m = SPAIR([C, case["I"], case["I"]], None, torch.device("cuda"), compute_dtype=dtype, differentiable_outputs=differentiable).to("cuda")
    m.load_state_dict(weights if weights is not None else case_weights(case))
    return m


def untie_decoder(w, x, step, noise, ocfg, margin=1e-4):
    """Move every MLP-decoder hidden unit whose pre-activation is within `margin` of zero for some object off the ReLU's kink, by shifting
    that unit's bias (in place, both layers in order).  z_attr does not depend on the decoder, so one oracle forward gives the inputs."""
    import torch.nn.functional as F
    with torch.no_grad():
        za = orc.forward(w, x, step, noise, ocfg)["z_attr"]
        h = za.permute(0, 2, 3, 1).reshape(-1, za.shape[1]).double()
        for layer in ("dense0", "dense1"):
            wt, b = w["object_decoder.%s.weight" % layer], w["object_decoder.%s.bias" % layer]
            pre = F.linear(h, wt.double(), b.double())
            for j in torch.nonzero((pre.abs() < margin).any(0)).flatten().tolist():
                for delta in (2e-3, -2e-3, 5e-3, -5e-3, 1e-2, -1e-2):
                    if ((pre[:, j] + delta).abs() >= margin).all():
                        b[j] += delta
                        break
                else:
                    raise AssertionError("no bias shift clears the ReLU tie of %s unit %d" % (layer, j))
            h = torch.relu(F.linear(h, wt.double(), b.double()))
    return w


def prepared(case, z):
    """(weights without decoder ReLU ties, oracle leaf copies of them, x, noise, user-term weights)."""
    x, noise, W = _inputs(z, case)
    w = untie_decoder(case_weights(case), x, int(z["global_step"]), noise, oracle_cfg(case))
    p = {k: v.clone().requires_grad_(not k.startswith("attn.")) for k, v in w.items()}
    return w, p, x, noise, W


def aux_weights(recon_shape, zw_shape, zp_shape, seed=7):
    g = torch.Generator().manual_seed(seed)
    return {"recon": torch.randn(recon_shape, generator=g), "z_where": torch.randn(zw_shape, generator=g),
            "z_pres": torch.randn(zp_shape, generator=g)}


def objective(target, loss, outs, W):
    """outs / W: dicts recon, z_where, z_pres (W on the outputs' device)."""
    terms = {k: (W[k] * outs[k]).sum() for k in ("recon", "z_where", "z_pres")}
    if target in terms:
        return terms[target]
    aux = terms["recon"] + terms["z_where"] + terms["z_pres"]
    return aux if target == "aux" else loss + aux


def oracle_grads(p, x, step, noise, ocfg, W, targets):
    out = orc.forward(p, x, step, noise, ocfg)
    outs = {"recon": out["recon_x"], "z_where": out["z_where"], "z_pres": out["z_pres"]}
    names = [k for k, v in p.items() if v.requires_grad]
    res = {}
    for t in targets:
        g = torch.autograd.grad(objective(t, out["loss"], outs, W), [p[k] for k in names], retain_graph=True, allow_unused=True)
        res[t] = {k: (torch.zeros_like(p[k]) if gk is None else gk).double() for k, gk in zip(names, g)}
    return res


def engine_grads(m, x, step, noise, W, target):
    m.zero_grad()
    loss, recon, z_where, z_pres = m(x, step, noise=noise)
    Wd = {k: v.cuda() for k, v in W.items()}
    objective(target, loss, {"recon": recon, "z_where": z_where, "z_pres": z_pres}, Wd).backward()
    return {k: q.grad.detach().double().cpu().clone() for k, q in m.named_parameters() if not k.startswith("attn.")}


def fp32_mismatches(got, ref):
    bad = []
    for k, r in ref.items():
        g = got[k]
        gn, rn = g.norm().item(), r.norm().item()
        err = (g - r).abs().max().item()
        if err > 2e-3 * r.abs().max().item() + 1e-6 or abs(gn - rn) > 2e-3 * rn + 1e-6:
            bad.append((k, err, gn, rn))
    return bad


def _inputs(z, case):
    x = torch.from_numpy(z["x"])
    noise = case_noise(z)
    G = z["eps_box"].shape[-1]
    B, C, I = x.shape[0], case.get("in_chan", 1), case["I"]
    return x, noise, aux_weights((B, C, I, I), (B, 4, G, G), (B, 1, G, G))


@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_output_gradients_match_oracle(name, spair_cfg):
    z, case = load_case(name)
    step = int(z["global_step"])
    w, p, x, noise, W = prepared(case, z)
    ref = oracle_grads(p, x, step, noise, oracle_cfg(case), W, TARGETS)
    m = build(case, "f32", spair_cfg, weights=w)
    xd, nd = x.cuda(), {k: v.cuda() for k, v in noise.items()}
    for t in TARGETS:
        got = engine_grads(m, xd, step, nd, W, t)
        assert not fp32_mismatches(got, ref[t]), (t, fp32_mismatches(got, ref[t]))
        # (the comparison is not of zeros: the user term reaches the encoder nets whichever output it is on)
        assert got["box_network.body.dense0.weight"].abs().max().item() > 0, t


def test_fp32_output_gradients_with_conv_object_encoder(spair_cfg):
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import SPAIR
    I, B, step, strides = 48, 3, 1500, (2, 2, 2, 1, 1, 1)
    topo = [(32, 4, 2), (32, 3, 2), (32, 3, 2), (32, 1, 1)]
    spair_cfg.set_grid(I, strides)
    torch.manual_seed(5)
    m = SPAIR([1, I, I], None, torch.device("cuda"), compute_dtype="f32", object_encoder="conv", differentiable_outputs=True).to("cuda")
    G = gi.grid_side(I, strides)
    x = torch.from_numpy(scattered_digits(21, B, I, 4)[0])
    noise = {k: torch.from_numpy(v) for k, v in gi.make_noise(9, B, G).items()}
    W = aux_weights((B, 1, I, I), (B, 4, G, G), (B, 1, G, G))
    p = {k: v.detach().cpu().clone().requires_grad_(not k.startswith("attn.")) for k, v in m.state_dict().items()}
    targets = ["aux", "loss+aux"]
    ref = oracle_grads(p, x, step, noise, orc.OracleConfig(image_shape=(1, I, I), conv_strides=strides, object_conv=topo), W, targets)
    for t in targets:
        got = engine_grads(m, x.cuda(), step, {k: v.cuda() for k, v in noise.items()}, W, t)
        assert not fp32_mismatches(got, ref[t]), (t, fp32_mismatches(got, ref[t]))
        assert got["object_encoder.conv.conv_0.weight"].abs().max().item() > 0, t


@pytest.mark.parametrize("flags", [0, 1], ids=["fused_chain", "per_wavefront"])
def test_bf16_output_gradients_within_case_bounds(flags, spair_cfg):
    from spair_pytorch_amd import models
    name = "c2_b2_step1001"
    _, _, _, tol_norm, min_cos = BF16_BOUNDS[name]
    z, case = load_case(name)
    step = int(z["global_step"])
    w, p, x, noise, W = prepared(case, z)
    ref = oracle_grads(p, x, step, noise, oracle_cfg(case), W, ["loss+aux"])["loss+aux"]
    m = build(case, "bf16", spair_cfg, weights=w)
    models.STEP_FLAGS = flags
    got = engine_grads(m, x.cuda(), step, {k: v.cuda() for k, v in noise.items()}, W, "loss+aux")
    bad = []
    for k, r in ref.items():
        g = got[k].flatten()
        r = r.flatten()
        gn, rn = g.norm().item(), r.norm().item()
        if abs(gn - rn) > tol_norm * rn + 1e-5:
            bad.append((k, "norm", gn / max(rn, 1e-30)))
        if rn > 1e-6:
            cos = float(torch.dot(g, r) / (gn * rn + 1e-30))
            if cos < min_cos:
                bad.append((k, "cos", cos))
    assert not bad, bad


def _step(case, z, dtype, cfg, differentiable):
    m = build(case, dtype, cfg, differentiable)
    x = torch.from_numpy(z["x"]).cuda()
    noise = {k: v.cuda() for k, v in case_noise(z).items()}
    m.zero_grad()
    loss, recon, z_where, z_pres = m(x, int(z["global_step"]), noise=noise)
    return m, loss, recon, z_where, z_pres


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_loss_only_backward_is_bit_identical_with_the_switch_on(dtype, spair_cfg):
    z, case = load_case("c2_b2_step1001")
    res = []
    for diff in (False, True):
        m, loss, recon, z_where, z_pres = _step(case, z, dtype, spair_cfg, diff)
        assert recon.requires_grad == diff and z_where.requires_grad == diff and z_pres.requires_grad == diff
        loss.backward()
        res.append((loss.detach().clone(), recon.detach().clone(), z_where.detach().clone(), z_pres.detach().clone(),
                    m.flat_gradients().clone()))
    names = ["loss", "recon", "z_where", "z_pres", "gradients"]
    for n, a, b in zip(names, *res):
        if dtype == "bf16" or n != "gradients":
            assert torch.equal(a, b), n
        else:    # (float atomics in the fp32 step: two default models differ by as much)
            assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item(), n


def test_retained_graph_backward_twice_doubles_the_gradient(spair_cfg):
    """The recon fold writes a separate scratch buffer: the forward's saved per-pixel state is the same for the second backward (bf16: the
    step without atomics, so the second backward repeats the first to the bit)."""
    z, case = load_case("c2_b2_step1001")
    m, loss, recon, z_where, z_pres = _step(case, z, "bf16", spair_cfg, True)
    W = {k: v.cuda() for k, v in aux_weights(recon.shape, z_where.shape, z_pres.shape).items()}
    obj = objective("loss+aux", loss, {"recon": recon, "z_where": z_where, "z_pres": z_pres}, W)
    obj.backward(retain_graph=True)
    once = m.flat_gradients().clone()
    assert once.abs().max().item() > 0
    obj.backward()
    assert torch.equal(m.flat_gradients(), 2 * once)


def test_outputs_require_grad_only_when_asked(spair_cfg):
    z, case = load_case("c2_b2_step1001")
    _, loss, recon, z_where, z_pres = _step(case, z, "f32", spair_cfg, False)
    assert loss.requires_grad and not (recon.requires_grad or z_where.requires_grad or z_pres.requires_grad)
    m = build(case, "f32", spair_cfg, True)
    with torch.no_grad():
        outs = m(torch.from_numpy(z["x"]).cuda(), int(z["global_step"]), noise={k: v.cuda() for k, v in case_noise(z).items()})
    assert not any(t.requires_grad for t in outs)
    assert np.isfinite(outs[0].item())
