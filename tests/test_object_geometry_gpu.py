"""The training step at the settings every other GPU test leaves at their defaults: align_corners = True (config.py ALIGN_CORNERS) and
object sizes other than 28 px (OBJECT_SHAPE).  There the step runs other kernels -- the renderer's fallback families, the per-wavefront
cell path instead of the fused chain, the fused decoder at 36 / 64 column pairs or the unfused decoder, the colour renderer with ac = 1.
Each case first asserts the plan it claims to cover (spair_step_plan), then compares the step with the CPU oracle on the same weights,
image and noise -- the oracle is pinned to the reference at these object sizes by the p* fixtures (test_oracle_golden.py) and at
align_corners = True by test_explicit_stn_matches_float64_grid_sample -- and, where a fixture exists, with the reference's own numbers.

Bounds: fp32 those of test_fp32_step_matches_reference / test_bench_geometry_under_sharp_count_prior_vs_oracle; bf16 the c1_b8_step1001
row of BF16_BOUNDS (the 48 x 48 fixtures' geometry)."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from helpers import KL_NAMES, case_noise, load_case
from oracle import spair_oracle as orc
from test_engine_gpu import BF16_BOUNDS

pytestmark = pytest.mark.gpu
STRIDES = (2, 2, 2, 1, 1, 1)
TOL_LOSS, TOL_RECON, TOL_ZW, TOL_NORM, MIN_COS = BF16_BOUNDS["c1_b8_step1001"]


def plan(fwd, bwd, s16=False, chain=False, dec_fused=False):
    return dict(fwd=fwd, bwd=bwd, rec=False, s16=s16, g16=s16, chain=chain, dec_fused=dec_fused)


# name -> (dtype, C, P, ac, I, B, global_step, weight seed, expected plan)
CASES = {
    "bf16_p28_ac1": ("bf16", 1, 28, 1, 64, 4, 1500, 31, plan("GEN2", "GEN2", s16=True, chain=True, dec_fused=True)),
    "bf16_p24": ("bf16", 1, 24, 0, 48, 4, 1500, 32, plan("GEN2", "GEN2", s16=True, dec_fused=True)),
    "bf16_p26": ("bf16", 1, 26, 0, 48, 3, 1500, 33, plan("GEN1", "GEN1", s16=True)),
    "bf16_p32": ("bf16", 1, 32, 0, 64, 2, 1500, 34, plan("GEN2", "GEN1", s16=True, dec_fused=True)),
    "f32_p28_ac1": ("f32", 1, 28, 1, 48, 4, 1500, 35, plan("GEN2", "GEN1")),
    "f32_p25": ("f32", 1, 25, 0, 48, 3, 1500, 36, plan("GEN1", "GEN1")),
    "f32_c3_p24_ac1": ("f32", 3, 24, 1, 48, 2, 1500, 37, plan("COLOUR", "COLOUR")),
    "bf16_c3_p24_ac1": ("bf16", 3, 24, 1, 48, 2, 1500, 37, plan("COLOUR", "COLOUR")),
}


@pytest.fixture
def geom_cfg():
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd import models
    old = list(cfg.OBJECT_SHAPE), cfg.ALIGN_CORNERS, list(cfg.INPUT_IMAGE_SHAPE), models.STEP_FLAGS
    yield cfg
    cfg.OBJECT_SHAPE[:], cfg.ALIGN_CORNERS, cfg.INPUT_IMAGE_SHAPE[:], models.STEP_FLAGS = old


def build(cfg, dtype, C, P, ac, I, weights, flags=0, differentiable=False):
    from spair_pytorch_amd import models
    cfg.OBJECT_SHAPE[:] = [P, P]
    cfg.ALIGN_CORNERS = bool(ac)
    cfg.set_grid(I, STRIDES)
    cfg.INPUT_IMAGE_SHAPE[0] = C
    models.STEP_FLAGS = flags
    m = models.SPAIR([C, I, I], None, torch.device("cuda"), compute_dtype=dtype, differentiable_outputs=differentiable).to("cuda")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()})
    return m


def inputs(C, P, I, B, wseed):
    G = gi.grid_side(I, STRIDES)
    w = gi.make_weights(wseed, 1.0, in_chan=C, obj_px=P)
    x = gi.make_image(100 + wseed, B, I, 3, in_chan=C)
    noise = gi.make_noise(200 + wseed, B, G)
    return w, torch.from_numpy(x), {k: torch.from_numpy(v) for k, v in noise.items()}


def oracle(w, x, step, noise, C, P, ac, I):
    p = {k: torch.from_numpy(v).clone().requires_grad_(not k.startswith("attn.")) for k, v in w.items()}
    ocfg = orc.OracleConfig(image_shape=(C, I, I), conv_strides=STRIDES, object_shape=(P, P), align_corners=bool(ac), inverse_mode="closed")
    out = orc.forward(p, x, step, noise, ocfg)
    out["loss"].backward()
    return p, out


def engine_step(m, x, step, noise):
    m.zero_grad()
    loss, recon, z_where, z_pres = m(x.cuda(), step, noise={k: v.cuda() for k, v in noise.items()})
    terms = m.loss_terms().cpu().numpy().copy()
    loss.backward()
    grads = {k: q.grad.detach().double().cpu().clone() for k, q in m.named_parameters() if not k.startswith("attn.")}
    return terms, recon.cpu(), z_where.cpu(), z_pres.cpu(), grads


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def check_against(dtype, terms, recon, z_where, z_pres, grads, ref_terms, ref_recon, ref_zw, ref_zp, ref_grads):
    """ref_terms: [loss, recon, 7 KL terms]; ref_grads: {key: float64 tensor}."""
    bad = []
    if dtype == "f32":
        if abs(terms[0] - ref_terms[0]) > 2e-5 * abs(ref_terms[0]) or abs(terms[1] - ref_terms[1]) > 2e-5 * abs(ref_terms[1]):
            bad.append(("loss", terms[:2], ref_terms[:2]))
        for i, n in enumerate(KL_NAMES):
            if abs(terms[2 + i] - ref_terms[2 + i]) > 1e-4 * abs(ref_terms[2 + i]) + 1e-4:
                bad.append((n, terms[2 + i], ref_terms[2 + i]))
        for k, a, b, tol in (("z_where", z_where, ref_zw, 1e-4), ("z_pres", z_pres, ref_zp, 1e-4), ("recon", recon, ref_recon, 2e-4)):
            if rel(a, b) >= tol:
                bad.append((k, rel(a, b)))
        for k, r in ref_grads.items():
            g = grads[k]
            if (g - r).abs().max().item() > 2e-3 * r.abs().max().item() + 1e-6 or abs(g.norm().item() - r.norm().item()) > 2e-3 * r.norm().item() + 1e-6:
                bad.append((k, (g - r).abs().max().item(), r.abs().max().item()))
    else:
        if abs(terms[0] - ref_terms[0]) > TOL_LOSS * abs(ref_terms[0]):
            bad.append(("loss", terms[0], ref_terms[0]))
        for i, n in enumerate(["recon"] + KL_NAMES):
            if abs(terms[1 + i] - ref_terms[1 + i]) > 1e-3 * abs(ref_terms[1 + i]) + 1e-3:
                bad.append((n, terms[1 + i], ref_terms[1 + i]))
        for k, a, b, tol in (("z_where", z_where, ref_zw, TOL_ZW), ("z_pres", z_pres, ref_zp, TOL_RECON), ("recon", recon, ref_recon, TOL_RECON)):
            err = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
            if err >= tol:
                bad.append((k, err))
        gn = float(np.sqrt(sum((g ** 2).sum().item() for g in grads.values())))
        rn = float(np.sqrt(sum((r ** 2).sum().item() for r in ref_grads.values())))
        if abs(gn - rn) > TOL_NORM * rn:
            bad.append(("grad norm", gn, rn))
        for k, r in ref_grads.items():
            g, r = grads[k].flatten(), r.flatten()
            if r.norm().item() > 1e-6 * max(1.0, rn):
                cos = float(torch.dot(g, r) / (g.norm() * r.norm() + 1e-30))
                if cos < MIN_COS:
                    bad.append((k, "cos", cos))
    return bad


def oracle_refs(out, p):
    terms = [out["loss"].item(), out["terms"]["recon"].item()] + [out["terms"]["kl_" + n].item() for n in KL_NAMES]
    grads = {k: t.grad.double() for k, t in p.items() if not k.startswith("attn.") and t.grad is not None}
    return terms, out["recon_x"].detach(), out["z_where"].detach(), out["z_pres"].detach(), grads


@pytest.mark.parametrize("name", list(CASES))
def test_step_vs_oracle(name, geom_cfg):
    dtype, C, P, ac, I, B, step, wseed, want = CASES[name]
    w, x, noise = inputs(C, P, I, B, wseed)
    m = build(geom_cfg, dtype, C, P, ac, I, w)
    assert m.step_plan(B) == want
    p, out = oracle(w, x, step, noise, C, P, ac, I)
    refs = oracle_refs(out, p)
    got = engine_step(m, x, step, noise)
    bad = check_against(dtype, *got, *refs)
    assert not bad, bad
    assert got[4]["box_network.body.dense0.weight"].abs().max().item() > 0      # past the training wheel: every net is trained


def test_bf16_align_corners_fused_chain_equals_per_wavefront_path(geom_cfg):
    """align_corners = True on the bf16 step: the fused chain's glimpse stage and its backward (the 0.5 (I - 1) clip multiplier) against
    the per-wavefront launches (SpairStep.flags bit 0), as test_fused_chain_equals_per_wavefront_path does at align_corners = False."""
    dtype, C, P, ac, I, B, step, wseed, want = CASES["bf16_p28_ac1"]
    w, x, noise = inputs(C, P, I, B, wseed)
    res = []
    for flags in (0, 1):
        m = build(geom_cfg, dtype, C, P, ac, I, w, flags=flags)
        assert m.step_plan(B) == dict(want, chain=not flags)
        res.append(engine_step(m, x, step, noise))
    (ta, ra, wa, pa, ga), (tb, rb, wb, pb, gb) = res
    for k, a, b in (("z_where", wa, wb), ("z_pres", pa, pb), ("recon", ra, rb)):
        assert (a - b).abs().max().item() <= 2e-3 * max(1.0, b.abs().max().item()), k
    assert abs(ta[0] - tb[0]) <= 2e-4 * abs(tb[0])
    va, vb = torch.cat([g.flatten() for g in ga.values()]), torch.cat([g.flatten() for g in gb.values()])
    assert (va - vb).norm().item() <= 3e-2 * vb.norm().item()


@pytest.mark.parametrize("name", ["f32_p25", "bf16_p26"])
def test_output_gradients_through_first_generation_renderer(name, geom_cfg):
    """differentiable_outputs=True with the first-generation forward renderer, which then stores 1/D per pixel for the recon adjoint:
    a user term on recon, z_where and z_pres plus the loss, against the oracle's autograd."""
    from test_output_grads_gpu import aux_weights, fp32_mismatches, objective, oracle_grads, untie_decoder
    dtype, C, P, ac, I, B, step, wseed, want = CASES[name]
    w, x, noise = inputs(C, P, I, B, wseed)
    ocfg = orc.OracleConfig(image_shape=(C, I, I), conv_strides=STRIDES, object_shape=(P, P), align_corners=bool(ac), inverse_mode="closed")
    wt = untie_decoder({k: torch.from_numpy(v).clone() for k, v in w.items()}, x, step, noise, ocfg)
    p = {k: v.clone().requires_grad_(not k.startswith("attn.")) for k, v in wt.items()}
    G = gi.grid_side(I, STRIDES)
    W = aux_weights((B, C, I, I), (B, 4, G, G), (B, 1, G, G))
    ref = oracle_grads(p, x, step, noise, ocfg, W, ["loss+aux"])["loss+aux"]
    m = build(geom_cfg, dtype, C, P, ac, I, wt, differentiable=True)
    assert m.step_plan(B) == want
    m.zero_grad()
    loss, recon, z_where, z_pres = m(x.cuda(), step, noise={k: v.cuda() for k, v in noise.items()})
    objective("loss+aux", loss, {"recon": recon, "z_where": z_where, "z_pres": z_pres}, {k: v.cuda() for k, v in W.items()}).backward()
    got = {k: q.grad.detach().double().cpu() for k, q in m.named_parameters() if not k.startswith("attn.")}
    if dtype == "f32":
        assert not fp32_mismatches(got, ref), fp32_mismatches(got, ref)
    else:
        bad = []
        for k, r in ref.items():
            g, r = got[k].flatten(), r.flatten()
            gn, rn = g.norm().item(), r.norm().item()
            if abs(gn - rn) > TOL_NORM * rn + 1e-5:
                bad.append((k, "norm", gn / max(rn, 1e-30)))
            if rn > 1e-6 and float(torch.dot(g, r) / (gn * rn + 1e-30)) < MIN_COS:
                bad.append((k, "cos"))
        assert not bad, bad


# ---- the reference's own numbers at other object sizes (tests/golden/p*.npz) ------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(gi.OBJ_CASES))
def test_step_vs_reference_fixture(name, dtype, geom_cfg):
    z, case = load_case(name)
    P, I, B = case["obj_px"], case["I"], case["B"]
    w = gi.make_weights(case["wseed"], case["wscale"], obj_px=P)
    m = build(geom_cfg, dtype, 1, P, 0, I, w)
    fwd, bwd = {("f32", 24): ("GEN2", "GEN1"), ("f32", 32): ("GEN2", "GEN1"), ("bf16", 24): ("GEN2", "GEN2"), ("bf16", 32): ("GEN2", "GEN1")}[dtype, P]
    assert m.step_plan(B) == plan(fwd, bwd, s16=dtype == "bf16", dec_fused=dtype == "bf16")
    terms, recon, z_where, z_pres, grads = engine_step(m, torch.from_numpy(z["x"]), int(z["global_step"]), case_noise(z))
    ref_terms = [float(z["loss"]), float(z["recon_loss"])] + [float(z["kl_" + n]) for n in KL_NAMES]
    bad = []
    if dtype == "f32":
        bad = check_against("f32", terms, recon, z_where, z_pres, {}, ref_terms, z["recon_x"], z["z_where"], z["z_pres"], {})
    else:
        bad = check_against("bf16", terms, recon, z_where, z_pres, {}, ref_terms, z["recon_x"], z["z_where"], z["z_pres"], {})
    # gradients: the fixture's per-tensor norm, and the full tensor or its fixed sample of elements
    for k, g in grads.items():
        ref_n = float(z["gradnorm_" + k])
        gv = g.flatten().numpy()
        if "grad_" + k in z.files:
            ref = z["grad_" + k].astype(np.float64).flatten()
        else:
            gv, ref = gv[z["gradidx_" + k]], z["gradsample_" + k].astype(np.float64)
        if dtype == "f32":
            if abs(np.linalg.norm(g.numpy()) - ref_n) > 2e-3 * ref_n + 1e-6 or np.abs(gv - ref).max() > 2e-3 * np.abs(ref).max() + 1e-6:
                bad.append((k, np.linalg.norm(g.numpy()), ref_n))
        else:
            if abs(np.linalg.norm(g.numpy()) - ref_n) > TOL_NORM * ref_n + 1e-5:
                bad.append((k, "norm", np.linalg.norm(g.numpy()) / max(ref_n, 1e-30)))
            if np.linalg.norm(ref) > 1e-6 * max(1.0, ref_n):
                cos = float(np.dot(gv, ref) / (np.linalg.norm(gv) * np.linalg.norm(ref) + 1e-30))
                if cos < MIN_COS:
                    bad.append((k, "cos", cos))
    assert not bad, bad
