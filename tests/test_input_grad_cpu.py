"""The gradient of the step with respect to its input image, host side (no GPU).

* The oracle's autograd ``x.grad`` reproduces the reference's (tests/golden/xgrad_<case>.npz, make_golden_input_grad.py): after
  loss.backward(), inf pattern included (torch's BCE target gradient -logit(recon) is not clamped), and after a term on z_where / z_pres
  alone (the network path).  This pins the yardstick test_input_grad_gpu.py holds the engine to.
* The backward takes the image gradient's buffers in SpairStepIO (grad_x, x_scratch, bce_target); the built library exports it and the
  host-only scratch query, which returns [B,C,I,I] fp32 rounded to 256 bytes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, case_noise, case_weights, load_case, oracle_cfg
from oracle import spair_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["c2_b2_step1001", "ref_default_b2_step1001", "c1_b8_step7001", "c4_b1_step1001", "rgb_c1_b4_step1001", "lb2_c1_b4_step1001",
         "p24_c1_b4_step1001"]


def load_xgrad(name):
    return np.load(os.path.join(GOLDEN, "xgrad_" + name + ".npz"))


def oracle_xgrads(name, z, case, ref):
    """(x.grad after loss.backward(), x.grad after the network-path term alone, recon) of the oracle, fp32."""
    x = torch.from_numpy(z["x"]).clone().requires_grad_()
    out = orc.forward(case_weights(case, requires_grad=True), x, int(z["global_step"]), case_noise(z), oracle_cfg(case))
    (g_loss,) = torch.autograd.grad(out["loss"], [x], retain_graph=True)
    term = (torch.from_numpy(ref["wz"]) * out["z_where"]).sum() + (torch.from_numpy(ref["wp"]) * out["z_pres"]).sum()
    (g_net,) = torch.autograd.grad(term, [x])
    return g_loss.numpy(), g_net.numpy(), out["recon_x"].detach().numpy()


def assert_close(got, ref, what, rel=2e-3):
    scale = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref).max()
    assert err <= rel * scale + 1e-9, "%s: max err %.3e vs max|ref| %.3e" % (what, err, scale)
    gn, rn = np.linalg.norm(got.astype(np.float64)), np.linalg.norm(ref.astype(np.float64))
    assert abs(gn - rn) <= rel * rn + 1e-9, "%s: norm %.6e vs %.6e" % (what, gn, rn)


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference_input_gradient(name):
    z, case = load_case(name)
    ref = load_xgrad(name)
    g_loss, g_net, recon = oracle_xgrads(name, z, case, ref)
    # the network path alone
    assert_close(g_net, ref["xgrad_net"], name + " network path")
    # after loss.backward(): inf exactly where the reference's recon is 0 (-inf where it is 1), the rest as the network + BCE terms
    r_inf = np.isinf(ref["xgrad_loss"])
    assert np.array_equal(r_inf, ref["recon_x"] == 0) or np.array_equal(r_inf, (ref["recon_x"] == 0) | (ref["recon_x"] == 1))
    assert np.array_equal(np.isinf(g_loss), r_inf), "%s: inf pattern differs (%d vs %d)" % (name, np.isinf(g_loss).sum(), r_inf.sum())
    assert np.array_equal(np.sign(g_loss[r_inf]), np.sign(ref["xgrad_loss"][r_inf]))
    assert not np.isnan(g_loss).any()
    fin = ~r_inf
    assert_close(g_loss[fin], ref["xgrad_loss"][fin], name + " loss")


def test_reference_default_fixture_has_the_documented_infinities():
    ref = load_xgrad("ref_default_b2_step1001")
    assert int(np.isinf(ref["xgrad_loss"]).sum()) == 409 and ref["xgrad_loss"].size == 32768
    assert (ref["xgrad_loss"][np.isinf(ref["xgrad_loss"])] > 0).all()


def test_bce_target_gradient_is_unclamped_neg_logit():
    r = torch.tensor([0.0, 1.0, 1e-45, 0.25, 0.5], dtype=torch.float32)
    t = torch.full_like(r, 0.5).requires_grad_()
    torch.nn.functional.binary_cross_entropy(r, t, reduction="sum").backward()
    g = t.grad.numpy()
    assert g[0] == np.inf and g[1] == -np.inf and abs(g[2] - 103.28) < 1e-2
    np.testing.assert_allclose(g[3:], (torch.log1p(-r[3:]) - torch.log(r[3:])).numpy(), rtol=1e-6)


def _lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def test_input_gradient_io_fields_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "spair_hip.h")).read()
    for name in ("spair_backward", "spair_input_grad_scratch_bytes", "spair_input_grad_glimpse", "spair_input_grad_stem"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(_lib(), name), name
    io = re.search(r"typedef struct SpairStepIO \{(.*?)\} SpairStepIO;", hdr, re.S).group(1)
    for field in ("grad_x", "x_scratch", "bce_target"):
        assert re.search(r"\b%s;" % field, io), field
    gone = "spair_backward" + "_x"       # the suffixed entry point SpairStepIO replaced (spelled in parts: nothing else names it)
    assert not re.search(r"\b%s\b" % gone, hdr) and not hasattr(_lib(), gone)


@pytest.mark.parametrize("B,C,I,strides", [(256, 1, 128, (3, 2, 2, 1, 1, 1)), (3, 3, 48, (2, 2, 2, 1, 1, 1))])
def test_scratch_query_size(B, C, I, strides):
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.models import make_dims
    from spair_pytorch_amd.modules import Backbone
    old = list(cfg.INPUT_IMAGE_SHAPE), [layer['stride'] for layer in cfg.DEFAULT_BACKBONE_TOPOLOGY]
    try:
        cfg.set_grid(I, strides)
        cfg.INPUT_IMAGE_SHAPE[0] = C
        topo = Backbone([C, I, I], cfg.N_BACKBONE_FEATURES).topology
        d = make_dims(B, [C, I, I], topo, "bf16")
    finally:
        cfg.INPUT_IMAGE_SHAPE[:] = old[0]
        for layer, st in zip(cfg.DEFAULT_BACKBONE_TOPOLOGY, old[1]):
            layer['stride'] = st
    lib = _lib()
    lib.spair_input_grad_scratch_bytes.restype = ctypes.c_int64
    lib.spair_workspace_bytes.restype = ctypes.c_int64
    assert lib.spair_workspace_bytes(ctypes.byref(d)) > 0
    assert lib.spair_input_grad_scratch_bytes(ctypes.byref(d)) == (B * C * I * I * 4 + 255) // 256 * 256
    bad = make_dims(B, [C, I, I], topo, "bf16")
    bad.B = 0
    assert lib.spair_input_grad_scratch_bytes(ctypes.byref(bad)) == -1
