"""Shared helpers for the parity tests: load golden vectors, build oracle inputs, build the engine's model for a case and hold its fp32
step to a fixture (the GPU helpers import the engine only when called)."""
import contextlib
import functools
import os

import numpy as np
import torch

import golden_inputs as gi
from oracle import spair_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, gi.all_cases()[name]


def oracle_cfg(case, **kw):
    """The oracle's configuration of a case: image, object size, lookback, and the backbone topology and network sizes a case may carry
    (golden_inputs.case_topology / case_net; the filter counts themselves come from the weight shapes)."""
    kw.setdefault("object_shape", (case.get("obj_px", gi.OBJ_PX),) * 2)
    topo, net = gi.case_topology(case), gi.case_net(case)
    return orc.OracleConfig(image_shape=(case.get("in_chan", 1), case["I"], case["I"]), conv_kernels=tuple(k for _, k, _ in topo),
                            conv_strides=tuple(s for _, _, s in topo), n_backbone_features=net["n_features"],
                            n_passthrough=net["n_passthrough"], n_attr=net["n_attr"], n_lookback=case.get("lookback", 1), **kw)


def case_weights(case, requires_grad=False):
    w = gi.make_weights(case["wseed"], case["wscale"], in_chan=case.get("in_chan", 1), lookback=case.get("lookback", 1),
                        obj_px=case.get("obj_px", gi.OBJ_PX), **gi.case_net(case))
    return {k: torch.from_numpy(v).clone().requires_grad_(requires_grad and not k.startswith("attn."))
            for k, v in w.items()}


def case_noise(z):
    return {k: torch.from_numpy(z[k]) for k in ("eps_box", "eps_attr", "eps_depth", "u_pres")}


KL_NAMES = ["cy_logit", "cx_logit", "height_logit", "width_logit", "attr", "depth_logit", "pres_dist"]


def assert_adam_updates_close(pa, pb, lr, tight=2e-6, outlier_frac=1e-5):
    """Parameters after Adam steps of two runs whose gradients agree to rounding (fp32 atomics in the bias / edge sums): Adam's update
    lr * m / (sqrt(v) + eps) is sign-like, so a gradient that is itself rounding noise (|g| <~ eps) may move its parameter by up to
    +-lr differently in the two runs.  All but a few elements in a million must agree to `tight`, none may differ by more than 2.2 lr."""
    d = np.abs(np.asarray(pa, np.float64) - np.asarray(pb, np.float64))
    assert d.max() <= 2.2 * lr, d.max()
    assert (d > tight).mean() <= outlier_frac, ((d > tight).sum(), d.size)


# ---- the engine on a case (GPU tests) ---------------------------------------------------------------------------------------------------------
def case_engine_topology(case):
    return [dict(filters=f, kernel_size=k, stride=s) for f, k, s in gi.case_topology(case)]


def apply_case_config(case):
    """Point spair_pytorch_amd.config at a case: image side, backbone topology, F / NP / A.  A case without a `topology` only moves the
    strides of the configured layers (config.set_grid), as the tests did before cases could carry one."""
    from spair_pytorch_amd import config as cfg
    if "topology" in case:
        cfg.DEFAULT_BACKBONE_TOPOLOGY[:] = case_engine_topology(case)
        cfg.INPUT_IMAGE_SHAPE[1:] = [int(case["I"])] * 2
    else:
        cfg.set_grid(case["I"], case["strides"])
    net = gi.case_net(case)
    for key, name in (("F", "N_BACKBONE_FEATURES"), ("NP", "N_PASSTHROUGH_FEATURES"), ("A", "N_ATTRIBUTES")):
        if key in case:
            setattr(cfg, name, int(case[key]))
    cfg.N_CONTEXT_DIM = 4 + net["n_attr"] + 1 + 1 if "A" in case else cfg.N_CONTEXT_DIM


@contextlib.contextmanager
def engine_config(case, flags=None):
    """The engine's configuration for `case` (apply_case_config) and, if given, SpairStep.flags, for the duration of the block: topology, F,
    NP, A, image shape and STEP_FLAGS are put back afterwards, whatever happened inside.  The model reads them whenever it sizes a
    workspace, so build AND run inside the block."""
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd import models
    names = ("N_BACKBONE_FEATURES", "N_PASSTHROUGH_FEATURES", "N_ATTRIBUTES", "N_CONTEXT_DIM")
    old = (list(cfg.INPUT_IMAGE_SHAPE), [dict(t) for t in cfg.DEFAULT_BACKBONE_TOPOLOGY], [getattr(cfg, n) for n in names], models.STEP_FLAGS)
    try:
        apply_case_config(case)
        if flags is not None:
            models.STEP_FLAGS = int(flags)
        yield cfg
    finally:
        cfg.INPUT_IMAGE_SHAPE[:] = old[0]
        cfg.DEFAULT_BACKBONE_TOPOLOGY[:] = old[1]
        for n, v in zip(names, old[2]):
            setattr(cfg, n, v)
        models.STEP_FLAGS = old[3]


def build_model(case, dtype):
    """The engine's SPAIR on the GPU with the case's configuration applied and its weights loaded."""
    from spair_pytorch_amd.models import SPAIR
    apply_case_config(case)
    m = SPAIR([case.get("in_chan", 1), case["I"], case["I"]], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
    m.load_state_dict({k: v for k, v in case_weights(case).items()})
    return m


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def assert_fp32_step_matches(m, z, retain_graph=False):
    """One fp32 step of model `m` on the inputs of `z` against the expected values `z` holds (a fixture, or oracle_fixture's dictionary of the
    same keys): loss 2e-5, KL 1e-4, outputs 1e-4 / 2e-4, every gradient's norm and its elements or samples at 2e-3."""
    x = torch.from_numpy(np.asarray(z["x"])).cuda()
    noise = {k: torch.from_numpy(np.asarray(z[k])).cuda() for k in ("eps_box", "eps_attr", "eps_depth", "u_pres")}
    m.zero_grad()
    loss, recon, z_where, z_pres = m(x, int(z["global_step"]), noise=noise)
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
    for i, n in enumerate(KL_NAMES[:6]):
        assert rel(m.dist_param[n]["mean"].cpu().numpy(), z["mean_" + n]) < 1e-4, n
        assert rel(m.dist_param[n]["sigma"].cpu().numpy(), z["sigma_" + n]) < 1e-4, n
    loss.backward(retain_graph=retain_graph)
    bad = []
    for k, p in m.named_parameters():
        if k.startswith("attn."):
            assert p.grad is None
            continue
        g = p.grad.cpu().numpy()
        gn = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        ref_n = float(z["gradnorm_" + k])
        if abs(gn - ref_n) > 2e-3 * ref_n + 1e-6:
            bad.append((k, gn, ref_n))
            continue
        if ("grad_" + k) in z:
            if np.abs(g - z["grad_" + k]).max() > 2e-3 * np.abs(z["grad_" + k]).max() + 1e-6:
                bad.append((k, "elements"))
        else:
            smp = g.reshape(-1)[z["gradidx_" + k]]
            if np.abs(smp - z["gradsample_" + k]).max() > 2e-3 * np.abs(z["gradsample_" + k]).max() + 1e-6:
                bad.append((k, "samples"))
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def oracle_fixture(name):
    """What a fixture would hold for a case of golden_inputs.ORACLE_CASES, from the oracle's fp32 forward and backward on the case's own
    inputs: the same keys, and the same gradient summary (norm of every tensor, the tensor itself up to 4096 elements, else 256 elements at
    indices drawn from default_rng(999) in parameter order), as tests/golden/make_golden.py writes.  Computed once; treat as read-only."""
    case = gi.ORACLE_CASES[name]
    w, x, noise = gi.case_inputs(case)
    p = {k: torch.from_numpy(v).clone().requires_grad_(not k.startswith("attn.")) for k, v in w.items()}
    out = orc.forward(p, torch.from_numpy(x), case["step"], {k: torch.from_numpy(v) for k, v in noise.items()}, oracle_cfg(case))
    out["loss"].backward()
    z = dict(x=x, global_step=np.int64(case["step"]), **noise)
    z["loss"], z["recon_loss"] = np.float32(out["loss"].item()), np.float32(out["terms"]["recon"].item())
    for n in KL_NAMES:
        z["kl_" + n] = np.float32(out["terms"]["kl_" + n].item())
    z["recon_x"] = out["recon_x"].detach().numpy()
    for k in ("z_where", "z_pres", "z_depth", "z_attr"):
        z[k] = out[k].detach().numpy()
    for n, (mu, sg) in out["dist"].items():
        z["mean_" + n], z["sigma_" + n] = mu.detach().numpy(), sg.detach().numpy()
    srng = np.random.default_rng(999)
    for k, t in p.items():
        if t.grad is None:
            z["gradnone_" + k] = np.int8(1)
            continue
        g = t.grad.numpy()
        z["gradnorm_" + k] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        if g.size <= 4096:
            z["grad_" + k] = g
        else:
            idx = srng.choice(g.size, 256, replace=False)
            z["gradidx_" + k], z["gradsample_" + k] = idx.astype(np.int64), g.reshape(-1)[idx]
    return z


def expected_of(name):
    """(expected values, case) of any case: its fixture, or the oracle's stand-in for a case of golden_inputs.ORACLE_CASES."""
    if name in gi.ORACLE_CASES:
        return oracle_fixture(name), gi.ORACLE_CASES[name]
    return load_case(name)
