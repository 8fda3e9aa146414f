#!/usr/bin/env python3
"""Golden image gradients: the reference's ``x.grad`` for the cases of make_golden.py (same weights, image and injected noise).

Each ``xgrad_<case>.npz`` holds
  xgrad_loss  x.grad after loss.backward()            (inf wherever recon_x is exactly 0: torch's BCE target gradient -logit(recon))
  xgrad_net   x.grad after term.backward() alone      (term = sum(wz * z_where) + sum(wp * z_pres): the network path, no BCE term)
  wz, wp      the term's fixed non-symmetric weights
  recon_x     the reference's reconstruction
Runs only in the build container, like make_golden.py; the tests read the .npz files.

Usage:  python tests/golden/make_golden_input_grad.py            # all cases (one subprocess each)
        python tests/golden/make_golden_input_grad.py --case c2_b2_step1001
"""
import argparse
import contextlib
import io
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import golden_inputs as gi  # noqa: E402
import make_golden as mg  # noqa: E402

CASES = ["c2_b2_step1001", "ref_default_b2_step1001", "c1_b8_step7001", "c4_b1_step1001", "rgb_c1_b4_step1001",
         "lb2_c1_b4_step1001", "p24_c1_b4_step1001"]


def term_weights(B, G, seed=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, 4, G, G)).astype(np.float32), rng.standard_normal((B, 1, G, G)).astype(np.float32)


@contextlib.contextmanager
def injected_noise(noise, B, G):
    """The 7 per-cell draws in the reference's order (models.py:333-336,84,95,402-403), as make_golden.run_case injects them."""
    import torch
    import torch.distributions.normal as tdn
    state = dict(cell=0, k=0)

    def fake_standard_normal(shape, dtype, device):
        h, w_ = divmod(state["cell"], G)
        k = state["k"]
        if k < 4:
            out = noise["eps_box"][:, k:k + 1, h, w_]
        elif k == 4:
            out = noise["eps_attr"][:, :, h, w_]
        elif k == 5:
            out = noise["eps_depth"][:, :, h, w_]
        else:
            raise AssertionError("unexpected normal draw")
        state["k"] += 1
        return torch.from_numpy(np.ascontiguousarray(out))

    def fake_rand(*shape, **kw):
        assert state["k"] == 6, state
        h, w_ = divmod(state["cell"], G)
        state["k"] = 0
        state["cell"] += 1
        return torch.from_numpy(np.ascontiguousarray(noise["u_pres"][:, :, h, w_]))

    real_sn, real_rand = tdn._standard_normal, torch.rand
    tdn._standard_normal, torch.rand = fake_standard_normal, fake_rand
    try:
        yield state
    finally:
        tdn._standard_normal, torch.rand = real_sn, real_rand
    assert state["cell"] == G * G


def run_case(name):
    import torch
    case = gi.all_cases()[name]
    in_chan = case.get("in_chan", 1)
    I, strides, B, step = case["I"], case["strides"], case["B"], case["step"]
    G = gi.grid_side(I, strides)
    obj_px = case.get("obj_px", gi.OBJ_PX)
    cfg, models, modules, SummaryWriter = mg._import_reference(I, strides, B, G, case.get("lookback", 1), in_chan, obj_px)
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        m = models.SPAIR(cfg.INPUT_IMAGE_SHAPE, SummaryWriter(), torch.device("cpu"))
    w = gi.make_weights(case["wseed"], case["wscale"], in_chan=in_chan, lookback=case.get("lookback", 1), obj_px=obj_px)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    x = gi.make_image(100 + case["wseed"], B, I, case["max_objects"], in_chan=in_chan)
    noise = gi.make_noise(200 + case["wseed"], B, G)
    wz, wp = term_weights(B, G)
    xt = torch.from_numpy(x).requires_grad_()
    with injected_noise(noise, B, G), contextlib.redirect_stdout(io.StringIO()):
        loss, recon, z_where, z_pres = m(xt, step)
    loss.backward(retain_graph=True)
    xg_loss = xt.grad.detach().numpy().copy()
    xt.grad = None
    ((torch.from_numpy(wz) * z_where).sum() + (torch.from_numpy(wp) * z_pres).sum()).backward()
    out = dict(xgrad_loss=xg_loss, xgrad_net=xt.grad.detach().numpy().copy(), wz=wz, wp=wp, recon_x=recon.detach().numpy(),
               loss=np.float32(loss.item()))
    path = os.path.join(HERE, "xgrad_" + name + ".npz")
    np.savez_compressed(path, **out)
    print(f"xgrad_{name}: inf={int(np.isinf(xg_loss).sum())} zero-recon={int((out['recon_x'] == 0).sum())}"
          f" max|net|={np.abs(out['xgrad_net']).max():.3e} -> {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        run_case(a.case)
    else:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        for nm in CASES:
            subprocess.check_call([sys.executable, __file__, "--case", nm], env=env)
