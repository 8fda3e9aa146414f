#!/usr/bin/env python3
"""Golden vectors of SPAIR.compose (a scene rendered from GIVEN latents, with object layers), produced by the reference in THIS container.

The reference is run exactly as make_golden.py / make_golden_rect.py run it (their own ``run_case``, ``numpy.savez_compressed`` muted so no
existing fixture is touched) and its model is KEPT: ``SPAIR._render`` is wrapped to remember ``self`` and the image it was called with.
Then the reference's own ``_render`` (models.py:452-542, a pure function of z_attr / z_where / z_depth / z_pres) is called once more on
EDITED latents -- the rule is ``compose_helpers.edit_latents``, deterministic from the case's base fixture and its parse fixture -- while
the name ``stn`` in ``spair.models`` is wrapped by a spy that keeps the ``inverse=True`` call's return value: the warped
``[B*HW, C+2, I, Iw]`` channels (colour.., alpha * pres, importance).  From that tensor, in float64 (models.py:524-537):

    imp = channel C+1 + 1e-9,  layer_weight_k = alpha_k * imp_k / sum_all imp,  layers_k = layer_weight_k * colour_k

``compose_<case>.npz`` holds the edited latents (z_where, z_what, z_depth, z_pres), ``recon`` (the reference's output), ``cells`` int32
[B,8] (the six largest-area cells, one edited cell, one -1) and ``layers`` [B,8,C,rows,Iw] / ``layer_weight`` [B,8,rows,Iw] as fp32 (zeros
for the -1).  A file above 1 MB keeps the top half of its canvas rows (again until it fits) in recon, layers and layer_weight.

Usage:  python tests/golden/make_golden_compose.py            # all cases (one subprocess each)
        python tests/golden/make_golden_compose.py --case c2_b2_step1001
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
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_rect as mgr  # noqa: E402
import compose_helpers as ch  # noqa: E402

CASES = ch.CASES
MAX_BYTES = 1000000


def run_case(name):
    import torch
    heard = {}
    real_import = mg._import_reference

    def import_and_listen(*a, **k):
        cfg, models, modules, writer = real_import(*a, **k)
        real_stn, real_render = models.stn, models.SPAIR._render

        def stn_spy(*sa, **sk):
            out = real_stn(*sa, **sk)
            if sk.get("inverse"):
                heard["warp"] = out.detach().clone()
            return out

        def render_spy(self, z_attr, z_where, z_depth, z_pres, x):
            heard["model"], heard["x"] = self, x
            return real_render(self, z_attr, z_where, z_depth, z_pres, x)

        models.stn, models.SPAIR._render = stn_spy, render_spy
        heard["cfg"] = cfg
        return cfg, models, modules, writer

    mg._import_reference = import_and_listen
    real_save = np.savez_compressed
    np.savez_compressed = lambda *a, **k: None
    try:
        (mgr if name in mgr.CASES else mg).run_case(name)
    finally:
        np.savez_compressed = real_save
        mg._import_reference = real_import
    C, I, Iw = (int(v) for v in heard["cfg"].INPUT_IMAGE_SHAPE)
    base = np.load(os.path.join(HERE, name + ".npz"))
    parse = np.load(os.path.join(HERE, "parse_" + name + ".npz"))
    zw, zt, zd, zp, cells = ch.edit_latents(base["z_where"], base["z_attr"], base["z_depth"], base["z_pres"], parse["owner"])
    m = heard["model"]
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        # (unedited first: the kept model must reproduce the base fixture's own recon from its stored latents)
        again = m._render(*(torch.from_numpy(base[k]) for k in ("z_attr", "z_where", "z_depth", "z_pres")), heard["x"]).numpy()
        recon = m._render(torch.from_numpy(zt), torch.from_numpy(zw), torch.from_numpy(zd), torch.from_numpy(zp), heard["x"]).numpy()
    assert np.abs(again - base["recon_x"]).max() < 2e-5, np.abs(again - base["recon_x"]).max()
    B = zw.shape[0]
    t = heard["warp"].numpy().astype(np.float64)
    assert t.shape[1:] == (C + 2, I, Iw) and t.shape[0] % B == 0, t.shape
    HW = t.shape[0] // B
    t = t.reshape(B, HW, C + 2, I, Iw)
    imp = t[:, :, C + 1] + 1e-9
    w = t[:, :, C] * imp / imp.sum(axis=1, keepdims=True)
    assert np.abs(np.clip((w[:, :, None] * t[:, :, :C]).sum(axis=1), 0, 1) - recon).max() < 1e-5
    ok = cells >= 0
    kk = np.where(ok, cells, 0)
    bi = np.arange(B)[:, None]
    lw = w[bi, kk] * ok[:, :, None, None]
    lay = lw[:, :, None] * t[bi, kk][:, :, :C]
    out = dict(z_where=zw, z_what=zt, z_depth=zd, z_pres=zp, cells=cells, recon=recon.astype(np.float32), layers=lay.astype(np.float32),
               layer_weight=lw.astype(np.float32))
    path = os.path.join(HERE, "compose_" + name + ".npz")
    rows = I
    np.savez_compressed(path, **out)
    while os.path.getsize(path) > MAX_BYTES:
        rows //= 2
        out.update(recon=out["recon"][:, :, :rows], layers=out["layers"][:, :, :, :rows], layer_weight=out["layer_weight"][:, :, :rows])
        np.savez_compressed(path, **out)
    print(f"compose_{name}: {HW} cells, canvas rows kept {rows} of {I}, edit moves recon by {np.abs(recon - base['recon_x']).max():.3f}, "
          f"layers hold {float(lw.sum(axis=1).mean() / max(w.sum(axis=1).mean(), 1e-30)):.3f} of the coverage "
          f"-> {os.path.getsize(path) / 1e6:.2f} MB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        run_case(a.case)
        return
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for name in CASES:      # one process per case: the reference's config is module-level state
        subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], check=True, env=env)


if __name__ == "__main__":
    main()
