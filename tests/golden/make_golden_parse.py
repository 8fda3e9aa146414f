#!/usr/bin/env python3
"""Golden vectors of the scene parse (SPAIR.parse: per-pixel owner, its weight, coverage), produced by the reference in THIS container.

The reference is run exactly as make_golden.py / make_golden_rect.py run it (their own ``run_case``: same injected noise, same weights from
golden_inputs) and only LISTENED to: the name ``stn`` in ``spair.models`` is wrapped by a spy that keeps the return value of the
``inverse=True`` call of ``_render`` (models.py:515) -- the warped ``[B*HW, C+2, I, Iw]`` channels (colour.., alpha * pres, importance).
From that tensor, in float64 (models.py:524-537):

    imp = channel C+1 + 1e-9,   w = alpha * imp / sum_k imp        -- the coefficient of object k's colour in the composite

``parse_<case>.npz`` holds
    owner      int16 [B,I,Iw]   arg-max over the cells k = h * Gw + w, the lowest index on an exact tie, -1 where the maximum is 0
    w1, w2     fp32  [B,I,Iw]   the largest and the second-largest weight
    coverage   fp32  [B,I,Iw]   sum_k w

The other modules' ``run_case`` would rewrite their own fixture at the end: ``numpy.savez_compressed`` is replaced by a no-op while they
run, so no existing file is touched.

Usage:  python tests/golden/make_golden_parse.py            # all cases (one subprocess each)
        python tests/golden/make_golden_parse.py --case c2_b2_step1001
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import golden_inputs as gi  # noqa: E402
import make_golden as mg  # noqa: E402
import make_golden_rect as mgr  # noqa: E402

CASES = ("c1_b8_step7001", "c2_b2_step1001", "ref_default_b2_step1001", "c4_b1_step1001", "p24_c1_b4_step1001", "lb2_c1_b4_step1001",
         "rgb_c1_b4_step1001", "rect_h48w80_b4_step1001")
MAX_BYTES = 1000000      # per fixture; a larger one keeps the top half of its canvas (rows 0 .. I/2 - 1)


def run_case(name):
    heard = {}
    real_import = mg._import_reference

    def import_and_listen(*a, **k):
        cfg, models, modules, writer = real_import(*a, **k)
        real_stn = models.stn

        def stn_spy(*sa, **sk):
            out = real_stn(*sa, **sk)
            if sk.get("inverse"):
                heard["warp"] = out.detach().clone()
            return out

        models.stn = stn_spy
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
    case = mgr.CASES[name] if name in mgr.CASES else gi.all_cases()[name]
    B = case["B"]
    t = heard["warp"].numpy().astype(np.float64)
    assert t.shape[1:] == (C + 2, I, Iw) and t.shape[0] % B == 0, t.shape
    HW = t.shape[0] // B
    t = t.reshape(B, HW, C + 2, I, Iw)
    imp = t[:, :, C + 1] + 1e-9
    w = t[:, :, C] * imp / imp.sum(axis=1, keepdims=True)
    del t, imp
    owner = np.argmax(w, axis=1)                      # (the first maximum: the lowest index on an exact tie)
    top2 = -np.partition(-w, 1, axis=1)[:, :2]
    w1, w2 = top2[:, 0], top2[:, 1]
    assert np.array_equal(w1, np.take_along_axis(w, owner[:, None], 1)[:, 0])
    owner = np.where(w1 > 0, owner, -1).astype(np.int16)
    out = dict(owner=owner, w1=w1.astype(np.float32), w2=w2.astype(np.float32), coverage=w.sum(axis=1).astype(np.float32))
    path = os.path.join(HERE, "parse_" + name + ".npz")
    np.savez_compressed(path, **out)
    if os.path.getsize(path) > MAX_BYTES:
        out = {k: v[:, :I // 2] for k, v in out.items()}
        np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_BYTES
    print(f"parse_{name}: {HW} cells, canvas rows kept {out['owner'].shape[1]} of {I}, owned {float((owner >= 0).mean()):.3f}, "
          f"w1 - w2 <= 4e-4 on {float((w1 - w2 <= 4e-4).mean()):.4f} -> {os.path.getsize(path) / 1e6:.2f} MB")


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
