"""The scene parse without a GPU: the oracle's restatement of the renderer reproduces every reference fixture tests/golden/parse_<case>.npz
under the comparison rule (which pins the definition and the fixture generator to each other), the pixel-box formula on a hand example,
and the public names."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import parse_helpers as ph
from oracle import spair_oracle as orc


def oracle_weights(name, inverse_mode="lu"):
    """w [B,HW,I,Iw] (float64) from the oracle's decoder and stn on the latents of the case's fixture, as the reference's _render forms it."""
    fx, z = ph.load_parse(name)
    c = ph.case_of(name)
    cfg = orc.OracleConfig(image_shape=(c["C"], c["H"], c["W"]), conv_strides=c["strides"], n_lookback=c["lookback"],
                           object_shape=(c["P"], c["P"]), inverse_mode=inverse_mode)
    p = {k: torch.from_numpy(v) for k, v in gi.make_weights(c["wseed"], c["wscale"], in_chan=c["C"], lookback=c["lookback"], obj_px=c["P"]).items()}
    zt = {k: torch.from_numpy(z[k]) for k in ("z_attr", "z_where", "z_depth", "z_pres")}
    with torch.no_grad():
        objects = orc.decode_sprites(p, zt["z_attr"], zt["z_depth"], zt["z_pres"], cfg).permute(0, 3, 1, 2)
        zw = zt["z_where"].permute(0, 2, 3, 1).reshape(-1, 4)
        t = orc.stn(objects, zw, (c["H"], c["W"]), inverse=True, align_corners=cfg.align_corners, inverse_mode=inverse_mode)
    B, C = z["x"].shape[0], c["C"]
    t = t.numpy().astype(np.float64).reshape(B, -1, C + 2, c["H"], c["W"])
    imp = t[:, :, C + 1] + 1e-9
    return fx, t[:, :, C] * imp / imp.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("name", ph.PARSE_CASES)
def test_oracle_restatement_reproduces_the_reference_fixture(name):
    fx, w = oracle_weights(name)
    assert fx["owner"].dtype == np.int16 and fx["owner"].shape[1] in (w.shape[2], w.shape[2] // 2)
    k, w1, w2, cov = ph.top2(w)
    for thr in ph.THRESHOLDS:
        ph.check_against_fixture(fx, ph.owner_of(k, w1, thr), w1, cov, thr, what=name)
    # the fixture against itself: -1 exactly where nothing reaches the pixel, second weight below the first
    assert np.array_equal(fx["owner"] < 0, fx["w1"] == 0) and (fx["w2"] <= fx["w1"]).all()
    assert (fx["coverage"] >= fx["w1"] - 1e-6).all() and fx["coverage"].max() <= 1 + 1e-5


@pytest.mark.parametrize("name", ("c1_b8_step7001", "rect_h48w80_b4_step1001", "rgb_c1_b4_step1001"))
def test_definition_on_raw_operands_agrees_with_the_oracle(name):
    """parse_helpers.composite_weights (what the GPU tests hold the kernel to, on raw operands) is the same quantity as the oracle's
    decoder + stn + composite: closed-form inverse, float64 warp of the oracle's own sprites."""
    fx, z = ph.load_parse(name)
    c = ph.case_of(name)
    cfg = orc.OracleConfig(image_shape=(c["C"], c["H"], c["W"]), conv_strides=c["strides"], n_lookback=c["lookback"], object_shape=(c["P"], c["P"]))
    p = {k: torch.from_numpy(v) for k, v in gi.make_weights(c["wseed"], c["wscale"], in_chan=c["C"], lookback=c["lookback"], obj_px=c["P"]).items()}
    B = z["x"].shape[0]
    ones = torch.ones(B, 1, *z["z_pres"].shape[2:])
    with torch.no_grad():     # presence and depth 1: the alpha channel after the sigmoid alone
        alpha = orc.decode_sprites(p, torch.from_numpy(z["z_attr"]), ones, ones, cfg)[..., c["C"]].numpy()
    HW = alpha.shape[0] // B
    cells = lambda v: np.moveaxis(v, 1, -1).reshape(B, HW, -1)
    w = ph.composite_weights(alpha.reshape(B, HW, c["P"], c["P"]), cells(z["z_where"]), cells(z["z_pres"])[..., 0], cells(z["z_depth"])[..., 0],
                             c["H"], c["W"])
    k, w1, w2, cov = ph.top2(w)
    for thr in ph.THRESHOLDS:
        ph.check_against_fixture(fx, ph.owner_of(k, w1, thr), w1, cov, thr, what=name + " (raw operands)")


def test_boxes_formula_on_a_hand_example():
    from spair_pytorch_amd import parse_boxes
    # one sample, a 1 x 2 grid: cell 0 centred at (x, y) = (0.5, 0.25) of an 80 x 40 canvas, half its width and a quarter of its height
    zw = torch.tensor([[[[0.5, 0.9]], [[0.25, 0.5]], [[0.5, 0.2]], [[0.25, 1.0]]]])
    b = parse_boxes(zw, 40, 80)
    assert tuple(b.shape) == (1, 2, 4)
    assert torch.allclose(b[0, 0], torch.tensor([20.0, 5.0, 60.0, 15.0]))
    assert torch.allclose(b[0, 1], torch.tensor([64.0, 0.0, 80.0, 40.0]))
    # align_corners: the normalised extent g maps to index (g + 1) / 2 * (n - 1), whose pixel centre is half a pixel further
    b = parse_boxes(zw, 40, 80, align_corners=True)
    assert torch.allclose(b[0, 0], torch.tensor([0.25 * 79 + 0.5, 0.125 * 39 + 0.5, 0.75 * 79 + 0.5, 0.375 * 39 + 0.5]))
    assert torch.allclose(b[0, 1], torch.tensor([0.8 * 79 + 0.5, 0.5, 79.5, 39.5]))
    # the footprint is where the renderer's source coordinate runs over the texel square: [-0.5, P - 0.5], with align_corners [0, P - 1]
    for ac, (lo, hi) in ((False, (-0.5, 27.5)), (True, (0.0, 27.0))):
        bx = parse_boxes(zw, 40, 80, align_corners=ac)[0, 0].double().numpy()
        for edge, want in ((bx[0], lo), (bx[2], hi)):      # the continuous index of the edge is its pixel coordinate - 0.5
            j = edge - 0.5
            base = 2 * j / 79 - 1 if ac else (2 * j + 1) / 80 - 1
            g = base / 0.5 - (2 * 0.5 - 1) / 0.5
            s = (g + 1) / 2 * 27 if ac else ((g + 1) * 28 - 1) / 2
            assert abs(s - want) < 1e-5, (ac, s, want)


def test_parse_is_exported():
    import spair_pytorch_amd as sp
    from spair_pytorch_amd import models
    assert sp.SPAIR is models.SPAIR and sp.ParseResult is models.ParseResult and callable(sp.SPAIR.parse)
    assert {"SPAIR", "ParseResult", "parse_boxes"} <= set(sp.__all__)
    assert "owner" in sp.ParseResult.__slots__ and "boxes" in sp.ParseResult.__slots__
    for fn in ("spair_render_owner", "spair_parse_owner", "spair_cell_rows"):
        assert fn in open(__import__("os").path.join(__import__("os").path.dirname(ph.GOLDEN), "..", "include", "spair_hip.h")).read()
