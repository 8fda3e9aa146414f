"""SPAIR.compose without a GPU: the oracle's decoder + stn + composite reproduce every reference fixture tests/golden/compose_<case>.npz
(which pins the definition and the fixture generator to each other), the stored edits follow compose_helpers.edit_latents when recomputed
from the base and parse fixtures, the public names, and the fixture sizes."""
import os

import numpy as np
import pytest
import torch

import compose_helpers as ch
import golden_inputs as gi
import parse_helpers as ph
from oracle import spair_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_setup(name):
    c = ch.case_of(name)
    cfg = orc.OracleConfig(image_shape=(c["C"], c["H"], c["W"]), conv_strides=c["strides"], n_lookback=c["lookback"],
                           object_shape=(c["P"], c["P"]))
    p = {k: torch.from_numpy(v) for k, v in gi.make_weights(c["wseed"], c["wscale"], in_chan=c["C"], lookback=c["lookback"], obj_px=c["P"]).items()}
    return c, cfg, p


@pytest.mark.parametrize("name", ch.CASES)
def test_oracle_reproduces_the_compose_fixture(name):
    fx = ch.load_compose(name)
    c, cfg, p = oracle_setup(name)
    zt = {k: torch.from_numpy(fx[k]) for k in ("z_what", "z_where", "z_depth", "z_pres")}
    C, I, Iw = c["C"], c["H"], c["W"]
    with torch.no_grad():
        # (oracle.render takes square grids only; the rectangular case's recon is formed below from the same decoder + stn output)
        recon = orc.render(p, zt["z_what"], zt["z_where"], zt["z_depth"], zt["z_pres"], cfg).numpy() if I == Iw else None
        objects = orc.decode_sprites(p, zt["z_what"], zt["z_depth"], zt["z_pres"], cfg).permute(0, 3, 1, 2)
        t = orc.stn(objects, zt["z_where"].permute(0, 2, 3, 1).reshape(-1, 4), (I, Iw), inverse=True, align_corners=cfg.align_corners,
                    inverse_mode=cfg.inverse_mode)
    B = fx["z_where"].shape[0]
    t = t.numpy().astype(np.float64).reshape(B, -1, C + 2, I, Iw)
    HW = t.shape[1]
    imp = t[:, :, C + 1] + 1e-9
    w = t[:, :, C] * imp / imp.sum(axis=1, keepdims=True)
    composite = np.clip((w[:, :, None] * t[:, :, :C]).sum(axis=1), 0, 1)
    recon = composite if recon is None else recon
    assert np.abs(composite - recon).max() < 1e-5
    cells = fx["cells"].astype(np.int64)
    assert cells.shape == (B, ch.K_LAYERS) and (cells[:, -1] == -1).all() and (cells[:, :-1] >= 0).all() and cells.max() < HW
    ok = cells >= 0
    kk, bi = np.where(ok, cells, 0), np.arange(B)[:, None]
    lw = w[bi, kk] * ok[:, :, None, None]
    lay = lw[:, :, None] * t[bi, kk][:, :, :C]
    rows = fx["recon"].shape[2]
    assert rows in (I, I // 2, I // 4) and fx["layers"].shape == (B, ch.K_LAYERS, C, rows, Iw) and fx["layer_weight"].shape == (B, ch.K_LAYERS, rows, Iw)
    e_r = np.abs(recon[:, :, :rows] - fx["recon"]).max()
    e_l, e_w = np.abs(lay[:, :, :, :rows] - fx["layers"]).max(), np.abs(lw[:, :, :rows] - fx["layer_weight"]).max()
    print("%s: oracle against the fixture: recon %.3g, layers %.3g, layer_weight %.3g" % (name, e_r, e_l, e_w))
    assert e_r <= ch.TOL and e_l <= ch.TOL and e_w <= ch.TOL
    # the fixture against itself: the -1 layer is zero, a layer is its weight times a colour in [0, 1], the weights of a pixel sum to <= 1
    assert not fx["layers"][:, -1].any() and not fx["layer_weight"][:, -1].any()
    assert (fx["layers"] <= fx["layer_weight"][:, :, None] + 1e-7).all() and fx["layer_weight"].min() >= 0
    assert fx["layer_weight"][:, :6].sum(axis=1).max() <= 1 + 1e-5 and fx["layer_weight"].max() > 0.05


@pytest.mark.parametrize("name", ("c1_b8_step7001", "rgb_c1_b4_step1001", "rect_h48w80_b4_step1001"))
def test_definition_on_raw_operands_agrees_with_the_fixture(name):
    """compose_helpers.layers_float64 (what the GPU tests hold the kernel to, on raw operands) is the reference's quantity: on the
    oracle's own sprites (presence and depth 1: the values after the sigmoid alone) it reproduces the fixture's layers."""
    fx = ch.load_compose(name)
    c, cfg, p = oracle_setup(name)
    B = fx["z_where"].shape[0]
    ones = torch.ones(B, 1, *fx["z_pres"].shape[2:])
    with torch.no_grad():
        tex = orc.decode_sprites(p, torch.from_numpy(fx["z_what"]), ones, ones, cfg)[..., :c["C"] + 1].numpy()
    HW = tex.shape[0] // B
    tex = tex.reshape(B, HW, c["P"] * c["P"], c["C"] + 1)
    lay, lw, pre, *_ = ch.layers_float64(tex, ch.to_cells(fx["z_where"]), ch.to_cells(fx["z_pres"])[..., 0], ch.to_cells(fx["z_depth"])[..., 0],
                                         fx["cells"], c["H"], c["W"])
    rows = fx["recon"].shape[2]
    e = [np.abs(lay[:, :, :, :rows] - fx["layers"]).max(), np.abs(lw[:, :, :rows] - fx["layer_weight"]).max(),
         np.abs(pre[:, :, :rows] - fx["recon"]).max()]
    print("%s: definition on raw operands against the fixture: layers %.3g, layer_weight %.3g, sum of all %.3g" % (name, *e))
    assert max(e) <= ch.TOL


@pytest.mark.parametrize("name", ch.CASES)
def test_stored_edits_follow_the_rule(name):
    fx = ch.load_compose(name)
    parse, z = ph.load_parse(name)
    zw, zt, zd, zp, cells = ch.edit_latents(z["z_where"], z["z_attr"], z["z_depth"], z["z_pres"], parse["owner"])
    for k, v in (("z_where", zw), ("z_what", zt), ("z_depth", zd), ("z_pres", zp), ("cells", cells)):
        assert fx[k].dtype == v.dtype and np.array_equal(fx[k], v), k
    B = zw.shape[0]
    HW = zw.shape[2] * zw.shape[3]
    area = ch.cell_areas(parse["owner"], HW)
    for b in range(B):
        top = cells[b, :6]
        assert (np.diff(area[b][top]) <= 0).all() and area[b][top[5]] >= np.delete(area[b], top).max()
        assert not zp[b, 0].reshape(-1)[top[:2]].any() and (z["z_pres"][b, 0].reshape(-1)[top[:2]] > 0).all()
        assert abs(float(zw[b, 0].reshape(-1)[cells[b, 6]] - z["z_where"][b, 0].reshape(-1)[cells[b, 6]]) - 0.1) < 1e-6
        # every edit changes something: two presences, two boxes, two attribute vectors, and the depths are a permutation of themselves
        assert (zw[b] != z["z_where"][b]).sum() == 2 and (zp[b] != z["z_pres"][b]).sum() == 2
        assert (zt[b] != z["z_attr"][b]).any() and np.array_equal(np.sort(zd[b].reshape(-1)), np.sort(z["z_depth"][b].reshape(-1)))
        here = z["z_pres"][b, 0].reshape(-1) > 0.5
        if here.sum() > 1:
            d0, d1 = z["z_depth"][b, 0].reshape(-1)[here], zd[b, 0].reshape(-1)[here]
            asc = np.argsort(d0, kind="stable")
            assert np.array_equal(d1[asc], d0[asc][::-1])
            assert d1[np.argmin(d0)] == d0.max() and d1[np.argmax(d0)] == d0.min()


def test_compose_is_exported():
    import spair_pytorch_amd as sp
    from spair_pytorch_amd import _lib, models
    assert sp.ComposeResult is models.ComposeResult and callable(sp.SPAIR.compose) and "ComposeResult" in sp.__all__
    assert sp.ComposeResult.__slots__ == ("recon", "boxes", "layers", "layer_weight")
    doc = sp.SPAIR.compose.__doc__
    for word in ("AS GIVEN", "z_pres = 0", "generation", "FusedAdam"):
        assert word in doc, word
    header = open(os.path.join(ROOT, "include", "spair_hip.h")).read()
    for fn in ("spair_compose", "spair_render_layers", "spair_render_layers_rows"):
        assert "int %s(" % fn in header
        assert fn in open(_lib.__file__).read()
    assert "#define SPAIR_ABI_VERSION %d" % _lib.ABI_VERSION in header and callable(_lib.render_layers)
    if os.path.exists(_lib.LIB_PATH):
        h = _lib.lib()
        for fn in ("spair_compose", "spair_render_layers", "spair_render_layers_rows"):
            assert hasattr(h, fn)


def test_fixture_sizes():
    for name in ch.CASES:
        path = os.path.join(ch.GOLDEN, "compose_" + name + ".npz")
        assert os.path.getsize(path) <= 1000000, (name, os.path.getsize(path))
