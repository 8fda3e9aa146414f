"""SPAIR.compose on the MI355X: the fp32 model on fixture weights against the reference (the base fixtures' stored latents and recon,
tests/golden/compose_<case>.npz for edited latents and object layers), the layer kernel against float64 on made-up operands, the layers'
sum against recon, the cross-check with parse, the round trip compose(parse(x)), isolation from the training run, argument errors and
the benchmark geometry once.  Definitions, the edit rule and the bounds: compose_helpers.py (and parse_helpers.py).

Stated, not asserted to the bit: ``layer_weight`` of the owning cell against ``parse``'s ``owner_weight``.  The two kernels share the
taps and the coordinate arithmetic, but not the denominator: the layer kernel multiplies by the 1/D the renderer forward stored (a sum in
the rows' dependency-wavefront order), the owner kernel sums D itself in row-major cell order.  test_layer_weight_agrees_with_parse
prints the observed difference and holds it to the two evaluations' fp32 bounds."""
import numpy as np
import pytest
import torch

import compose_helpers as ch
import golden_inputs as gi
import parse_helpers as ph

pytestmark = pytest.mark.gpu

NOISE = ("eps_box", "eps_attr", "eps_depth", "u_pres")


@pytest.fixture
def cfg():
    from spair_pytorch_amd import config as cfg
    old = (list(cfg.INPUT_IMAGE_SHAPE), [t["stride"] for t in cfg.DEFAULT_BACKBONE_TOPOLOGY], cfg.N_LOOKBACK, cfg.ALIGN_CORNERS,
           list(cfg.OBJECT_SHAPE))
    yield cfg
    cfg.INPUT_IMAGE_SHAPE[:] = old[0]
    for t, s in zip(cfg.DEFAULT_BACKBONE_TOPOLOGY, old[1]):
        t["stride"] = s
    cfg.N_LOOKBACK, cfg.ALIGN_CORNERS = old[2], old[3]
    cfg.OBJECT_SHAPE[:] = old[4]


def build(name, dtype, cfg):
    from spair_pytorch_amd.models import SPAIR
    c = ch.case_of(name)
    cfg.INPUT_IMAGE_SHAPE[0] = c["C"]
    cfg.set_grid(c["H"], c["strides"], image_width=c["W"])
    cfg.N_LOOKBACK = c["lookback"]
    cfg.OBJECT_SHAPE[:] = [c["P"], c["P"]]
    m = SPAIR([c["C"], c["H"], c["W"]], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
    w = gi.make_weights(c["wseed"], c["wscale"], in_chan=c["C"], lookback=c["lookback"], obj_px=c["P"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m, c


def cuda(z, *keys):
    return [torch.from_numpy(np.ascontiguousarray(z[k])).cuda() for k in keys]


def base_fixture(name):
    return np.load(ch.GOLDEN + "/" + name + ".npz")


def small_model(dtype, cfg, seed=3, **kw):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(seed)
    return SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype=dtype, **kw).to("cuda")


def small_batch(seed=1, B=8):
    return torch.from_numpy(gi.make_image(seed, B, 48, 3)).cuda()


def stored_texels(m, B, HW, P, C):
    """texels [B,HW,P*P,C+1] (float64, exact) of the sprites the latest compose / forward left in the workspace, in cell order."""
    S = m.workspace_view("S")
    rows = m.cell_rows().cpu().numpy().astype(np.int64)
    idx = torch.from_numpy((rows[None, :] * B + np.arange(B)[:, None]).reshape(-1)).cuda()
    return S.dtype, S[idx].reshape(B, HW, P * P, C + 1).double().cpu().numpy()


# ---- 1. the fp32 model against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ch.CASES + ch.EXTRA_BASE)
def test_unedited_latents_reproduce_the_fixture_recon(name, cfg):
    z = base_fixture(name)
    m, c = build(name, "f32", cfg)
    zw, zt, zd, zp = cuda(z, "z_where", "z_attr", "z_depth", "z_pres")
    r = m.compose(z_where=zw, z_what=zt, z_depth=zd, z_pres=zp)
    err = np.abs(r.recon.cpu().numpy().astype(np.float64) - z["recon_x"]).max()
    print("%s: |compose(stored latents) - recon_x| %.3g" % (name, err))
    assert r.layers is None and r.layer_weight is None and tuple(r.boxes.shape) == (zw.shape[0], zw.shape[2] * zw.shape[3], 4)
    assert err <= ch.TOL, (name, err)


@pytest.mark.parametrize("name", ch.CASES)
def test_edited_latents_match_the_reference_render_and_layers(name, cfg):
    fx = ch.load_compose(name)
    m, c = build(name, "f32", cfg)
    zw, zt, zd, zp, cells = cuda(fx, "z_where", "z_what", "z_depth", "z_pres", "cells")

    class Scene:
        z_where, z_what, z_depth, z_pres = zw, zt, zd, zp

    r = m.compose(Scene, layers=cells)
    rows = fx["recon"].shape[2]
    B, K = cells.shape
    assert tuple(r.layers.shape) == (B, K, c["C"], c["H"], c["W"]) and tuple(r.layer_weight.shape) == (B, K, c["H"], c["W"])
    e_r = np.abs(r.recon.cpu().numpy()[:, :, :rows].astype(np.float64) - fx["recon"]).max()
    e_l = np.abs(r.layers.cpu().numpy()[:, :, :, :rows].astype(np.float64) - fx["layers"]).max()
    e_w = np.abs(r.layer_weight.cpu().numpy()[:, :, :rows].astype(np.float64) - fx["layer_weight"]).max()
    moved = np.abs(fx["recon"] - base_fixture(name)["recon_x"][:, :, :rows]).max()
    print("%s: recon err %.3g, layers err %.3g, layer_weight err %.3g (the edit moves recon by %.3f; rows %d)" % (name, e_r, e_l, e_w, moved, rows))
    assert moved > 0.1                                # a wrong implementation cannot hide inside the tolerance
    assert e_r <= ch.TOL and e_l <= ch.TOL and e_w <= ch.TOL, (name, e_r, e_l, e_w)
    assert not r.layers[:, K - 1].any() and not r.layer_weight[:, K - 1].any()       # the -1 entry
    # keyword tensors override single fields of the scene
    r2 = m.compose(Scene, z_pres=torch.zeros_like(zp))
    assert float(r2.recon.abs().max()) == 0.0


# ---- 2. the layers' sum, on the operands the compose stored --------------------------------------------------------------------------------
def layer_check(m, c, lat, cells, r, what):
    """r.layers / r.layer_weight against float64 on the stored sprites and the given latents at compose_helpers.layer_bounds; returns the
    per-pixel bound of |sum of the layers of ALL cells - recon| and the float64 parts."""
    zw, zt, zd, zp = lat
    B, HW = zw.shape[0], zw.shape[2] * zw.shape[3]
    dt, tex = stored_texels(m, B, HW, c["P"], c["C"])
    nbox, pres, depth = ch.to_cells(zw.cpu().numpy()), ch.to_cells(zp.cpu().numpy())[..., 0], ch.to_cells(zd.cpu().numpy())[..., 0]
    lay, lw, pre, a, mm, reach, D, col = ch.layers_float64(tex, nbox, pres, depth, cells.cpu().numpy(), c["H"], c["W"])
    w, E_w, E_col = ch.layer_bounds(a, mm, reach, nbox, pres, c["P"])
    E_lay = ch.layer_error(w, E_w, E_col, col)                          # [B,HW,C,I,Iw]
    cl = cells.cpu().numpy().astype(np.int64)
    ok = (cl >= 0) & (cl < HW)
    kk, bi = np.where(ok, cl, 0), np.arange(B)[:, None]
    fin = np.isfinite(E_w[bi, kk])
    r_w = (np.abs(r.layer_weight.cpu().numpy() - lw) / (E_w[bi, kk] + 1e-30))[fin]
    fin_l = np.isfinite(E_lay[bi, kk])
    r_l = (np.abs(r.layers.cpu().numpy() - lay) / (E_lay[bi, kk] + 1e-30))[fin_l]
    print("%s: layer_weight err %.3g (%.3f of its bound), layers err %.3g (%.3f of its bound), bound median where an object reaches %.3g, finite %.4f"
          % (what, np.abs(r.layer_weight.cpu().numpy() - lw)[fin].max(), r_w.max(), np.abs(r.layers.cpu().numpy() - lay)[fin_l].max(),
             r_l.max(), np.median(E_w[bi, kk][fin & (E_w[bi, kk] > 0)]), fin.mean()))
    assert r_w.max() <= 1 and r_l.max() <= 1, (what, r_w.max(), r_l.max())
    assert fin.mean() >= 0.99 and np.median(E_w[bi, kk][fin & (E_w[bi, kk] > 0)]) < 0.5 * ch.TOL, "vacuous bound"
    # pixels no requested object reaches, and skipped cells, are exact zeros
    dead = ~(reach[bi, kk] & ok[:, :, None, None])
    assert not r.layer_weight.cpu().numpy()[dead].any()
    return dict(E_lay=E_lay, E_w=E_w, pre=pre, reach=reach)


@pytest.mark.parametrize("name", ["c1_b8_step7001", "rgb_c1_b4_step1001"])
def test_layers_of_all_cells_sum_to_recon(name, cfg):
    """6 x 6 grids, `cells` lists all 36.  Both sides are fp32 evaluations of the same float64 sum of n terms t_k = w_k col_k: the layers
    each within E_layer_k of t_k (layer_check), recon's numerator terms g a (m + 1e-9) within the same E_layer_k D of t_k D, its
    n-term fp32 accumulation within n 2^-24 of the sum of magnitudes, one product with 1/D and the store.  The layers are summed here in
    float64, so the test adds no rounding of its own:  |sum layers - recon| <= 2 sum_k E_layer_k + (n + 2) 2^-24 sum_k t_k."""
    fx = ch.load_compose(name)
    m, c = build(name, "f32", cfg)
    lat = cuda(fx, "z_where", "z_what", "z_depth", "z_pres")
    B, HW = lat[0].shape[0], lat[0].shape[2] * lat[0].shape[3]
    assert HW == 36
    cells = torch.arange(HW, device="cuda").repeat(B, 1)
    r = m.compose(z_where=lat[0], z_what=lat[1], z_depth=lat[2], z_pres=lat[3], layers=cells)
    f = layer_check(m, c, lat, cells, r, name)
    total = r.layers.double().sum(dim=1).cpu().numpy()
    n = f["reach"].sum(axis=1)[:, None]
    bound = 2 * f["E_lay"].sum(axis=1) + (n + 2) * 2.0 ** -24 * f["pre"]
    recon = r.recon.double().cpu().numpy()
    fin = np.isfinite(bound) & (recon < 1)              # (where the composite's clamp acts, recon is not the sum)
    diff = np.abs(total - recon)
    print("%s: |sum of 36 layers - recon| %.3g (%.3f of its bound; bound median %.3g, max finite %.3g), recon max %.3f"
          % (name, diff[fin].max(), (diff[fin] / (bound[fin] + 1e-30)).max(), np.median(bound[fin]), bound[fin].max(), float(r.recon.max())))
    assert (diff[fin] <= bound[fin]).all()
    assert fin.mean() >= 0.99 and np.median(bound[fin]) < 0.5 * ch.TOL, "vacuous bound"
    assert float(r.recon.max()) > 0.2
    assert float(r.layer_weight.sum(dim=1).max()) <= 1 + 1e-5


# ---- 3. the cross-check with parse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_b8_step7001", "rect_h48w80_b4_step1001"])
def test_layer_weight_agrees_with_parse(name, cfg):
    _, z = ph.load_parse(name)
    m, c = build(name, "f32", cfg)
    x = torch.from_numpy(z["x"]).cuda()
    noise = {k: torch.from_numpy(z[k]).cuda() for k in NOISE}
    p = m.parse(x, int(z["global_step"]), threshold=0.0, noise=noise)
    B, HW = p.area.shape
    cells = torch.argsort(p.area, dim=1, descending=True, stable=True)[:, :8]
    r = m.compose(p, layers=cells)
    lat = (p.z_where, p.z_what, p.z_depth, p.z_pres)
    E_w = layer_check(m, c, lat, cells, r, name + " (parse's scene)")["E_w"]
    own = p.owner.cpu().numpy().astype(np.int64)
    cl = cells.cpu().numpy()
    hit = own[:, None] == cl[:, :, None, None]                      # [B,K,I,Iw]: the owner is the j-th requested cell
    assert hit.any(axis=1).mean() > 0.05
    got = np.where(hit, r.layer_weight.cpu().numpy(), 0).sum(axis=1)
    want = p.owner_weight.cpu().numpy()
    sel = hit.any(axis=1)
    diff = np.abs(got - want)[sel]
    # both are fp32 evaluations of w_owner, each within E_w of float64 (parse_helpers.fp32_bounds covers either denominator)
    bi = np.arange(B)[:, None, None]
    E_own = E_w[bi, np.maximum(own, 0), np.arange(c["H"])[None, :, None], np.arange(c["W"])[None, None, :]]
    fin = np.isfinite(E_own[sel])
    print("%s: layer_weight of the owner against parse's owner_weight: bit-equal on %.4f of %d pixels, max difference %.3g (%.3f of the two "
          "bounds)" % (name, (diff == 0).mean(), diff.size, diff.max(), (diff[fin] / (2 * E_own[sel][fin] + 1e-30)).max()))
    assert (diff[fin] <= 2 * E_own[sel][fin]).all()
    assert torch.equal(r.recon, p.recon)


# ---- 4. the round trip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_b8_step7001", "rgb_c1_b4_step1001", "rect_h48w80_b4_step1001", "lb2_c1_b4_step1001"])
def test_round_trip_fp32_is_bit_identical(name, cfg):
    _, z = ph.load_parse(name)
    m, c = build(name, "f32", cfg)
    x = torch.from_numpy(z["x"]).cuda()
    p = m.parse(x, int(z["global_step"]), noise={k: torch.from_numpy(z[k]).cuda() for k in NOISE})
    r = m.compose(p)
    assert torch.equal(r.recon, p.recon) and torch.equal(r.boxes, p.boxes)
    assert torch.equal(m.export_map(0), p.z_what) and torch.equal(m.export_map(1), p.z_depth)      # what the import left in the rows


@pytest.mark.parametrize("flags,conv", [(0, False), (1, False), (0, True)])
def test_round_trip_bf16_is_bit_identical(flags, conv, cfg, monkeypatch):
    """The fused chain rounds Za16 from the fp32 attribute its record row holds (chain.hip), the per-wavefront launches convert Za with
    spair_to_bf16, the conv decoder reads the fp32 Za: in each case the import reproduces the decoder's input to the bit."""
    from spair_pytorch_amd import models
    monkeypatch.setattr(models, "STEP_FLAGS", flags)
    m = small_model("bf16", cfg, object_encoder="conv" if conv else None)
    x = small_batch()
    plan = m.step_plan(x.shape[0])
    assert plan["chain"] == (flags == 0 and not conv)
    p = m.parse(x, 2000)
    S0 = m.workspace_view("S").clone()
    r = m.compose(p, layers=torch.arange(8, device="cuda").repeat(x.shape[0], 1))
    assert torch.equal(m.workspace_view("S"), S0)
    assert torch.equal(r.recon, p.recon)
    # (the matrix-core renderer's 1/D carries its fp16 hat weights: the weights of a pixel sum to 1 within its own 5e-4-class error)
    assert torch.isfinite(r.layers).all() and float(r.layer_weight.sum(dim=1).max()) <= 1.01


# ---- 5. kernel units ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_import_then_export_is_exact(dtype, cfg):
    m = small_model(dtype, cfg)
    B, G, A = 5, 6, 50
    g = torch.Generator(device="cuda").manual_seed(5)
    zw = torch.rand(B, 4, G, G, device="cuda", generator=g) * 0.5 + 0.2
    zt = torch.randn(B, A, G, G, device="cuda", generator=g)
    zd, zp = torch.rand(B, 1, G, G, device="cuda", generator=g), torch.rand(B, 1, G, G, device="cuda", generator=g)
    m.compose(z_where=zw, z_what=zt, z_depth=zd, z_pres=zp)
    assert torch.equal(m.export_map(0), zt) and torch.equal(m.export_map(1), zd)
    rows = m.cell_rows().long()
    idx = (rows[None, :] * B + torch.arange(B, device="cuda")[:, None]).reshape(-1)
    want = zt.permute(0, 2, 3, 1).reshape(B * G * G, A)
    Za = m.workspace_view("Za", padded=True)
    assert torch.equal(Za[idx][:, :A], want) and not Za[:, A:].any()
    if dtype == "bf16":
        Za16 = m.workspace_view("Za16", padded=True)
        assert torch.equal(Za16[idx][:, :A], want.to(torch.bfloat16)) and not Za16[:, A:].any()


UNIT = [
    #  seed B  G  Gw  I   Iw  P  ch  s16    ac
    (1, 3, 5, 5, 48, 48, 28, 2, True, 0),
    (2, 2, 4, 7, 40, 72, 24, 4, False, 1),       # rectangular canvas, four channels per texel, align_corners
    (3, 8, 6, 6, 64, 64, 32, 2, False, 0),
    (4, 1, 32, 32, 96, 96, 28, 2, True, 0),      # 1024 cells
    (5, 2, 3, 5, 50, 35, 28, 4, True, 1),        # canvas sides that are no multiple of the tile, fp16 with four channels
    (6, 4, 4, 4, 32, 32, 24, 2, False, 1),
    (7, 3, 4, 5, 40, 56, 28, 3, True, 0),        # three elements per texel (two colour channels), fp16 ...
    (8, 2, 5, 4, 48, 32, 24, 3, False, 1),       # ... and fp32
]


@pytest.mark.parametrize("seed,B,G,Gw,I,Iw,P,chn,s16,ac", UNIT)
def test_layer_kernel_matches_float64_on_its_operands(seed, B, G, Gw, I, Iw, P, chn, s16, ac):
    from spair_pytorch_amd import _lib as L
    HW = G * Gw
    c = ph.make_unit_case(seed, B, G, Gw, I, Iw, P, chn, True)
    rows = c["rows"]
    r = (rows[None, :] * B + np.arange(B)[:, None]).reshape(-1)                       # [B*HW] row of (b, k)
    dt = torch.float16 if s16 else torch.float32
    tex = torch.from_numpy(c["texels"]).to(dt).reshape(B * HW, P * P * chn)
    ld = (P * P * chn + 7) // 8 * 8 + 8                                               # a padded leading dimension
    S = torch.full((B * HW, ld), float("nan"), dtype=dt)
    S[torch.from_numpy(r), :P * P * chn] = tex
    store = lambda v: torch.from_numpy(np.asarray(v).reshape(B * HW, -1))
    nbox, pres, depth = (torch.zeros(B * HW, n) for n in (4, 1, 1))
    nbox[torch.from_numpy(r)], pres[torch.from_numpy(r)], depth[torch.from_numpy(r)] = store(c["nbox"]), store(c["pres"]), store(c["depth"])
    texels = tex.reshape(B, HW, P * P, chn).double().numpy()                          # the stored values, exactly
    rng = np.random.default_rng(seed)
    K = 12 if HW >= 12 else HW
    cells = np.stack([rng.choice(HW, K, replace=False) for _ in range(B)]).astype(np.int64)
    cells[:, 0] = np.arange(B) % 4                       # one box of every kind (make_unit_case: ordinary, magnified, few-pixel, half outside)
    cells[:, 1], cells[:, 2], cells[:, 3] = -1, HW, 10 ** 6
    cells[:, 4] = cells[:, 5]                            # a duplicate
    cells[0, 6] = c["twin"][1]
    lay, lw, pre, a, m, reach, D, col = ch.layers_float64(texels, c["nbox"], c["pres"], c["depth"], cells, I, Iw, bool(ac))
    inv_den = torch.from_numpy((1.0 / D[:, 0]).astype(np.float32))
    Sd = S.cuda()[:, :P * P * chn]
    run = lambda: L.render_layers(Sd, chn, nbox.cuda(), pres.cuda().reshape(-1), depth.cuda().reshape(-1), torch.from_numpy(cells).cuda(),
                                  inv_den.cuda(), B, HW, I, Iw, P, bool(ac), torch.from_numpy(rows).cuda())
    (gl, gw), (gl2, gw2) = run(), run()
    assert torch.equal(gl, gl2) and torch.equal(gw, gw2), "two runs differ"
    gl, gw = gl.cpu().numpy(), gw.cpu().numpy()
    w, E_w, E_col = ch.layer_bounds(a, m, reach, c["nbox"], c["pres"], P)
    E_lay = ch.layer_error(w, E_w, E_col, col)
    ok = (cells >= 0) & (cells < HW)
    kk, bi = np.where(ok, cells, 0), np.arange(B)[:, None]
    Ew, El = E_w[bi, kk], E_lay[bi, kk]
    fin = np.isfinite(Ew)
    r_w = (np.abs(gw - lw) / (Ew + 1e-30))[fin]
    r_l = (np.abs(gl - lay) / (El + 1e-30))[np.isfinite(El)]
    print("unit %d: layer_weight err %.3g (%.3f of its bound), layers err %.3g (%.3f of its bound), bound median where an object reaches %.3g, finite %.4f, "
          "weight max %.3f" % (seed, np.abs(gw - lw)[fin].max(), r_w.max(), np.abs(gl - lay)[np.isfinite(El)].max(), r_l.max(),
                               np.median(Ew[fin & (Ew > 0)]), fin.mean(), gw.max()))
    assert r_w.max() <= 1 and r_l.max() <= 1
    assert fin.mean() >= 0.99 and np.median(Ew[fin & (Ew > 0)]) < 0.5 * ch.TOL, "vacuous bound"
    assert lw.max() > 0 and gw.max() > 0
    assert not gw[:, 1:4].any() and not gl[:, 1:4].any()                 # -1, HW and 10**6: all-zero layers
    assert np.array_equal(gw[:, 4], gw[:, 5]) and np.array_equal(gl[:, 4], gl[:, 5])
    dead = ~(reach[bi, kk] & ok[:, :, None, None])
    assert not gw[dead].any()
    assert gw[0, 6].max() > 0                                            # the large, fully present cell


def test_layer_kernel_refuses_what_it_cannot_run():
    from spair_pytorch_amd import _lib as L
    S = torch.zeros(8, 8, device="cuda")
    z = torch.zeros(8, 4, device="cuda")
    cells = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    inv = torch.ones(2, 16, 16, device="cuda")
    with pytest.raises(L.SpairHipError):      # a sprite row shorter than P * P texels
        L.render_layers(S, 2, z, z[:, 0], z[:, 0], cells, inv, 2, 4, 16, 16, 28)
    with pytest.raises(L.SpairHipError):      # five elements per texel
        L.render_layers(S, 5, z, z[:, 0], z[:, 0], cells, inv, 2, 4, 16, 16, 1)


# ---- 6. the training run is left alone ---------------------------------------------------------------------------------------------------
def test_compose_between_steps_leaves_the_bf16_training_run_alone(cfg):
    from spair_pytorch_amd.optim import FusedAdam
    x, x_val = small_batch(1), small_batch(2)

    def train(with_compose):
        m = small_model("bf16", cfg)
        opt = FusedAdam(m, lr=1e-3)
        scene = m.parse(x_val, 2000)
        cells = torch.arange(8, device="cuda").repeat(x_val.shape[0], 1)
        torch.manual_seed(11)
        for it in range(10):
            opt.zero_grad()
            m(x, 2000 + it)[0].backward()
            if with_compose and it % 2:      # between backward() and the optimizer step too
                m.compose(scene, layers=cells)
            opt.step()
            if with_compose:
                before = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
                m.compose(scene, layers=cells)
                assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(), before[1])
        assert m.step_status() == 0 and opt.skipped() == (0, False)
        return m.flat_parameters().cpu().numpy()

    assert np.array_equal(train(False), train(True))


def test_compose_leaves_the_step_status_word_alone(cfg):
    """Between backward() and FusedAdam.step() of a step whose flag a made-up non-finite value set: compose neither clears the flag (the
    optimizer still skips the step) nor raises, and on a clean model it sets nothing.  The non-finite value is the one test_status_gpu.py
    uses -- a NaN in one bias of the attribute encoder, which makes that step's Gaussian KL term NaN and nothing else; no GPU fault is
    involved.  (compose itself reads the object decoder's parameters only, so what it renders stays finite.)"""
    from spair_pytorch_amd._lib import SpairHipError
    from spair_pytorch_amd.optim import FusedAdam
    m = small_model("bf16", cfg)
    opt = FusedAdam(m, lr=1e-3)
    x = small_batch()
    scene = m.parse(x, 2000)
    assert m.step_status() == 0
    m.compose(scene)
    assert m.step_status() == 0 and m._status_host[0] == 0
    bias = dict(m.named_parameters())["object_encoder.out.bias"]
    keep = bias.detach().clone()
    with torch.no_grad():
        bias[3] = float("nan")
    params = m.flat_parameters().clone()
    opt.zero_grad()
    m(x, 2000)[0].backward()
    word = m._status_dev.clone()
    r = m.compose(scene, layers=torch.arange(8, device="cuda").repeat(x.shape[0], 1))
    assert torch.equal(m._status_dev, word) and int(word[0]) & 2
    assert torch.isfinite(r.recon).all() and torch.isfinite(r.layers).all()
    opt.step()
    assert opt.skipped()[0] == 1
    assert torch.equal(torch.nan_to_num(m.flat_parameters(), nan=7.0), torch.nan_to_num(params, nan=7.0))
    m.compose(scene)                       # still no complaint from compose: it reads no status
    with pytest.raises(SpairHipError, match="non-finite"):
        m(x, 2001)
    with torch.no_grad():
        bias.copy_(keep)
    m.clear_step_status()
    assert m.step_status() == 0


def test_backward_through_a_forward_that_compose_overwrote_raises(cfg):
    from spair_pytorch_amd._lib import SpairHipError
    m = small_model("bf16", cfg)
    x = small_batch()
    scene = m.parse(x, 1001)
    loss = m(x, 1001)[0]
    m.compose(scene)
    with pytest.raises(SpairHipError, match="overwritten"):
        loss.backward()
    m.zero_grad()
    m(x, 1001)[0].backward()      # and a fresh forward trains as before
    assert m.step_status() == 0


# ---- 7. argument errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(cfg):
    from spair_pytorch_amd._lib import SpairHipError
    m = small_model("f32", cfg)
    p = m.parse(small_batch(B=4), 2000)
    with pytest.raises(AssertionError):
        m.compose(p, z_what=p.z_what[:, :49])
    with pytest.raises(AssertionError):
        m.compose(p, z_pres=p.z_pres[:2])
    with pytest.raises(AssertionError):
        m.compose(p, z_where=p.z_where[:, :, :5])
    with pytest.raises(AssertionError):
        m.compose(p, layers=torch.zeros(3, 8, dtype=torch.int64, device="cuda"))
    with pytest.raises(AssertionError):
        m.compose(z_where=p.z_where, z_what=p.z_what, z_depth=p.z_depth)           # no z_pres anywhere
    with pytest.raises(SpairHipError):
        m.compose(p, z_depth=p.z_depth.cpu())
    with pytest.raises(SpairHipError):
        m.compose(p, layers=torch.zeros(4, 8, dtype=torch.int64))
    r = m.compose(p, z_pres=p.z_pres.double(), layers=torch.tensor([[0, 35, 36, -5]] * 4, device="cuda"))      # converted; 36 and -5: skipped
    assert torch.equal(r.recon, p.recon) and not r.layers[:, 2:].any()


# ---- 8. the benchmark geometry, once ------------------------------------------------------------------------------------------------------
def test_compose_at_the_benchmark_geometry(cfg):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(128, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(3)
    m = SPAIR([1, 128, 128], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
    B = 256
    x = torch.cat([torch.from_numpy(gi.make_image(40 + i, 32, 128, 11)) for i in range(B // 32)]).cuda()
    p = m.parse(x, 1001, threshold=0.25)
    cells = torch.argsort(p.area, dim=1, descending=True, stable=True)[:, :8]
    r = m.compose(p, layers=cells)
    assert torch.equal(r.recon, p.recon)
    assert tuple(r.layers.shape) == (B, 8, 1, 128, 128) and tuple(r.layer_weight.shape) == (B, 8, 128, 128)
    for v in (r.recon, r.layers, r.layer_weight):
        assert torch.isfinite(v).all()
    assert float(r.layer_weight.min()) >= 0 and float(r.layer_weight.sum(dim=1).max()) <= 1.01
    again = m.compose(p, layers=cells)
    assert torch.equal(again.recon, r.recon) and torch.equal(again.layers, r.layers) and torch.equal(again.layer_weight, r.layer_weight)
    assert m.step_status() == 0
