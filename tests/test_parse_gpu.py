"""SPAIR.parse on the MI355X: the owner kernel against float64 on its own operands, the fp32 model against the reference's fixtures
(tests/golden/parse_<case>.npz), the bf16 model against float64 on the operands its forward stored, determinism and isolation from the
training run, the pixel boxes, and the benchmark geometry once.  The definition, the bounds and the comparison rule: parse_helpers.py.

Measured, not asserted (test_bf16_parse_on_its_stored_operands prints it per case): how often the bf16 model's owner differs from the
reference fixture outside a w1 - w2 <= 4e-3 margin -- the bf16 step's latents differ from the reference by their own, separately tested
bounds.  The measured shares are in DESIGN.md section 7, row f8."""
import numpy as np
import pytest
import torch

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


def build(name, dtype, cfg, weights=True):
    from spair_pytorch_amd.models import SPAIR
    c = ph.case_of(name)
    cfg.INPUT_IMAGE_SHAPE[0] = c["C"]
    cfg.set_grid(c["H"], c["strides"], image_width=c["W"])
    cfg.N_LOOKBACK = c["lookback"]
    cfg.OBJECT_SHAPE[:] = [c["P"], c["P"]]
    m = SPAIR([c["C"], c["H"], c["W"]], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
    if weights:
        w = gi.make_weights(c["wseed"], c["wscale"], in_chan=c["C"], lookback=c["lookback"], obj_px=c["P"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m, c


def fixture_inputs(z):
    return torch.from_numpy(z["x"]).cuda(), {k: torch.from_numpy(z[k]).cuda() for k in NOISE}, int(z["global_step"])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def fields(r):
    return {k: getattr(r, k) for k in r.__slots__}


# ---- 1. the kernel against float64 on its own operands ---------------------------------------------------------------------------------
UNIT = [
    #  seed B  G  Gw  I   Iw  P  ch  s16    ac  permute
    (1, 3, 5, 5, 48, 48, 28, 2, True, 0, True),
    (2, 2, 4, 7, 40, 72, 24, 4, False, 1, True),       # rectangular canvas, four channels per texel, align_corners
    (3, 8, 6, 6, 64, 64, 32, 2, False, 0, False),      # B % 8 == 0: the XCD-aware block order; identity rows
    (4, 1, 32, 32, 96, 96, 28, 2, True, 0, True),      # 1024 cells: four cull chunks
    (5, 2, 3, 5, 50, 35, 28, 4, True, 1, True),        # canvas sides that are no multiple of the tile, fp16 with four channels
    (6, 4, 4, 4, 32, 32, 24, 2, False, 1, False),
]


@pytest.mark.parametrize("seed,B,G,Gw,I,Iw,P,ch,s16,ac,permute", UNIT)
def test_owner_kernel_matches_float64_on_its_operands(seed, B, G, Gw, I, Iw, P, ch, s16, ac, permute):
    from spair_pytorch_amd import _lib as L
    HW = G * Gw
    c = ph.make_unit_case(seed, B, G, Gw, I, Iw, P, ch, permute)
    rows = c["rows"] if permute else np.arange(HW, dtype=np.int32)
    # storage order: cell k of sample b is row rows[k] * B + b
    r = (rows[None, :] * B + np.arange(B)[:, None]).reshape(-1)                       # [B*HW] row of (b, k)
    dt = torch.float16 if s16 else torch.float32
    tex = torch.from_numpy(c["texels"]).to(dt).reshape(B * HW, P * P * ch)
    ld = (P * P * ch + 7) // 8 * 8 + 8                                                # a padded leading dimension
    S = torch.full((B * HW, ld), float("nan"), dtype=dt)
    S[torch.from_numpy(r), :P * P * ch] = tex
    store = lambda v: torch.from_numpy(np.asarray(v).reshape(B * HW, -1))
    nbox, pres, depth = (torch.zeros(B * HW, n) for n in (4, 1, 1))
    nbox[torch.from_numpy(r)], pres[torch.from_numpy(r)], depth[torch.from_numpy(r)] = store(c["nbox"]), store(c["pres"]), store(c["depth"])
    alpha = tex.reshape(B, HW, P * P, ch)[..., ch - 1].double().numpy().reshape(B, HW, P, P)      # the stored values, exactly
    Sd = S.cuda()[:, :P * P * ch]
    for thr in ph.THRESHOLDS:
        run = lambda: L.render_owner(Sd, ch, nbox.cuda(), pres.cuda().reshape(-1), depth.cuda().reshape(-1), B, HW, I, Iw, P, bool(ac), thr,
                                     torch.from_numpy(rows).cuda() if permute else None)
        got, again = run(), run()
        for a_, b_ in zip(got, again):
            assert torch.equal(a_, b_), "two runs differ"
        if thr == 0:     # the large, fully present cell leads somewhere (its copy never does: check_on_operands)
            assert (got[0][c["twin"][0]] == c["twin"][1]).sum().item() > 0
        ph.check_on_operands(alpha, c["nbox"], c["pres"], c["depth"], [t.cpu().numpy() for t in got], thr, bool(ac), c["twin"],
                             what="unit %d" % seed)


def test_owner_kernel_refuses_what_it_cannot_run():
    from spair_pytorch_amd import _lib as L
    S = torch.zeros(2 * 1025, 8, device="cuda")
    z = torch.zeros(2 * 1025, 4, device="cuda")
    with pytest.raises(L.SpairHipError):      # more cells than the step itself takes
        L.render_owner(S, 2, z, z[:, 0], z[:, 0], 2, 1025, 16, 16, 2)
    with pytest.raises(L.SpairHipError):      # a sprite row shorter than P * P texels
        L.render_owner(S[:8], 2, z[:8], z[:8, 0], z[:8, 0], 2, 4, 16, 16, 28)


# ---- 2. the fp32 model against the reference's fixtures --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ph.PARSE_CASES)
def test_fp32_parse_matches_the_reference_fixture(name, cfg):
    fx, z = ph.load_parse(name)
    m, c = build(name, "f32", cfg)
    x, noise, step = fixture_inputs(z)
    for thr in ph.THRESHOLDS:
        r = m.parse(x, step, threshold=thr, noise=noise)
        assert rel(r.z_where.cpu().numpy(), z["z_where"]) < 1e-4 and rel(r.z_pres.cpu().numpy(), z["z_pres"]) < 1e-4
        assert rel(r.z_depth.cpu().numpy(), z["z_depth"]) < 1e-4 and rel(r.z_what.cpu().numpy(), z["z_attr"]) < 1e-4
        assert rel(r.recon.cpu().numpy(), z["recon_x"]) < 2e-4
        ph.check_against_fixture(fx, r.owner.cpu().numpy(), r.owner_weight.cpu().numpy(), r.coverage.cpu().numpy(), thr, what=name)
        own = r.owner.cpu().numpy()
        HW = r.area.shape[1]
        assert np.array_equal(r.area.cpu().numpy(), np.stack([np.bincount(o[o >= 0], minlength=HW) for o in own]))
    t = r.loss_terms.cpu().numpy()
    assert t.shape == (9,) and abs(t[0] - float(z["loss"])) <= 2e-5 * abs(float(z["loss"]))
    assert m.step_status() == 0


# ---- 3. the bf16 model on the operands its forward stored ------------------------------------------------------------------------------
def stored_operands(m, r, C, P):
    """alpha [B,HW,P,P] (float64, exact) from the sprites the forward left in the workspace, through the cell-to-row table; nbox / pres /
    depth as parse returned them."""
    B = r.z_where.shape[0]
    HW = r.area.shape[1]
    S = m.workspace_view("S")
    rows = m.cell_rows().cpu().numpy().astype(np.int64)
    assert sorted(rows.tolist()) == list(range(HW))
    idx = torch.from_numpy((rows[None, :] * B + np.arange(B)[:, None]).reshape(-1)).cuda()
    alpha = S[idx].reshape(B, HW, P * P, C + 1)[..., C].double().cpu().numpy().reshape(B, HW, P, P)
    cells = lambda v: v.permute(0, 2, 3, 1).reshape(B, HW, -1).cpu().numpy()
    return S.dtype, alpha, cells(r.z_where), cells(r.z_pres)[..., 0], cells(r.z_depth)[..., 0]


BF16_CASES = ("c1_b8_step7001", "c2_b2_step1001", "ref_default_b2_step1001", "c4_b1_step1001")


@pytest.mark.parametrize("name", BF16_CASES)
def test_bf16_parse_on_its_stored_operands(name, cfg):
    fx, z = ph.load_parse(name)
    m, c = build(name, "bf16", cfg)
    x, noise, step = fixture_inputs(z)
    assert m.step_plan(x.shape[0])["s16"] and m.step_plan(x.shape[0])["chain"]
    for thr in ph.THRESHOLDS:
        r = m.parse(x, step, threshold=thr, noise=noise)
        dt, alpha, nbox, pres, depth = stored_operands(m, r, c["C"], c["P"])
        assert dt == torch.float16
        got = [t.cpu().numpy() for t in (r.owner, r.owner_weight, r.coverage, r.area)]
        ph.check_on_operands(alpha, nbox, pres, depth, got, thr, what=name + " bf16")
    # measured, not asserted: agreement with the REFERENCE's owners (threshold 0) outside a 4e-3 margin
    rows_kept = fx["owner"].shape[1]
    own = r0 = m.parse(x, step, threshold=0.0, noise=noise).owner.cpu().numpy()[:, :rows_kept]
    clear = (fx["w1"] - fx["w2"]) > 4e-3
    print("%s bf16: owner differs from the reference fixture on %.3g of the pixels outside the w1 - w2 <= 4e-3 margin (%.3f of all inside it)"
          % (name, ((own != fx["owner"]) & clear).mean(), 1 - clear.mean()))


def test_bf16_parse_per_wavefront_launches_on_stored_operands(cfg, monkeypatch):
    """SPAIR_STEP_FLAGS bit 0: the per-wavefront launches (fp32 rows, still fp16 sprites) -- parse reads the formats that plan wrote."""
    from spair_pytorch_amd import models
    monkeypatch.setattr(models, "STEP_FLAGS", 1)
    name = "c1_b8_step7001"
    fx, z = ph.load_parse(name)
    m, c = build(name, "bf16", cfg)
    x, noise, step = fixture_inputs(z)
    assert not m.step_plan(x.shape[0])["chain"]
    r = m.parse(x, step, threshold=0.25, noise=noise)
    dt, alpha, nbox, pres, depth = stored_operands(m, r, c["C"], c["P"])
    ph.check_on_operands(alpha, nbox, pres, depth, [t.cpu().numpy() for t in (r.owner, r.owner_weight, r.coverage, r.area)], 0.25,
                         what=name + " bf16, flags 1")


def test_conv_decoder_fp32_sprites_on_stored_operands(cfg):
    """The conv object decoder writes fp32 sprites, in the bf16 step too."""
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(5)
    m = SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype="bf16", object_encoder="conv").to("cuda")
    x = torch.rand(4, 1, 48, 48, device="cuda")
    r = m.parse(x, 1001, threshold=0.25)
    dt, alpha, nbox, pres, depth = stored_operands(m, r, 1, 28)
    assert dt == torch.float32
    # an untrained model's cells are near copies of each other: about half of its pixels sit in a tie or at the threshold, so no share of
    # decided pixels is asked for here -- the weights and the coverage are held to their bounds on every pixel, the owner wherever it is decided
    ph.check_on_operands(alpha, nbox, pres, depth, [t.cpu().numpy() for t in (r.owner, r.owner_weight, r.coverage, r.area)], 0.25,
                         what="conv decoder", max_undecided=1.0)


# ---- 4. determinism and isolation ------------------------------------------------------------------------------------------------------
def small_model(dtype, cfg, seed=3):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(seed)
    return SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")


def small_batch(seed=1, B=8):
    return torch.from_numpy(gi.make_image(seed, B, 48, 3)).cuda()


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
def test_parse_is_repeatable_and_is_the_posterior_mean_forward(dtype, cfg):
    m = small_model(dtype, cfg)
    x = small_batch()
    a, b = fields(m.parse(x)), fields(m.parse(x))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    e = m._engine(x.shape[0])
    mean = {k: torch.full_like(v, 0.5 if k == "u_pres" else 0.0) for k, v in e["noise"].items()}
    with torch.no_grad():
        loss, recon, z_where, z_pres = m(x, 0, noise=mean)
    assert torch.equal(recon, a["recon"]) and torch.equal(z_where, a["z_where"]) and torch.equal(z_pres, a["z_pres"])
    assert torch.equal(m.loss_terms(), a["loss_terms"])
    # sample=True draws as forward does
    torch.manual_seed(77)
    s = m.parse(x, sample=True)
    torch.manual_seed(77)
    with torch.no_grad():
        loss, recon, z_where, z_pres = m(x)
    assert torch.equal(recon, s.recon) and torch.equal(z_where, s.z_where) and torch.equal(z_pres, s.z_pres)
    assert not torch.equal(s.z_where, a["z_where"])
    # the default draws nothing from torch's generators
    torch.manual_seed(78)
    before = torch.get_rng_state().clone()
    m.parse(x)
    assert torch.equal(torch.get_rng_state(), before)


def test_parse_between_steps_leaves_the_bf16_training_run_alone(cfg):
    """Ten Adam steps with a parse of the same batch size after every step against ten steps without: the bf16 step has no atomics and
    parse draws nothing, so the parameters are equal bit for bit."""
    from spair_pytorch_amd.optim import FusedAdam
    x, x_val = small_batch(1), small_batch(2)

    def train(with_parse):
        m = small_model("bf16", cfg)
        opt = FusedAdam(m, lr=1e-3)
        torch.manual_seed(11)
        for it in range(10):
            opt.zero_grad()
            m(x, 2000 + it)[0].backward()
            opt.step()
            if with_parse:
                m.parse(x_val, 2000 + it)
        assert m.step_status() == 0 and opt.skipped() == (0, False)
        return m.flat_parameters().cpu().numpy()

    assert np.array_equal(train(False), train(True))


def test_parse_between_steps_leaves_the_fp32_training_run_alone(cfg):
    """The fp32 step sums its bias / edge gradients with fp32 atomics, so two runs of the SAME program agree to rounding, not to the bit, and
    helpers.assert_adam_updates_close words what that allows for ONE update from equal state (test_checkpoint_gpu.py compares one such step).
    Ten updates apart the allowance does not apply: every step starts from what the one before left, and an element that moved the other way
    once keeps its distance (two runs without any parse differ as much; the first version of this test compared such trajectories at the
    one-step allowance).  So the ten steps are held to it one by one: model P parses after every step; before each step model A, which never
    parses, takes P's parameters and optimizer state, both do the step on the same noise, and the two updates must agree at the one-step
    allowance -- every step of P that follows a parse against the same step on a workspace no parse has touched."""
    from helpers import assert_adam_updates_close
    from spair_pytorch_amd.optim import FusedAdam
    x, x_val = small_batch(1), small_batch(2)
    P, A = small_model("f32", cfg), small_model("f32", cfg)
    oP, oA = FusedAdam(P, lr=1e-3), FusedAdam(A, lr=1e-3)
    oP._state(), oA._state()
    for it in range(10):
        A.flat_parameters().copy_(P.flat_parameters())
        oA.exp_avg.copy_(oP.exp_avg)
        oA.exp_avg_sq.copy_(oP.exp_avg_sq)
        oA.step_count = oP.step_count
        for m, opt in ((P, oP), (A, oA)):
            torch.manual_seed(100 + it)          # the step's noise
            opt.zero_grad()
            m(x, 2000 + it)[0].backward()
            opt.step()
        assert_adam_updates_close(P.flat_parameters().cpu().numpy(), A.flat_parameters().cpu().numpy(), 1e-3, tight=1e-6)
        r = P.parse(x_val, 2000 + it)
        assert torch.isfinite(r.coverage).all()
    assert P.step_status() == 0 and A.step_status() == 0 and oP.skipped() == (0, False) and oA.skipped() == (0, False)


def test_backward_through_a_forward_that_parse_overwrote_raises(cfg):
    from spair_pytorch_amd._lib import SpairHipError
    m = small_model("bf16", cfg)
    x = small_batch()
    loss = m(x, 1001)[0]
    m.parse(small_batch(2), 1001)
    with pytest.raises(SpairHipError):
        loss.backward()
    m.zero_grad()
    m(x, 1001)[0].backward()      # and a fresh forward trains as before
    m.parse(small_batch(2, B=4))  # another batch size has its own workspace
    assert m.step_status() == 0


# ---- 5. geometry -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ac", [("c1_b8_step7001", False), ("rect_h48w80_b4_step1001", False), ("p24_c1_b4_step1001", True),
                                     ("c2_b2_step1001", False)])
def test_boxes_and_owned_pixels_lie_together(name, ac, cfg):
    fx, z = ph.load_parse(name)
    cfg.ALIGN_CORNERS = ac
    m, c = build(name, "f32", cfg)
    x, noise, step = fixture_inputs(z)
    r = m.parse(x, step, threshold=0.25, noise=noise)
    I, Iw, P = c["H"], c["W"], c["P"]
    B, HW = r.area.shape
    zw = (r.z_where if ac else torch.from_numpy(z["z_where"])).double().cpu().permute(0, 2, 3, 1).reshape(B, HW, 4).numpy()
    xt, yt, xs, ys = (zw[..., i] for i in range(4))
    if ac:
        want = np.stack(((xt - xs / 2) * (Iw - 1) + 0.5, (yt - ys / 2) * (I - 1) + 0.5, (xt + xs / 2) * (Iw - 1) + 0.5,
                         (yt + ys / 2) * (I - 1) + 0.5), -1)
    else:      # against the formula on the FIXTURE's z_where
        want = np.stack(((xt - xs / 2) * Iw, (yt - ys / 2) * I, (xt + xs / 2) * Iw, (yt + ys / 2) * I), -1)
    boxes = r.boxes.double().cpu().numpy()
    assert boxes.shape == (B, HW, 4)
    assert np.abs(boxes - want).max() <= 1e-4 * max(I, Iw)
    # every owned pixel's centre lies in its owner's box grown by one texel of the (P - 1)-texel extent: the zero-padded bilinear footprint
    own = r.owner.cpu().numpy()
    b, y, x_ = np.nonzero(own >= 0)
    k = own[b, y, x_]
    assert len(k) > 0.05 * own.size
    gx, gy = xs[b, k] * Iw / (P - 1), ys[b, k] * I / (P - 1)
    bx = boxes[b, k]
    inside = (x_ + 0.5 >= bx[:, 0] - gx) & (x_ + 0.5 <= bx[:, 2] + gx) & (y + 0.5 >= bx[:, 1] - gy) & (y + 0.5 <= bx[:, 3] + gy)
    assert inside.all(), int((~inside).sum())


# ---- 6. the benchmark geometry, once ------------------------------------------------------------------------------------------------------
def test_parse_at_the_benchmark_geometry(cfg):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(128, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(3)
    m = SPAIR([1, 128, 128], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
    B = 256
    x = torch.cat([torch.from_numpy(gi.make_image(40 + i, 32, 128, 11)) for i in range(B // 32)]).cuda()
    r = m.parse(x, 1001, threshold=0.25)
    assert tuple(r.owner.shape) == (B, 128, 128) and tuple(r.area.shape) == (B, 256) and tuple(r.boxes.shape) == (B, 256, 4)
    for k, v in fields(r).items():
        assert torch.isfinite(v.float()).all(), k
    assert int(r.owner.min()) >= -1 and int(r.owner.max()) < 256
    assert float(r.coverage.min()) >= 0 and float(r.coverage.max()) <= 1 + 1e-5 and bool((r.owner_weight <= r.coverage * (1 + 1e-6)).all())
    own = r.owner.reshape(B, -1).long()
    counts = torch.zeros(B, 257, dtype=torch.long, device="cuda").scatter_add_(1, own + 1, torch.ones_like(own))
    assert torch.equal(counts[:, 1:], r.area.long())
    assert int(r.area.sum()) + int((r.owner < 0).sum()) == B * 128 * 128
    again = m.parse(x, 1001, threshold=0.25)
    for k, v in fields(r).items():
        assert torch.equal(v, getattr(again, k)), k
    assert m.step_status() == 0
