"""SPAIR.evaluate on the MI355X: k_sample_terms alone against float64 on made-up operands at the bound derived from their magnitudes
(evaluate_helpers.fp32_bounds), the fp32 model against the oracle on the reference's fixtures, the bf16 model against float64 on the
operands its own forward stored, the draws, determinism and isolation from the training run, and the benchmark geometry once.

Measured (printed by the tests): the largest fraction of the derived bound per output, and the largest
distance of the fp32 model's maps from the oracle's."""
import ctypes

import numpy as np
import pytest
import torch

import evaluate_helpers as eh
import golden_inputs as gi
import parse_helpers as ph

pytestmark = pytest.mark.gpu

NOISE = ("eps_box", "eps_attr", "eps_depth", "u_pres")


@pytest.fixture
def cfg():
    from spair_pytorch_amd import config as cfg
    old = (list(cfg.INPUT_IMAGE_SHAPE), [t["stride"] for t in cfg.DEFAULT_BACKBONE_TOPOLOGY], cfg.N_LOOKBACK, list(cfg.OBJECT_SHAPE))
    yield cfg
    cfg.INPUT_IMAGE_SHAPE[:] = old[0]
    for t, s in zip(cfg.DEFAULT_BACKBONE_TOPOLOGY, old[1]):
        t["stride"] = s
    cfg.N_LOOKBACK = old[2]
    cfg.OBJECT_SHAPE[:] = old[3]


def build(name, dtype, cfg):
    from spair_pytorch_amd.models import SPAIR
    c = ph.case_of(name)
    cfg.INPUT_IMAGE_SHAPE[0] = c["C"]
    cfg.set_grid(c["H"], c["strides"], image_width=c["W"])
    cfg.N_LOOKBACK = c["lookback"]
    cfg.OBJECT_SHAPE[:] = [c["P"], c["P"]]
    m = SPAIR([c["C"], c["H"], c["W"]], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
    w = gi.make_weights(c["wseed"], c["wscale"], in_chan=c["C"], lookback=c["lookback"], obj_px=c["P"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m, c


def fixture_inputs(z):
    return torch.from_numpy(z["x"]).cuda(), {k: torch.from_numpy(z[k]).cuda() for k in NOISE}, int(z["global_step"])


def small_model(dtype, cfg, seed=3):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(seed)
    return SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")


def small_batch(seed=1, B=8):
    return torch.from_numpy(gi.make_image(seed, B, 48, 3)).cuda()


# the fp32 model's maps against the oracle's, relative to the map's maximum: the largest seen over the seven fixtures (kl_map 2.5e-7 on
# c1_b8_step7001, bce_map 1.71e-5 on c4_b1_step1001; per fixture: DESIGN.md section 7, row f12); asserted at four times that -- an upstream
# latent difference of up to 1e-4 may land on a steeper cell in another run -- and never above eh.MAP_CAP
KL_MAP_OBSERVED, BCE_MAP_OBSERVED = 2.5e-7, 1.71e-5


def slices_of(B, HW, I, Iw):
    from spair_pytorch_amd import _lib as L
    n = int(L.lib().spair_sample_terms_scratch_floats(B, HW, I, Iw))
    assert n > 0 and n % (8 * B) == 0
    return n // (8 * B)


def to_np(out):
    return [None if t is None else t.double().cpu().numpy() for t in out]


def unit(seed, B, HW, A, C, I, Iw, permute):
    c = eh.make_unit_case(seed, B, HW, A, C, I, Iw, permute)
    st = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in eh.store_rows(c, B, HW, A).items()}
    st["recon"], st["x"] = torch.from_numpy(c["recon"]).cuda(), torch.from_numpy(c["x"]).cuda()
    pri = eh.config_priors()
    args = (c["z"], c["pz"], c["mu"], c["sd"], pri, 0.75, c["recon"], c["x"])
    return c, st, pri, eh.terms_float64(*args), eh.fp32_bounds(*args, slices=slices_of(B, HW, I, Iw))


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,B,HW,A,C,I,Iw,permute", eh.UNIT_CASES)
def test_kernel_matches_float64_on_its_operands(seed, B, HW, A, C, I, Iw, permute):
    c, st, pri, ref, bounds = unit(seed, B, HW, A, C, I, Iw, permute)
    got = eh.run_rows(c, st, pri, 0.75)
    again = eh.run_rows(c, st, pri, 0.75)
    for a_, b_ in zip(got, again):
        assert torch.equal(a_, b_), "two runs differ"
    assert tuple(got[0].shape) == (B, 9) and tuple(got[1].shape) == (B, 7, HW) and tuple(got[2].shape) == (B, I, Iw)
    g = to_np(got)
    eh.check_outputs(g, ref, bounds, what="unit %d" % seed)
    # without the maps: the same terms, bit for bit
    bare = eh.run_rows(c, st, pri, 0.75, maps=False)
    assert bare[1] is None and bare[2] is None and torch.equal(bare[0], got[0])
    # the bound bites: the reference without one pixel, one cell or one attribute element is out of it
    terms, kl_map, bce_map = ref
    b = B - 1
    for what, j, gone in (("pixel", 1, bce_map[b].max()), ("cell", 8, np.abs(kl_map[b, 6]).max()),
                          ("attribute lane", 6, np.abs(eh._pieces(c["z"], c["pz"], c["mu"], c["sd"], pri, c["recon"], c["x"])[0][4][b]).max())):
        short = terms.copy()
        short[b, j] -= gone
        with pytest.raises(AssertionError):
            eh.check_outputs(g, (short, kl_map, bce_map), bounds, what="unit %d without one %s" % (seed, what))


@pytest.mark.parametrize("case", (2, 3))
def test_accumulate_over_three_calls_is_the_mean(case):
    spec = eh.UNIT_CASES[case]
    runs = [unit(100 * k + spec[0], *spec[1:]) for k in range(3)]
    B, HW, A, C, I, Iw = spec[1:7]
    out = (torch.empty(B, 9, device="cuda"), torch.full((B, 7, HW), float("nan"), device="cuda"), torch.full((B, I, Iw), float("nan"), device="cuda"))
    plain = []
    for k, (c, st, pri, ref, bounds) in enumerate(runs):
        c = dict(c, rows=runs[0][0]["rows"])              # (one cell-to-row table for the three)
        st = {k_: (v.cuda() if torch.is_tensor(v) else v) for k_, v in eh.store_rows(c, B, HW, A).items()}
        st["recon"], st["x"] = torch.from_numpy(c["recon"]).cuda(), torch.from_numpy(c["x"]).cuda()
        plain.append(to_np(eh.run_rows(c, st, pri, 0.75)))
        eh.run_rows(c, st, pri, 0.75, out=out, accumulate=k > 0, scale=1.0 / 3)
        assert np.array_equal(out[0].double().cpu().numpy(), plain[-1][0])          # terms: written plainly, the latest call's
    for i in (1, 2):
        mean = sum(p[i] for p in plain) / 3
        ref_mean = sum(r[3][i] for r in runs) / 3
        bound = sum(r[4][i] for r in runs) / 3 + 4 * eh.E32 * sum(np.abs(r[3][i]) for r in runs) / 3
        got = out[i].double().cpu().numpy()
        assert (np.abs(got - mean) <= 4 * eh.E32 * sum(np.abs(p[i]) for p in plain) / 3 + 1e-30).all()
        assert (np.abs(got - ref_mean) <= bound + 1e-30).all()


# ---- 2. the fp32 model against the oracle on the reference's fixtures ---------------------------------------------------------------------
def held_to_oracle(t, want, what):
    """terms [B,9] against the oracle's: BCE within 2e-5 relative, each KL within 1e-4 of the larger of the sample's value and the batch
    mean of that term."""
    e_b = np.abs(t[:, 1] - want[:, 1]) / np.abs(want[:, 1])
    scale = np.maximum(np.abs(want[:, 2:]), np.abs(want[:, 2:]).mean(axis=0, keepdims=True))
    e_k = np.abs(t[:, 2:] - want[:, 2:]) / scale
    print("%s: terms against the oracle: BCE %.3g, KLs %s" % (what, e_b.max(), " ".join("%.2g" % v for v in e_k.max(axis=0))))
    assert e_b.max() <= eh.BCE_TOL and e_k.max() <= eh.KL_TOL, (what, e_b.max(), e_k.max())


def batch_identities(r, B, world=1, what=""):
    t, lt = r.terms_draws[-1].double().cpu().numpy(), r.loss_terms.double().cpu().numpy()
    e_b = abs(t[:, 1].sum() - lt[1]) / abs(lt[1])
    e_k = np.abs(t[:, 2:].sum(axis=0) / (B * world) - lt[2:9]) / np.abs(lt[2:9])
    print("%s: batch identities: BCE %.3g, KLs %.3g" % (what, e_b, e_k.max()))
    assert e_b <= eh.BCE_TOL and e_k.max() <= eh.KL_TOL, (what, e_b, e_k)


@pytest.mark.parametrize("name", eh.FIXTURES)
def test_fp32_model_matches_the_oracle_on_the_fixture(name, cfg):
    o, pz, (terms, kl_map, bce_map) = eh.fixture_reference(name)
    m, c = build(name, "f32", cfg)
    x, noise, step = fixture_inputs(o["npz"])
    r = m.evaluate(x, step, noise=noise)
    B, G, Gw = o["B"], o["G"], o["Gw"]
    assert tuple(r.terms.shape) == (B, 9) and tuple(r.terms_draws.shape) == (1, B, 9) and tuple(r.kl_map.shape) == (B, 7, G, Gw)
    assert tuple(r.bce_map.shape) == (B, c["H"], c["W"]) and tuple(r.loss.shape) == (B,) and torch.equal(r.loss, r.terms[:, 0])
    t = r.terms.double().cpu().numpy()
    held_to_oracle(t, terms, name)
    assert np.abs(t[:, 0] - terms[:, 0]).max() <= eh.BCE_TOL * np.abs(terms[:, 0]).max() + eh.KL_TOL * np.abs(terms[:, 2:]).sum(axis=1).max()
    batch_identities(r, B, what=name)
    e_kl = np.abs(r.kl_map.double().cpu().numpy().reshape(B, 7, -1) - kl_map).max() / np.abs(kl_map).max()
    e_bce = np.abs(r.bce_map.double().cpu().numpy() - bce_map).max() / bce_map.max()
    print("%s: maps against the oracle, relative to the map's maximum: kl_map %.3g, bce_map %.3g" % (name, e_kl, e_bce))
    assert 4 * KL_MAP_OBSERVED <= eh.MAP_CAP and 4 * BCE_MAP_OBSERVED <= eh.MAP_CAP
    assert e_kl <= 4 * KL_MAP_OBSERVED and e_bce <= 4 * BCE_MAP_OBSERVED, (name, e_kl, e_bce)
    assert m.step_status() == 0


# ---- 3. the bf16 model on the operands its forward stored ---------------------------------------------------------------------------------
def held_to_its_stored_operands(m, r, x, what):
    """evaluate's outputs against float64 on what the model's own forward left in the workspace (export_map 2 .. 14 walks the rows through
    the cell-to-row table) and returned (z_pres, recon), at the derived bound."""
    B, _, G, Gw = r.z_pres.shape
    HW = G * Gw
    rows = m.cell_rows().cpu().numpy()
    assert sorted(rows.tolist()) == list(range(HW))
    cells = lambda v: v.double().permute(0, 2, 3, 1).reshape(B, HW, -1).cpu().numpy()
    mu, sd = [cells(m.export_map(2 + j)) for j in range(6)], [cells(m.export_map(8 + j)) for j in range(6)]
    z, pz = cells(r.z_pres)[..., 0], cells(m.export_map(14))[..., 0]
    Oe = m.workspace_view("Oe")                                                              # [N, 2A] = [mean | logstd], fp32 in every plan
    idx = torch.from_numpy((rows[None, :].astype(np.int64) * B + np.arange(B)[:, None]).reshape(-1)).cuda()
    A = mu[4].shape[-1]
    assert np.array_equal(Oe[idx][:, :A].double().cpu().numpy().reshape(B, HW, A), mu[4])      # the rows the kernel walks ARE these maps
    pri = eh.config_priors()
    I, Iw = x.shape[2:]
    args = (z, pz, mu, sd, pri, 1.0, r.recon.double().cpu().numpy(), x.double().cpu().numpy())
    fr = eh.check_outputs(to_np((r.terms_draws[-1], r.kl_map.reshape(B, 7, HW), r.bce_map)), eh.terms_float64(*args),
                          eh.fp32_bounds(*args, slices=slices_of(B, HW, I, Iw)), what=what)
    batch_identities(r, B, what=what)
    return fr


@pytest.mark.parametrize("name", ("c1_b8_step7001", "c2_b2_step1001"))
def test_bf16_fused_chain_on_its_stored_operands(name, cfg):
    m, c = build(name, "bf16", cfg)
    x, noise, step = fixture_inputs(eh.fixture_operands(name)["npz"])
    assert m.step_plan(x.shape[0])["chain"]
    held_to_its_stored_operands(m, m.evaluate(x, step, noise=noise), x, name + " bf16")
    assert m.step_status() == 0


def test_bf16_per_wavefront_launches_on_stored_operands(cfg, monkeypatch):
    from spair_pytorch_amd import models
    monkeypatch.setattr(models, "STEP_FLAGS", 1)
    name = "c1_b8_step7001"
    m, c = build(name, "bf16", cfg)
    x, noise, step = fixture_inputs(eh.fixture_operands(name)["npz"])
    assert not m.step_plan(x.shape[0])["chain"]
    held_to_its_stored_operands(m, m.evaluate(x, step, noise=noise), x, name + " bf16, flags 1")


def test_bf16_conv_object_pair_on_stored_operands(cfg):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(5)
    m = SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype="bf16", object_encoder="conv").to("cuda")
    x = small_batch(3, B=4)
    held_to_its_stored_operands(m, m.evaluate(x, 1001, seed=3), x, "conv object pair")


# ---- 4. the draws, determinism, isolation ----------------------------------------------------------------------------------------------------
def fields(r):
    return {k: getattr(r, k) for k in r.__slots__ if getattr(r, k) is not None}


def same(a, b):
    fa, fb = fields(a), fields(b)
    assert fa.keys() == fb.keys()
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k


def rng_states():
    return torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
def test_draws_and_repeatability(dtype, cfg):
    m = small_model(dtype, cfg)
    x = small_batch()
    B = x.shape[0]
    # the posterior mean: repeatable to the bit, nothing drawn
    torch.manual_seed(78)
    before = rng_states()
    a, b = m.evaluate(x, 1001, sample=False), m.evaluate(x, 1001, sample=False)
    same(a, b)
    assert all(torch.equal(u, v) for u, v in zip(before, rng_states()))
    p = m.parse(x, 1001)
    assert torch.equal(p.recon, a.recon) and torch.equal(p.loss_terms, a.loss_terms)
    # seed=: repeatable, no torch generator touched, the mean over the draws, draw k = seed + k
    s3, s3b = m.evaluate(x, 1001, seed=7, samples=3), m.evaluate(x, 1001, seed=7, samples=3)
    same(s3, s3b)
    assert all(torch.equal(u, v) for u, v in zip(before, rng_states()))
    assert tuple(s3.terms_draws.shape) == (3, B, 9) and torch.equal(s3.terms, s3.terms_draws.mean(0)) and torch.equal(s3.loss, s3.terms[:, 0])
    singles = [m.evaluate(x, 1001, seed=7 + k) for k in range(3)]
    for k, s in enumerate(singles):
        assert torch.equal(s3.terms_draws[k], s.terms_draws[0]) and torch.equal(s.terms, s.terms_draws[0])
    assert not torch.equal(singles[0].terms, singles[1].terms)
    assert torch.equal(s3.recon, singles[2].recon) and torch.equal(s3.loss_terms, singles[2].loss_terms)
    for name in ("kl_map", "bce_map"):          # the maps: the mean of the three draws' maps, accumulated in place
        mean = sum(getattr(s, name).double() for s in singles) / 3
        got = getattr(s3, name).double()
        assert float((got - mean).abs().max()) <= 8 * eh.E32 * float(mean.abs().max())
    # seed=None: one seed from torch's CPU generator
    torch.manual_seed(5)
    n1 = m.evaluate(x, 1001)
    assert not torch.equal(torch.get_rng_state(), before[0])
    torch.manual_seed(5)
    same(n1, m.evaluate(x, 1001))
    # noise=: a no_grad forward with that noise
    e = m._engine(B)
    noise = {k: torch.empty_like(v) for k, v in e["noise"].items()}
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd.models import NOISE_MAPS
    L.check(L.lib().spair_noise_fill(ctypes.byref(e["dims"]), 9, *(L.ptr(noise[k]) for k in NOISE_MAPS), L.stream()), "spair_noise_fill")
    rn = m.evaluate(x, 1001, noise=noise, seed=1234)
    with torch.no_grad():
        loss, recon, z_where, z_pres = m(x, 1001, noise=noise)
    assert torch.equal(recon, rn.recon) and torch.equal(m.loss_terms(), rn.loss_terms) and torch.equal(z_pres, rn.z_pres)
    same(rn, m.evaluate(x, 1001, seed=9))                    # ... which is what seed=9 fills
    # maps=False: the same terms
    bare = m.evaluate(x, 1001, seed=7, samples=3, maps=False)
    assert bare.kl_map is None and bare.bce_map is None and torch.equal(bare.terms_draws, s3.terms_draws) and torch.equal(bare.terms, s3.terms)
    assert m.step_status() == 0


def test_world_size_plays_no_part_in_the_terms(cfg):
    m = small_model("f32", cfg)
    x = small_batch()
    a = m.evaluate(x, 1001, seed=3)
    m.world_size = 4
    b = m.evaluate(x, 1001, seed=3)
    m.world_size = 1
    assert torch.equal(a.terms, b.terms) and torch.equal(a.kl_map, b.kl_map) and not torch.equal(a.loss_terms, b.loss_terms)
    batch_identities(b, x.shape[0], world=4, what="world_size 4")


def test_argument_errors(cfg):
    from spair_pytorch_amd._lib import SpairHipError
    m = small_model("bf16", cfg)
    x = small_batch()
    e = m._engine(x.shape[0])
    noise = {k: torch.zeros_like(v) + 0.5 for k, v in e["noise"].items()}
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=2, noise=noise), dict(samples=2, sample=False)):
        with pytest.raises(AssertionError):
            m.evaluate(x, **kw)
    with pytest.raises(AssertionError):
        m.evaluate(x[:, :, :40])
    with pytest.raises(AssertionError):
        m.evaluate(x, noise=dict(noise, eps_attr=noise["eps_attr"][:, :7]))
    with pytest.raises(SpairHipError):
        m.evaluate(x.cpu())


def test_backward_through_a_forward_that_evaluate_overwrote_raises(cfg):
    from spair_pytorch_amd._lib import SpairHipError
    m = small_model("bf16", cfg)
    x = small_batch()
    loss = m(x, 1001)[0]
    m.evaluate(small_batch(2), 1001, seed=1)
    with pytest.raises(SpairHipError):
        loss.backward()
    m.zero_grad()
    m(x, 1001)[0].backward()
    m.evaluate(small_batch(2, B=4), seed=1)      # another batch size has its own workspace
    assert m.step_status() == 0


def test_evaluate_between_steps_leaves_the_bf16_training_run_alone(cfg):
    """Ten Adam steps with an evaluate(seed=...) of the same batch size after every step against ten steps without: the bf16 step has no
    atomics and evaluate(seed=) draws nothing from torch, so the parameters are equal bit for bit."""
    from spair_pytorch_amd.optim import FusedAdam
    x, x_val = small_batch(1), small_batch(2)

    def train(with_eval):
        m = small_model("bf16", cfg)
        opt = FusedAdam(m, lr=1e-3)
        torch.manual_seed(11)
        for it in range(10):
            opt.zero_grad()
            m(x, 2000 + it)[0].backward()
            opt.step()
            if with_eval:
                assert torch.isfinite(m.evaluate(x_val, 2000 + it, seed=it, samples=2).loss).all()
        assert m.step_status() == 0 and opt.skipped() == (0, False)
        return m.flat_parameters().cpu().numpy()

    assert np.array_equal(train(False), train(True))


# ---- 5. the benchmark geometry, once ------------------------------------------------------------------------------------------------------
def test_evaluate_at_the_benchmark_geometry(cfg):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(128, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(3)
    m = SPAIR([1, 128, 128], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
    B = 256
    x = torch.cat([torch.from_numpy(gi.make_image(40 + i, 32, 128, 11)) for i in range(B // 32)]).cuda()
    r = m.evaluate(x, 1001, seed=1)
    assert tuple(r.terms.shape) == (B, 9) and tuple(r.kl_map.shape) == (B, 7, 16, 16) and tuple(r.bce_map.shape) == (B, 128, 128)
    for k, v in fields(r).items():
        assert torch.isfinite(v).all(), k
    assert float(r.kl_map[:, :6].min()) >= -1e-5 and float(r.bce_map.min()) >= 0
    batch_identities(r, B, what="B = 256, 16 x 16 cells")
    t, km, bm = r.terms.double(), r.kl_map.double().sum(dim=(2, 3)), r.bce_map.double().sum(dim=(1, 2))
    assert float(((km - t[:, 2:]).abs() / (t[:, 2:].abs() + 1e-3)).max()) <= 1e-5 and float(((bm - t[:, 1]).abs() / t[:, 1]).max()) <= 1e-5
    same(r, m.evaluate(x, 1001, seed=1))
    assert m.step_status() == 0
