"""SPAIR.generate on the MI355X.

The sampler at unit level (spair_prior_presence through _lib.prior_presence) against generate_helpers.presence_float64 under the
TEACHER-FORCED rule: on the kernel's own z_pres the float64 recursion gives p_z64 per cell; the kernel's p_z must lie within 5e-5 of it
(the bound tests/test_countkl_gpu.py holds k_count_kl to), its decision must equal [u < p_z64] wherever |u - p_z64| > 5e-5, and at most
0.5 % of a case's cells may lie inside that margin (test_generate_cpu.py shows the seeds used here stay under it on the reference alone).
The exact-count mode is checked to the bit against its closed form in fp32.

The planted dense patterns run at p = 0.999999 (the step-0 value) and p = 0.99: a pattern of ~1000 present cells needs prior mass at
counts ~1000, and an fp32 prior has none there once p^1000 underflows (p = 0.9: 1e-46), in the kernel as in the reference's own fp32
evaluation; a float64 reference is only meaningful where the fp32 prior exists.

Then the Gaussian maps against float64 at bounds derived from the operand magnitudes (generate_helpers.gauss_bounds) and the model-level
properties: repeatability, compose(generate(...)), layers, seeds and generators, the status word, isolation from training, errors, and
one call at B = 256 on 16 x 16 cells.

Observed (MI355X; printed by the tests): DESIGN.md section 7, row f11."""
import numpy as np
import pytest
import torch

import generate_helpers as gh
import golden_inputs as gi

pytestmark = pytest.mark.gpu

NOISE = ("eps_box", "eps_attr", "eps_depth", "u_pres")


def run_presence(u, p, count=None):
    from spair_pytorch_amd import _lib as L
    z, pz, n = L.prior_presence(torch.from_numpy(np.ascontiguousarray(u)).cuda(), p, count)
    return z.cpu().numpy(), pz.cpu().numpy(), n.cpu().numpy()


# ---- 1. the sampler under the teacher-forced rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", gh.SAMPLER_HW)
def test_sampler_follows_the_teacher_forced_rule(HW):
    worst = 0.0
    for B in gh.SAMPLER_B:
        for p in gh.SAMPLER_P:
            u = gh.uniform_u(gh.sampler_seed(HW, B, p), B, HW)
            z, pz, n = run_presence(u, p)
            assert z.shape == (B, HW) and pz.shape == (B, HW) and n.shape == (B,) and n.dtype == np.int32
            pz64 = gh.presence_float64(HW, B, prob=p, z=z)[1]
            err, _ = gh.check_presence_rule(u, z, pz, n, pz64, "HW %d, B %d, p %g" % (HW, B, p))
            worst = max(worst, err)
    print("HW %d: largest |p_z - p_z64| over its cases %.3g" % (HW, worst))


# ---- 2. planted dense patterns -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one_off", "iid", "runs"])
@pytest.mark.parametrize("HW,B", [(256, 64), (1024, 64)])
def test_sampler_on_planted_dense_patterns(HW, B, kind):
    """u = 0 switches a cell on wherever p_z > 0, u = 1 - 2^-24 switches it off wherever p_z < 1: the planted pattern itself must come out
    (on the float64 reference every p_z of these patterns lies in [0.08, 0.9995]), under the same rule."""
    on = gh.dense_patterns(kind, B, HW)
    u = np.where(on, np.float32(0), gh.ONE_BELOW).astype(np.float32)
    for p in (0.999999, 0.99):
        z, pz, n = run_presence(u, p)
        pz64 = gh.presence_float64(HW, B, prob=p, z=z)[1]
        gh.check_presence_rule(u, z, pz, n, pz64, "HW %d, %s, p %g" % (HW, kind, p))
        assert np.array_equal(z > 0.5, on), (kind, p)


# ---- 3. exact count ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [1, 2, 65, 128, 1024])
def test_exact_count(HW):
    B = 5
    ns = sorted({0, 1, HW // 2, HW - 1, HW})
    for tag, u in (("random", gh.uniform_u(7 + HW, B, HW)), ("zeros", np.zeros((B, HW), np.float32)),
                   ("one_below", np.full((B, HW), gh.ONE_BELOW, np.float32))):
        for n in ns:
            z, pz, got = run_presence(u, 0.5, n)
            zr, pzr, nr = gh.exact_count_fp32(HW, n, u)
            assert (got == n).all() and np.array_equal(z.sum(axis=1), np.full(B, n, np.float32)), (tag, n)
            assert np.array_equal(z, zr) and np.array_equal(pz.view(np.int32), pzr.view(np.int32)), (tag, n)
            if tag == "zeros":
                assert z[:, :n].all() and not z[:, n:].any()
            if tag == "one_below":
                assert z[:, HW - n:].all() and not z[:, :HW - n].any()
        # per-sample counts, out-of-range values included: -3 is 0, HW + 7 is HW
        mixed = np.array([-3, HW + 7, HW // 2, 1, HW - 1], np.int64)
        z, pz, got = run_presence(u, float("nan"), torch.from_numpy(mixed).cuda())      # (count given: the probability is not read)
        zr, pzr, nr = gh.exact_count_fp32(HW, mixed, u)
        assert np.array_equal(got, np.clip(mixed, 0, HW)) and np.array_equal(got, nr), tag
        assert np.array_equal(z, zr) and np.array_equal(pz.view(np.int32), pzr.view(np.int32)), tag


# ---- 4. the distribution ---------------------------------------------------------------------------------------------------------------------
def test_sampler_distribution():
    B, HW = 4096, 16
    u = gh.uniform_u(5, B, HW)
    z, _, n = run_presence(u, 0.5, 4)
    assert (n == 4).all()
    sigma = np.sqrt(0.25 * 0.75 / B)
    freq = z.mean(axis=0)
    print("count = 4: cell frequencies %.4f .. %.4f (0.25 +- %.4f)" % (freq.min(), freq.max(), 5 * sigma))
    assert np.abs(freq - 0.25).max() <= 5 * sigma
    z, _, n = run_presence(gh.uniform_u(6, B, HW), 0.5)
    pi = 0.5 ** np.arange(HW + 1)
    pi /= pi.sum()
    hist = np.bincount(n, minlength=HW + 1) / B
    dev = np.abs(hist - pi) / np.sqrt(pi * (1 - pi) / B)
    print("geometric prior, p = 0.5: histogram of n_present within %.2f sigma of p^k / sum p^k" % dev.max())
    assert dev.max() <= 5


# ---- 5. repeatability ------------------------------------------------------------------------------------------------------------------------
def test_sampler_is_repeatable():
    for HW, B, p, count in ((129, 37, 0.999999, None), (1024, 9, 0.5, None), (300, 6, 0.5, 150)):
        u = gh.uniform_u(HW, B, HW)
        a, b = run_presence(u, p, count), run_presence(u, p, count)
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


# ---- the Gaussian maps and the model ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cfg():
    from spair_pytorch_amd import config as cfg
    old = (list(cfg.INPUT_IMAGE_SHAPE), [t["stride"] for t in cfg.DEFAULT_BACKBONE_TOPOLOGY])
    yield cfg
    cfg.INPUT_IMAGE_SHAPE[:] = old[0]
    for t, s in zip(cfg.DEFAULT_BACKBONE_TOPOLOGY, old[1]):
        t["stride"] = s


MODELS = {"g6_f32": (1, 48, 48, "f32"), "g6_bf16": (1, 48, 48, "bf16"), "rect_f32": (1, 48, 80, "f32"), "rgb_bf16": (3, 48, 48, "bf16")}


def make_model(name, cfg, seed=3):
    from spair_pytorch_amd.models import SPAIR
    C, H, W, dtype = MODELS[name]
    cfg.INPUT_IMAGE_SHAPE[0] = C
    cfg.set_grid(H, (2, 2, 2, 1, 1, 1), image_width=W)
    torch.manual_seed(seed)
    return SPAIR([C, H, W], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")


def made_noise(seed, B, A, G, Gw):
    """Noise maps whose first three samples hold eps = 0 (the prior mean), +40 and -40 (clamp10 acts)."""
    rng = np.random.default_rng(seed)
    n = dict(eps_box=rng.standard_normal((B, 4, G, Gw)), eps_attr=rng.standard_normal((B, A, G, Gw)),
             eps_depth=rng.standard_normal((B, 1, G, Gw)))
    for v in n.values():
        v[0], v[1], v[2] = 0.0, 40.0, -40.0
    n = {k: v.astype(np.float32) for k, v in n.items()}
    n["u_pres"] = gh.uniform_u(seed + 1, B, G * Gw).reshape(B, 1, G, Gw)
    return n


def same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("z_where", "z_what", "z_depth", "z_pres", "p_z", "count", "recon", "boxes"))


@pytest.mark.parametrize("name", list(MODELS))
def test_generate_on_a_model(name, cfg):
    from spair_pytorch_amd.models import DIST_NAMES
    m = make_model(name, cfg)
    C, H, W, _ = MODELS[name]
    B, A = 5, int(cfg.N_ATTRIBUTES)
    G, Gw = H // 8, W // 8
    HW = G * Gw
    noise = made_noise(21, B, A, G, Gw)
    dn = {k: torch.from_numpy(v).cuda() for k, v in noise.items()}
    step = 7001
    r = m.generate(B, step, noise=dn)
    assert tuple(r.z_where.shape) == (B, 4, G, Gw) and tuple(r.z_what.shape) == (B, A, G, Gw) and tuple(r.recon.shape) == (B, C, H, W)
    assert tuple(r.p_z.shape) == (B, 1, G, Gw) and r.count.dtype == torch.int32 and r.layers is None and r.layer_weight is None
    # the Gaussian maps against float64, at the bound of their operands
    priors = [cfg.PRIORS[n] for n in DIST_NAMES]
    hyper = dict(min_yx=float(cfg.MIN_YX), max_yx=float(cfg.MAX_YX), min_hw=float(cfg.MIN_HW), max_hw=float(cfg.MAX_HW),
                 anchor=float(cfg.ANCHORBOX_SHAPE[0]), cell_px=int(m.pixels_per_cell[0]), I=H, Iw=W)
    ref = gh.gauss_float64(noise["eps_box"], noise["eps_attr"], noise["eps_depth"], priors, hyper)
    bound = gh.gauss_bounds(noise["eps_box"], noise["eps_attr"], noise["eps_depth"], priors, hyper)
    for what, got, want, E in zip(("z_where", "z_what", "z_depth"), (r.z_where, r.z_what, r.z_depth), ref, bound):
        err = np.abs(got.double().cpu().numpy() - want)
        frac = (err[E > 0] / E[E > 0]).max()                  # (z_what at eps = 0 with a zero prior mean: error and bound are both 0)
        print("%s %s: largest error %.3g, largest fraction of its bound %.3f" % (name, what, err.max(), frac))
        assert (err <= E).all(), (what, frac)
    assert torch.equal(r.z_what[0], torch.full_like(r.z_what[0], float(priors[4][0])))      # eps = 0: the prior mean itself
    assert float((r.z_depth[1] - 4 / (1 + np.exp(-10.0))).abs().max()) <= 1e-6      # clamp10 acts at +40 ...
    assert 1.8e-4 < float(r.z_depth[2].min()) and float(r.z_depth[2].max()) < 1.83e-4      # ... and at -40: 4 sigmoid(-10)
    # presence: the sampler's rule on the model's schedule, hard, counted
    from spair_pytorch_amd.models import step_scalars
    p = step_scalars(step, B).count_prior_prob
    z = r.z_pres.cpu().numpy().reshape(B, HW)
    gh.check_presence_rule(noise["u_pres"].reshape(B, HW), z, r.p_z.cpu().numpy().reshape(B, HW), r.count.cpu().numpy(),
                           gh.presence_float64(HW, B, prob=p, z=z)[1], name)
    # repeatable; a scene for compose; layers as compose gives them
    status = m._status_dev.clone()
    assert same(m.generate(B, step, noise=dn), r)
    assert torch.equal(m.compose(r).recon, r.recon)
    cells = torch.tensor([[0, 7, HW - 1, -1]] * B, device="cuda")
    rl = m.generate(B, step, noise=dn, layers=cells)
    cl = m.compose(r, layers=cells)
    assert same(rl, r) and torch.equal(rl.layers, cl.layers) and torch.equal(rl.layer_weight, cl.layer_weight)
    assert tuple(rl.layers.shape) == (B, 4, C, H, W)
    # seeds and generators
    torch.manual_seed(123)
    before = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    s7 = m.generate(B, step, seed=7)
    assert same(m.generate(B, step, seed=7), s7) and not torch.equal(m.generate(B, step, seed=8).z_what, s7.z_what)
    assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(), before[1])
    a = m.generate(B, step)
    assert not torch.equal(torch.get_rng_state(), before[0])           # seed=None draws its seed from the CPU generator
    torch.manual_seed(123)
    assert same(m.generate(B, step), a)
    assert torch.isfinite(a.recon).all() and float(a.z_pres.min()) >= 0 and set(a.z_pres.unique().tolist()) <= {0.0, 1.0}
    assert torch.equal(a.z_pres.sum((1, 2, 3)).to(torch.int32), a.count)
    # an exact count
    c3 = m.generate(B, step, count=3, seed=5)
    assert (c3.count == 3).all() and torch.equal(c3.z_pres.sum((1, 2, 3)), torch.full((B,), 3.0, device="cuda"))
    ct = torch.tensor([0, 1, HW, HW + 9, -2], device="cuda")
    cm = m.generate(B, 0, count=ct, seed=5)
    assert cm.count.tolist() == [0, 1, HW, HW, 0] and torch.equal(cm.z_what, c3.z_what)
    # nothing above wrote the step-status word
    assert torch.equal(m._status_dev, status) and m.step_status() == 0 and m._status_host[0] == 0


def small_batch(seed=1, B=8):
    return torch.from_numpy(gi.make_image(seed, B, 48, 3)).cuda()


def test_generate_between_steps_leaves_the_bf16_training_run_alone(cfg):
    from spair_pytorch_amd.optim import FusedAdam
    x = small_batch(1)

    def train(with_generate):
        m = make_model("g6_bf16", cfg)
        opt = FusedAdam(m, lr=1e-3)
        torch.manual_seed(11)
        for it in range(10):
            opt.zero_grad()
            m(x, 2000 + it)[0].backward()
            if with_generate and it % 2:      # between backward() and the optimizer step too
                m.generate(8, 2000 + it, seed=it)
            opt.step()
            if with_generate:
                before = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
                m.generate(8, 2000 + it, seed=100 + it, count=it)
                assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(), before[1])
        assert m.step_status() == 0 and opt.skipped() == (0, False)
        return m.flat_parameters().cpu().numpy()

    assert np.array_equal(train(False), train(True))


def test_generate_leaves_a_set_status_word_alone(cfg):
    """As test_compose_gpu.py does for compose: a NaN in one bias of the attribute encoder makes that step's Gaussian KL term NaN and sets
    the step's flag (no GPU fault is involved); generate between backward() and FusedAdam.step() neither clears it nor raises."""
    from spair_pytorch_amd.optim import FusedAdam
    m = make_model("g6_bf16", cfg)
    opt = FusedAdam(m, lr=1e-3)
    x = small_batch()
    bias = dict(m.named_parameters())["object_encoder.out.bias"]
    keep = bias.detach().clone()
    with torch.no_grad():
        bias[3] = float("nan")
    opt.zero_grad()
    m(x, 2000)[0].backward()
    word = m._status_dev.clone()
    r = m.generate(8, 2000, seed=1)
    assert torch.equal(m._status_dev, word) and int(word[0]) & 2
    assert torch.isfinite(r.recon).all()
    opt.step()
    assert opt.skipped()[0] == 1
    with torch.no_grad():
        bias.copy_(keep)
    m.clear_step_status()
    assert m.step_status() == 0


def test_backward_through_a_forward_that_generate_overwrote_raises(cfg):
    from spair_pytorch_amd._lib import SpairHipError
    m = make_model("g6_bf16", cfg)
    x = small_batch()
    loss = m(x, 1001)[0]
    m.generate(8, 1001, seed=2)
    with pytest.raises(SpairHipError, match="overwritten"):
        loss.backward()


def test_argument_errors(cfg):
    from spair_pytorch_amd._lib import SpairHipError
    m = make_model("g6_f32", cfg)
    B, A = 4, int(cfg.N_ATTRIBUTES)
    good = {k: torch.from_numpy(v).cuda() for k, v in made_noise(3, B, A, 6, 6).items()}
    m.generate(B, noise=good)
    m.generate(B, noise={k: v.cpu() for k, v in good.items()})                 # moved to the device, as forward does
    for k, bad in (("eps_attr", good["eps_attr"][:, :49]), ("u_pres", good["u_pres"][:2]), ("eps_box", good["eps_box"][:, :, :5])):
        with pytest.raises(AssertionError):
            m.generate(B, noise=dict(good, **{k: bad}))
    with pytest.raises(KeyError):
        m.generate(B, noise={k: good[k] for k in NOISE[:3]})
    with pytest.raises(AssertionError):
        m.generate(B, count=torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(AssertionError):
        m.generate(B, count=torch.zeros(B, device="cuda"))                      # a float tensor
    with pytest.raises(SpairHipError):
        m.generate(B, count=torch.zeros(B, dtype=torch.int64))                  # on the host
    with pytest.raises(AssertionError):
        m.generate(B, seed=1, layers=torch.zeros(3, 8, dtype=torch.int64, device="cuda"))
    with pytest.raises(SpairHipError):
        m.generate(B, seed=1, layers=torch.zeros(B, 8, dtype=torch.int64))
    with pytest.raises(AssertionError):
        m.generate(0)


def test_generate_at_the_benchmark_geometry(cfg):
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(128, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(3)
    m = SPAIR([1, 128, 128], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
    B = 256
    r = m.generate(B, 0, seed=9)
    assert tuple(r.recon.shape) == (B, 1, 128, 128) and tuple(r.z_pres.shape) == (B, 1, 16, 16)
    for v in (r.recon, r.z_where, r.z_what, r.z_depth, r.p_z):
        assert torch.isfinite(v).all()
    assert torch.equal(r.z_pres.sum((1, 2, 3)).to(torch.int32), r.count)
    n = r.count.float()
    # step 0: the count prior is almost flat over 0 .. 256 -- mean 128, standard deviation 74; the mean of 256 samples within 5 sigma
    assert abs(float(n.mean()) - 128) <= 5 * 74.2 / 16 and float(r.p_z.min()) >= 0 and float(r.p_z.max()) <= 1
    late = m.generate(B, 100000, seed=9, count=torch.arange(B, device="cuda"))
    assert torch.equal(late.count, torch.arange(B, device="cuda", dtype=torch.int32))
    assert same(m.generate(B, 0, seed=9), r) and torch.equal(m.compose(r).recon, r.recon)
    assert m.step_status() == 0
