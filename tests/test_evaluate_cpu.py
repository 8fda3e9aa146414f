"""SPAIR.evaluate without a GPU: the float64 restatement of its definition (evaluate_helpers.terms_float64) against the oracle's KL maps and
torch's BCE on the fixtures' float64 operands, the batch identities against the fixtures' stored scalars, the margin condition of the
fixtures the GPU tests use, the public names, and what the two entry points refuse before any launch.

(The oracle's compute_kl takes square grids only.  On rect_h48w80_b4_step1001 the Gaussian maps are compared against its formula applied to
the 6 x 10 maps directly and the count prior's p_z comes from generate_helpers.presence_float64, which test_generate_cpu.py pins to the
oracle; the batch identities against the reference's own stored scalars hold there as everywhere.)"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import evaluate_helpers as eh
from oracle import spair_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE = 0, -1


@pytest.mark.parametrize("name", eh.FIXTURES)
def test_float64_restatement_is_the_oracle_and_the_batch_identities_hold(name):
    o, pz, (terms, kl_map, bce_map) = eh.fixture_reference(name)
    B, HW, G, Gw = o["B"], o["HW"], o["G"], o["Gw"]
    ocfg = orc.OracleConfig(image_shape=(1, 8 * G, 8 * G))
    maps = lambda v: torch.from_numpy(np.ascontiguousarray(v.transpose(0, 2, 1))).view(B, -1, G, Gw)
    dist = {n: (maps(o["mu"][j]), maps(o["sd"][j])) for j, n in enumerate(eh.NAMES)}
    zp = torch.from_numpy(o["z"]).view(B, 1, G, Gw)
    if G == Gw:
        kl = orc.compute_kl(dist, zp, o["step"], ocfg)
    else:       # the oracle's Gaussian formula on the rectangular maps; its count prior through the pinned helper
        kl = {}
        for n, (mu, sigma) in dist.items():
            m, s = ocfg.priors[n]
            kl[n] = zp * (0.5 * ((sigma / s) ** 2 + ((mu - m) / s) ** 2 - 1 - ((sigma / s) ** 2).log()))
        p = torch.from_numpy(pz).view(B, 1, G, Gw)
        kl["pres_dist"] = zp * (torch.log(zp + 1e-9) - torch.log(p + 1e-9)) + (1 - zp) * (torch.log(1 - zp + 1e-9) - torch.log(1 - p + 1e-9))
    assert [float(ocfg.priors[n][0]) for n in eh.NAMES] == [m for m, _ in eh.config_priors()]
    assert [float(ocfg.priors[n][1]) for n in eh.NAMES] == [s for _, s in eh.config_priors()]
    for j, n in enumerate(eh.NAMES + ("pres_dist",)):
        per_cell = kl[n].sum(dim=1).reshape(B, HW).numpy()
        assert np.abs(kl_map[:, j] - per_cell).max() <= 1e-12 * (1 + np.abs(per_cell).max()), n
        per_sample = kl[n].reshape(B, -1).sum(dim=1).numpy()
        assert np.abs(terms[:, 2 + j] - per_sample).max() <= 1e-12 * (1 + np.abs(per_sample).max()), n
    recon, x = torch.from_numpy(o["recon"]), torch.from_numpy(o["x"])
    bce = np.array([float(F.binary_cross_entropy(recon[b], x[b], reduction="sum")) for b in range(B)])
    assert np.abs(terms[:, 1] - bce).max() <= 1e-12 * bce.max()
    per_px = F.binary_cross_entropy(recon, x, reduction="none").sum(dim=1).numpy()
    assert np.abs(bce_map - per_px).max() <= 1e-12 * (1 + per_px.max())
    assert np.abs(terms[:, 0] - (terms[:, 1] + terms[:, 2:].sum(axis=1))).max() <= 1e-12 * np.abs(terms[:, 0]).max()
    # the batch scalars the reference stored (fp32): BCE summed over the batch, each KL divided by B
    z = o["npz"]
    got, want = terms[:, 1].sum(), float(z["recon_loss"])
    print("%s: recon_loss %.9g against %.9g" % (name, got, want))
    assert abs(got - want) <= eh.BCE_TOL * abs(want)
    for j, n in enumerate(eh.NAMES + ("pres_dist",)):
        got, want = terms[:, 2 + j].sum() / B, float(z["kl_" + n])
        print("%s: kl_%s %.9g against %.9g" % (name, n, got, want))
        assert abs(got - want) <= eh.KL_TOL * abs(want), n


def test_margin_condition_of_the_fixtures():
    """Every z_pres of the GPU tests' fixtures lies more than 2e-4 from 0.5: under the fp32 step's latent bound (1e-4) the hard decision
    inside the count prior cannot flip.  The two fixtures that fail it are not used."""
    worst = {}
    for name in eh.FIXTURES + ("c1_b16_step1", "t_feat64"):
        z = np.load(os.path.join(eh.ph.GOLDEN, name + ".npz"))["z_pres"].astype(np.float64)
        worst[name] = float(np.abs(z - 0.5).min())
    print(", ".join("%s %.2g" % kv for kv in worst.items()))
    for name in eh.FIXTURES:
        assert worst[name] > eh.MARGIN, (name, worst[name])
    assert worst["c1_b16_step1"] < eh.MARGIN and worst["t_feat64"] < eh.MARGIN
    assert "c1_b16_step1" not in eh.FIXTURES and "t_feat64" not in eh.FIXTURES


@pytest.mark.parametrize("spec", eh.UNIT_CASES)
def test_bound_is_small_against_the_terms_and_a_dropped_addend_exceeds_it(spec, lib):
    """The derived bound on the GPU tests' made-up operands: far below the project's comparison bounds relative to each term, and several
    times smaller than the one pixel, one cell or one attribute element those tests take out of the reference."""
    seed, B, HW, A, C, I, Iw, permute = spec
    c = eh.make_unit_case(seed, B, HW, A, C, I, Iw, permute)
    pri = eh.config_priors()
    S = lib.spair_sample_terms_scratch_floats(B, HW, I, Iw) // (8 * B)
    terms, kl_map, bce_map = eh.terms_float64(c["z"], c["pz"], c["mu"], c["sd"], pri, 0.75, c["recon"], c["x"])
    E_t, E_kl, E_bce = eh.fp32_bounds(c["z"], c["pz"], c["mu"], c["sd"], pri, 0.75, c["recon"], c["x"], slices=S)
    assert (E_t[:, 1:] <= 1e-5 * np.abs(terms[:, 1:]) + 1e-5).all()
    b = B - 1
    g = eh._pieces(c["z"], c["pz"], c["mu"], c["sd"], pri, c["recon"], c["x"])[0]
    print("unit %d: S %d, dropped pixel %.3g (bound %.3g), cell %.3g (%.3g), attribute element %.3g (%.3g)"
          % (seed, S, bce_map[b].max(), E_t[b, 1], np.abs(kl_map[b, 6]).max(), E_t[b, 8], np.abs(g[4][b]).max(), E_t[b, 6]))
    assert bce_map[b].max() > 4 * E_t[b, 1] and np.abs(kl_map[b, 6]).max() > 4 * E_t[b, 8] and np.abs(g[4][b]).max() > 4 * E_t[b, 6]


def test_evaluate_is_exported():
    import spair_pytorch_amd as sp
    from spair_pytorch_amd import _lib, models
    assert sp.EvalResult is models.EvalResult and callable(sp.SPAIR.evaluate) and "EvalResult" in sp.__all__ and "ParseResult" in sp.__all__
    assert sp.EvalResult.__slots__ == ("loss", "terms", "terms_draws", "kl_map", "bce_map", "recon", "z_where", "z_pres", "loss_terms")
    doc = sp.SPAIR.evaluate.__doc__
    for word in ("PER IMAGE", "no_grad", "NO torch generator", "FusedAdam.step()", "backward()", "generation", "world_size", "seed + k",
                 "posterior mean", "maps=False"):
        assert word in doc, word
    header = open(os.path.join(ROOT, "include", "spair_hip.h")).read()
    source = open(_lib.__file__).read()
    for fn in ("spair_sample_terms_rows", "spair_eval_terms"):
        assert "int %s(" % fn in header and fn in source
    assert "#define SPAIR_ABI_VERSION 3" in header and _lib.ABI_VERSION == 3
    assert callable(_lib.sample_terms) and callable(_lib._declare_evaluate)
    if os.path.exists(_lib.LIB_PATH):
        h = _lib.lib()
        for fn in ("spair_sample_terms_rows", "spair_eval_terms", "spair_sample_terms_scratch_floats"):
            assert hasattr(h, fn)


@pytest.fixture(scope="module")
def lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def rows_call(lib, B=2, HW=16, A=50, C=1, I=32, Iw=32, null=(), lds=None, priors=True):
    """(the non-NULL pointers are never read: every call here returns from the checks before the launch)"""
    vp = lambda name: None if name in null else ctypes.c_void_p(64)
    ld = dict(z=56, pz=16, mu_box=16, sd_box=16, mu_attr=104, sd_attr=56, mu_depth=16, sd_depth=16)
    ld.update(lds or {})
    ops = []
    for n in ("z", "pz", "mu_box", "sd_box", "mu_attr", "sd_attr", "mu_depth", "sd_depth"):
        ops += [vp(n), ld[n]]
    pm = (ctypes.c_float * 6)(0, 0, 7, 7, 0, 0)
    ps = (ctypes.c_float * 6)(1, 1, 0.5, 0.5, 1, 1)
    pr = lambda a, name: None if name in null else ctypes.cast(a, ctypes.c_void_p)
    return lib.spair_sample_terms_rows(*ops, vp("cidx"), pr(pm, "prior_mean"), pr(ps, "prior_std"), 1.0, vp("recon"), vp("x"), B, HW, A, C,
                                       I, Iw, vp("terms"), vp("kl_map"), vp("bce_map"), vp("scratch"), 0, 1.0, None)


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-3), dict(HW=0), dict(HW=-1), dict(HW=1025), dict(A=60), dict(A=0), dict(C=0), dict(I=0),
                                dict(Iw=0), dict(I=-4)] +
                         [dict(null=(n,)) for n in ("z", "pz", "mu_box", "sd_box", "mu_attr", "sd_attr", "mu_depth", "sd_depth", "prior_mean",
                                                    "prior_std", "recon", "x", "terms", "scratch")] +
                         [dict(lds=dict(mu_attr=49)), dict(lds=dict(sd_box=3)), dict(lds=dict(z=0))])
def test_sample_terms_rows_refusals(lib, kw):
    assert rows_call(lib, **kw) == ERR_SHAPE


def test_scratch_size_follows_the_shape_alone(lib):
    f = lib.spair_sample_terms_scratch_floats
    assert f(256, 256, 128, 128) == 256 * 8 * 8            # 2048 workgroups: eight per sample
    assert f(1, 1024, 256, 256) == 1 * 256 * 8             # one sample: the cap of 256 workgroups
    assert f(1, 1, 1, 1) == 8 and f(5, 64, 1, 1) == 5 * 16 * 8     # never more workgroups than rows / 4
    assert f(0, 16, 8, 8) == ERR_SHAPE and f(1, 1025, 8, 8) == ERR_SHAPE and f(1, 16, 0, 8) == ERR_SHAPE


def test_eval_terms_refusals(lib):
    from spair_pytorch_amd import _lib
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.models import make_dims
    topo = [dict(t) for t in cfg.DEFAULT_BACKBONE_TOPOLOGY]
    for t, s in zip(topo, (2, 2, 2, 1, 1, 1)):
        t["stride"] = s

    def call(d, null=(), **kw):
        vp = lambda name: None if name in null else ctypes.c_void_p(64)
        return lib.spair_eval_terms(None if "d" in null else ctypes.byref(d), vp("workspace"), 0, vp("x"), vp("recon"), 1.0, vp("terms"),
                                    vp("kl_map"), vp("bce_map"), vp("scratch"), 0, 1.0, None)

    good = lambda: make_dims(2, [1, 48, 48], topo, "f32")
    for n in ("d", "workspace", "x", "recon", "terms", "scratch"):
        assert call(good(), null=(n,)) == ERR_SHAPE, n
    for field, v in (("B", 0), ("B", -2), ("A", 60), ("A", 0), ("I", 0), ("I", -1), ("G", 0), ("G", 33)):
        d = good()
        setattr(d, field, v)
        assert call(d) == ERR_SHAPE, (field, v)
    d = good()
    d.Iw = -5
    assert call(d) == ERR_SHAPE
