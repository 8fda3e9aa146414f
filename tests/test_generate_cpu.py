"""SPAIR.generate without a GPU: the float64 restatement of the sampler (generate_helpers.presence_float64) against the oracle's count
prior, the one-hot recursion of the reference run literally, the margin condition of the GPU tests' seeds on the reference alone, the
public names, and what spair_prior_presence refuses before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import generate_helpers as gh
from oracle import spair_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE = 0, -1


def oracle_prob(step, ocfg):
    return float(1 / ((-orc.exponential_decay(step, **ocfg.count_prior)).exp() + 1))


@pytest.mark.parametrize("step", [0, 1001, 7001])
@pytest.mark.parametrize("G", [4, 11])
def test_teacher_forced_helper_is_the_oracles_count_prior(step, G):
    """oracle.compute_kl is pinned to the reference by test_oracle_golden.py; on a float64 z_pres it runs the recursion in float64."""
    from spair_pytorch_amd.models import step_scalars
    ocfg = orc.OracleConfig(image_shape=(1, 8 * G, 8 * G))
    B, HW = 6, G * G
    rng = np.random.default_rng(100 + G)
    dens = np.array([0.0, 1.0, 0.05, 0.5, 0.8, 0.97])[:, None]
    z = (rng.uniform(size=(B, HW)) < dens).astype(np.float64)
    out = []
    orc.compute_kl({}, torch.from_numpy(z).view(B, 1, G, G), step, ocfg, p_z_out=out)
    ref = out[0].double().numpy().reshape(B, HW)
    prob = oracle_prob(step, ocfg)
    assert prob == step_scalars(step, 1).count_prior_prob      # the schedule generate() reads
    _, pz, n = gh.presence_float64(HW, B, prob=prob, z=z)
    err = np.abs(pz - ref).max()
    print("step %d, G %d: helper against the oracle %.3g" % (step, G, err))
    assert err <= 1e-12 and np.array_equal(n, z.sum(axis=1).astype(np.int64))


@pytest.mark.parametrize("HW", [1, 7, 16])
def test_onehot_recursion_is_need_over_rem_and_keeps_exactly_n(HW):
    rng = np.random.default_rng(HW)
    for n in sorted({0, 1, HW // 2, HW - 1, HW}):
        for u in (gh.uniform_u(HW + n, 1, HW)[0], np.zeros(HW, np.float32), np.full(HW, gh.ONE_BELOW, np.float32), rng.uniform(size=HW)):
            z, pz = gh.onehot_reference_literal(HW, n, u)
            need = n - np.concatenate(([0.0], np.cumsum(z)[:-1]))
            assert np.abs(pz - need / (HW - np.arange(HW))).max() <= 1e-15, (HW, n)
            assert z.sum() == n, (HW, n)
            # the helper (absolute bins from the one-hot start) and the fp32 closed form take the same decisions
            zh, pzh, nh = gh.presence_float64(HW, 1, count=n, u=np.asarray(u)[None, :])
            assert np.array_equal(zh[0], z) and np.abs(pzh[0] - pz).max() <= 1e-15 and nh[0] == n
    u = gh.uniform_u(3, 4, HW)
    z32, pz32, n32 = gh.exact_count_fp32(HW, [-3, HW + 7, HW // 2, 1], u)
    assert list(n32) == [0, HW, HW // 2, min(1, HW)]
    assert pz32.dtype == np.float32 and pz32.min() >= 0 and pz32.max() <= 1


def test_margin_share_of_the_gpu_cases_on_the_reference_alone():
    """The GPU tests excuse a decision where |u - p_z64| <= 5e-5 and hold the share of such cells to 0.5 %: on the free-running float64
    reference the seeds they use stay under it (expected share: about 1e-4)."""
    worst = 0.0
    for HW in gh.SAMPLER_HW:
        for B in gh.SAMPLER_B:
            for p in gh.SAMPLER_P:
                u = gh.uniform_u(gh.sampler_seed(HW, B, p), B, HW)
                z, pz, n = gh.presence_float64(HW, B, prob=p, u=u)
                share = (np.abs(u.astype(np.float64) - pz) <= gh.MARGIN).mean()
                worst = max(worst, share)
                assert share <= gh.MARGIN_SHARE, (HW, B, p, share)
    print("largest share of cells inside the margin: %.3g" % worst)


def test_generate_is_exported():
    import spair_pytorch_amd as sp
    from spair_pytorch_amd import _lib, models
    assert sp.GenerateResult is models.GenerateResult and callable(sp.SPAIR.generate) and "GenerateResult" in sp.__all__
    assert sp.GenerateResult.__slots__ == ("z_where", "z_what", "z_depth", "z_pres", "p_z", "count", "recon", "boxes", "layers", "layer_weight")
    doc = sp.SPAIR.generate.__doc__
    for word in ("prior", "HARD", "clamped", "row-major", "NO torch generator", "FusedAdam", "generation", "compose", "count"):
        assert word in doc, word
    header = open(os.path.join(ROOT, "include", "spair_hip.h")).read()
    source = open(_lib.__file__).read()
    for fn in ("spair_prior_presence", "spair_prior_sample"):
        assert "int %s(" % fn in header and fn in source
    assert "#define SPAIR_ABI_VERSION 3" in header and _lib.ABI_VERSION == 3
    assert callable(_lib.prior_presence) and callable(_lib._declare_prior)
    if os.path.exists(_lib.LIB_PATH):
        h = _lib.lib()
        for fn in ("spair_prior_presence", "spair_prior_sample"):
            assert hasattr(h, fn)


@pytest.fixture(scope="module")
def lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def presence(lib, B=2, HW=16, p=0.5, u=64, count=None, z=64, pz=64, n=64):
    """(the non-NULL pointers are never read: every call here returns from the checks before the launch)"""
    vp = lambda a: ctypes.c_void_p(a) if a else None
    return lib.spair_prior_presence(vp(u), B, HW, p, vp(count), vp(z), vp(pz), vp(n), None)


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(HW=0), dict(HW=-4), dict(HW=1025), dict(p=0.0), dict(p=1.0), dict(p=-0.1),
                                dict(p=1.5), dict(p=float("nan")), dict(u=0), dict(z=0), dict(pz=0), dict(n=0),
                                dict(count=64, B=0), dict(count=64, HW=1025), dict(count=64, u=0), dict(count=64, n=0)])
def test_prior_presence_refusals(lib, kw):
    assert presence(lib, **kw) == ERR_SHAPE


def test_prior_sample_refuses_null_operands(lib):
    from spair_pytorch_amd import _lib
    d = _lib.SpairDims()
    d.B, d.G, d.A, d.I, d.cell_px = 2, 4, 50, 32, 8
    p = [ctypes.c_void_p(64)] * 10
    assert lib.spair_prior_sample(None, 0.5, None, *p, None) == ERR_SHAPE
    for k in range(10):
        q = list(p)
        q[k] = None
        assert lib.spair_prior_sample(ctypes.byref(d), 0.5, None, *q, None) == ERR_SHAPE
    assert lib.spair_prior_sample(ctypes.byref(d), 1.0, None, *p, None) == ERR_SHAPE
    d.G = 33                                                          # 33 x 33 cells > 1024
    assert lib.spair_prior_sample(ctypes.byref(d), 0.5, None, *p, None) == ERR_SHAPE
    d.G, d.B = 4, 0
    assert lib.spair_prior_sample(ctypes.byref(d), 0.5, None, *p, None) == ERR_SHAPE
