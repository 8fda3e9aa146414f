"""The directed inputs of tests/latent_edges.py on the reference alone: that they reach the clamps they are meant to reach, that the
reference is well conditioned there (fp32 oracle against float64 oracle), and that the assertions test_latent_edges_gpu.py applies to the
HIP step reject a reference whose clamps are missing (no kernel is mutated: the oracle is, by monkeypatching).

Measured (fp32 oracle / float64 oracle, 6 x 6 cells, B = 4; 8,784 clamp inputs per step):
  L-std + L-pres + N-eps: 3,640 clamp inputs outside +-10, one within 0.05 (a presence logit at 0.035); presence logits -12.8 .. 22.9,
    40 of 144 outside, 9 within 0.5 of +-10.  fp32 against float64: worst cell 0.09 of the f32 bound, whole maps <= 9.6e-5, loss 5.8e-8,
    exact-zero patterns identical.
  N-eps alone: 480 outside, none nearer than 7.2.  Worst cell 0.17 of the f32 bound (d recon term / d depth latents), whole maps <= 5.8e-5.
  L-std + N-eps, forward: z_where 1.35e-7, depth 2.4e-7, z_pres 7.0e-8 (latent_edges.SPREAD takes the larger of this and N-u).
  N-u: z_where 1.1e-7, depth 3.45e-7, z_pres 7.0e-8, loss 3.5e-8 relative; the fp32 oracle rounds 48 z_pres values (every u = 1 cell) to
    exactly 1.0, the float64 oracle none.
  Under bf16 operands (float64 oracle on the operands the bf16 step reads against the float64 oracle; test_latent_edges_gpu.py's docstring has
    the whole table): L-std + L-pres + N-eps moves the loss by 1.4e-3, 5.8 times the bf16 step's loss bound; d z_pres term / d box latents
    leaves its cell bound in either regime (4.6 and 1.15 of it).  The figures move by a few percent from run to run (threaded float64
    sums decide bf16 roundings), which is why latent_edges.BF16_WIDENED states them 10 % high and this test holds them in a window.
"""
import pytest
import torch

import latent_edges as le

MODES = ("loss", "z_where", "recon")


def pair(regimes, targets):
    return le.oracle_run(regimes, "f32", targets), le.oracle_run(regimes, "f64", targets)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_directed_inputs_reach_the_clamps_on_the_reference(dtype):
    """The caps and counts the GPU test asserts on the kernel's latents hold on the oracle's, and its zero / non-zero assertions hold on the
    oracle's gradients (so a failure on the GPU is the kernel's)."""
    r = le.oracle_run(le.ALL, dtype, le.TARGETS)
    ci = le.clamp_inputs(r["latents"], r["noise"])
    assert le.band_share(ci) <= le.MAX_BAND_SHARE
    # L-pres, with the reference-side band of 0.5: both sides of the clamp populated, few logits near it
    lg = ci["logit"]
    n_off, n_open = int(le.off(lg, le.PRES_BAND).sum()), int(le.opn(lg, le.PRES_BAND).sum())
    assert n_off >= le.MIN_COUNT and n_open >= le.MIN_COUNT and lg.numel() - n_off - n_open <= le.MAX_BAND_SHARE * lg.numel(), (n_off, n_open)
    assert int((lg > 10).sum()) >= 10 and int((lg < -10).sum()) >= 1      # (measured: 38 above +10, 2 below -10)
    for mode in MODES:
        failures, counts = le.zero_mask_report(r["grads"][mode], ci, mode)
        print(dtype, mode, counts)
        assert not failures, failures
    # N-eps alone: two thirds of the box and depth logits far outside, everything else far inside
    r = le.oracle_run(("N-eps",), dtype, le.TARGETS)
    ci = le.clamp_inputs(r["latents"], r["noise"])
    assert sum(int((v.abs() > 10).sum()) for v in ci.values()) == 480
    assert min(float((v.abs() - 10).abs().min()) for v in ci.values()) > 7
    for mode in ("z_where", "recon"):
        failures, counts = le.zero_mask_report(r["grads"][mode], ci, mode)
        failures = [f for f in failures if not f.startswith("presence logit")]      # (no presence logit leaves +-0.3 without L-pres)
        assert not failures, failures


@pytest.mark.parametrize("regimes", [le.ALL, ("N-eps",)], ids=["L-std+L-pres+N-eps", "N-eps"])
def test_reference_is_well_conditioned_in_the_clamps(regimes):
    """fp32 oracle against float64 oracle: every per-cell latent gradient within 0.25 of the f32 step's bound, the same exact zeros."""
    a, b = pair(regimes, le.TARGETS)
    cell_tol, floor_tol, map_tol, loss_tol = le.F32_BOUNDS
    assert abs(a["loss"] - b["loss"]) <= 0.25 * loss_tol * abs(b["loss"])
    for t in le.TARGETS:
        for n in le.NAMES:
            ga, gb = a["grads"][t][n], b["grads"][t][n]
            worst, whole = le.cell_errors(ga, gb, cell_tol, floor_tol)
            print("%s d %s: worst cell %.3f of the f32 bound, whole map %.2e" % (n, t, worst, whole))
            assert worst <= 0.25 and whole <= 0.25 * map_tol, (t, n, worst, whole)
            assert torch.equal(ga == 0, gb == 0), (t, n)


def test_forward_spread_of_the_reference():
    """latent_edges.SPREAD is the reference's own fp32-versus-float64 spread (not below it, not more than 3 x above it), and the forward
    bound derived from it sees a missing clamp."""
    a, b = pair(("L-std", "N-eps"), ("loss",))
    c, d = pair(("N-u",), ("loss",))
    for k in ("z_where", "z_depth", "z_pres"):
        spread = max(float((a[k] - b[k]).abs().max()), float((c[k] - d[k]).abs().max()))
        print(k, spread)
        assert spread <= le.SPREAD[k] <= 3 * spread, (k, spread)
    effect = le.missing_clamp_effect(48)
    for k in ("z_where", "z_depth"):
        assert le.FWD_FACTOR * le.SPREAD[k] < effect[k] / 3, k
    # N-u: the two oracles' losses agree to less than one fp32 unit of the loss (6e-8), which is resolution, not spread: the loss bound
    # stands on the 1.2e-6 the fp32 oracle has been seen to differ by, and the measured value must not exceed it
    assert abs(c["loss"] - d["loss"]) <= le.SPREAD["loss_nu"] * abs(d["loss"])
    assert int((c["z_pres"] == 1).sum()) > 0 and int((d["z_pres"] == 1).sum()) == 0      # (why no per-cell gradient bound is set under N-u)
    u = c["noise"]["u_pres"]
    assert float(u.min()) == 2.0 ** -25 and float(u.max()) == 1.0 and int((u == 1.0 - 2.0 ** -24).sum()) == 1


@pytest.mark.parametrize("mutation", ["no_sigmoid_clamps", "no_presence_clamp"])
def test_assertions_reject_a_reference_without_its_clamps(mutation):
    """A float64 oracle whose clamped_sigmoid / latent_to_mean_std do not clamp, or whose presence logit is not clamped (float64: without
    the clamp a -60 box is 1e-52 wide, which fp32 cannot render), must fail the zero-mask assertions -- applied to its own taps -- in every
    mode, and, for the sigmoids, the forward bound."""
    r = le.oracle_run(le.ALL, "f64", MODES, mutation=mutation)
    ci = le.clamp_inputs(r["latents"], r["noise"])
    want = {"no_sigmoid_clamps": {"loss": ("box log-std", "encoder log-std", "depth log-std"), "z_where": ("box mean", "box log-std"),
                                  "recon": ("box mean", "box log-std", "depth latents")},
            "no_presence_clamp": {m: ("presence logit",) for m in MODES}}[mutation]
    for mode in MODES:
        failures, _ = le.zero_mask_report(r["grads"][mode], ci, mode)
        print(mutation, mode, failures)
        for name in want[mode]:
            assert any(f.startswith(name) and "not exactly 0" in f for f in failures), (mode, name, failures)
    if mutation == "no_sigmoid_clamps":
        a = le.oracle_run(("L-std", "N-eps"), "f64", ("loss",), mutation=mutation)
        b = le.oracle_run(("L-std", "N-eps"), "f64", ("loss",))
        for k in ("z_where", "z_depth"):
            assert float((a[k] - b[k]).abs().max()) > le.FWD_FACTOR * le.SPREAD[k], k


def test_assertions_reject_a_reference_clamped_at_5():
    """The non-zero side: with the sigmoids' clamps at +-5 the log-stds moved to +-8 by L-std lose their gradient, and the whole-loss
    assertions must say so."""
    r = le.oracle_run(le.ALL, "f64", ("loss",), mutation="sigmoid_clamps_at_5")
    failures, _ = le.zero_mask_report(r["grads"]["loss"], le.clamp_inputs(r["latents"], r["noise"]), "loss")
    for name in ("box log-std", "encoder log-std"):
        assert any(f.startswith(name) and "open elements are 0" in f for f in failures), (name, failures)


@pytest.mark.parametrize("regimes", [le.ALL, ("N-eps",)], ids=["L-std+L-pres+N-eps", "N-eps"])
def test_bf16_operand_spread_of_the_reference(regimes):
    """The reference on bf16 operands against itself.  Every figure of latent_edges.BF16_WIDENED -- the spreads behind the few bf16 bounds
    that test_latent_edges_gpu.py sets at 4 x the spread -- is re-measured: not above the stated figure, not below 2/3 of it, and above
    a quarter of the undirected bound it replaces (else the bound would not have needed it).  Every other bf16 bound is the undirected
    one whatever this model says."""
    sp = le.bf16_operand_spread(regimes)
    cell_tol, floor_tol, map_tol, loss_tol = le.BF16_BOUNDS
    for key, stated in le.BF16_WIDENED[regimes].items():
        pairs = [(sp["loss"], stated, loss_tol)] if key == "loss" else [(sp[key][0], stated[0], 1.0), (sp[key][1], stated[1], map_tol)]
        for measured, figure, undirected in pairs:
            print(key, measured, figure)
            if figure is not None:
                assert 2 / 3 * figure <= measured <= figure, (key, measured, figure)
                assert le.SPREAD_MARGIN * figure > undirected, key
    assert set(le.BF16_WIDENED) == {le.ALL, ("N-eps",)}
