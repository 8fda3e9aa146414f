"""The training step on other backbone topologies and network sizes (golden_inputs.TOPO_CASES, ORACLE_CASES) against fixtures produced by the
reference itself (tests/golden/t_*.npz, make_golden.py) -- and, for N_ATTRIBUTES != 50, which the reference cannot run (its models.py:66,167
write 55 context channels out), against the CPU oracle, which tests/test_oracle_golden.py pins to the reference on every t_* fixture.

tests/test_topology_cpu.py pins which kernels each case runs (the weight packs of T = k / s = 3 and 1, tap-parity order at cin = 64, 1x1
stacks of 2 and 3 layers, a 1x1 layer outside the stack, conv_out alone, the stem's weight gradient inside a k = 6 conv_1's data gradient, a
patch data gradient gated by the stored activation, the per-wavefront bf16 path behind the patch-resident backbone, k_gauss_kl at 64 lanes);
tests/test_step_operands_gpu.py says which kernel is wrong when a comparison here fails.  Every test is one step of B <= 4, I <= 48."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from helpers import assert_fp32_step_matches, build_model, engine_config, expected_of

pytestmark = pytest.mark.gpu

CHAIN_CASES = ("t_shallow64", "t_k3", "t_k6", "t_nostack", "t_deep8", "t_stack5", "t_stem5")      # (tests/test_topology_cpu.py pins it)


@pytest.mark.parametrize("name", list(gi.TOPO_CASES))
def test_fp32_step_matches_reference(name):
    z, case = expected_of(name)
    with engine_config(case, 0):
        assert_fp32_step_matches(build_model(case, "f32"), z)


@pytest.mark.parametrize("name", list(gi.ORACLE_CASES))
def test_fp32_step_matches_oracle(name):
    """N_ATTRIBUTES = 16 and 59: the same quantities and tolerances, the oracle's fp32 forward and backward as the expected values."""
    z, case = expected_of(name)
    with engine_config(case, 0):
        m = build_model(case, "f32")
        assert m.state_dict()["object_encoder.out.weight"].shape[0] == 2 * case["A"]
        assert_fp32_step_matches(m, z)


# Per-case bounds of the bf16 step, by the convention of tests/test_engine_gpu.py's BF16_BOUNDS: recon and z_where absolute (a [0, 1] image,
# normalised boxes), |g| / |g_ref| - 1 and the cosine per tensor.  Each bound is about 4x the observed deviation, rounded up to 1, 1.5, 2, 3, 5 or
# 8 x 10^n (a norm deviation of 2 % or more gets the 1.6 - 2.5x that table gives its own: 0.018 -> 0.04, 0.049 -> 0.08); the cosine bound is
# the observed minimum less 0.005 (a last-bit change upstream re-rolls every later bf16 rounding and moves a cosine by about 0.002).  The
# loss is not measured: it is held to BASELINE.json's 1e-3 relative (observed 1.1e-5 .. 1.0e-4), and every output must be finite.
# Observed on the MI355X (the bf16 step has no atomics: the figures repeat bit for bit).  Key: (case, SpairStep.flags); flags 1 = the
# per-wavefront cell path, run for the cases whose fused chain is on at flags 0.
# The two cosines near 0.95 were chased, and neither is a kernel's:
#  * t_k3, 0.9524 on backbone.net.conv_3.weight (conv_1 .. conv_3: 0.95 - 0.97), the same on both cell paths and at batch 2, 4 and 16 against
#    the engine's own fp32 step (0.961 / 0.963 / 0.966 / 0.967 on conv_2.bias, conv_1.bias, conv_3.bias, conv_1.weight).  The CPU oracle, all
#    in fp32 with nothing but the backbone's WEIGHTS rounded to bf16, turns its own gradient by the same amounts (0.9609 / 0.9635 / 0.9660 /
#    0.9673 on those four tensors; 0.9977 or better on c1_b8_step1001 and t_k6): this network's backbone gradient is that sensitive to
#    2^-9 in its weights.  tests/test_step_operands_gpu.py (T_k3) holds every kernel of the step to float64 on its stored operands.
#  * t_deep8, 0.9508 on object_decoder.dense0.weight: the cosine of the fixture's 256 sampled elements at batch 2 (72 objects); over the
#    whole tensor against the engine's fp32 step it is 0.987 at batch 2 and above 0.996 at batch 4 and 16 (T_deep8 as above).
BF16_BOUNDS = {
    #                      recon    z_where  norm   cos          observed: recon / z_where / norm / cos (the tensor of the lowest cosine)
    ("t_shallow64", 0):    (0.0015, 8e-05,   0.02,  0.991),    # 3.1e-4 / 1.4e-5 / 0.0046 / 0.9969  z_network.body.dense0.weight
    ("t_k3", 0):           (0.0015, 5e-05,   0.08,  0.947),    # 3.2e-4 / 7.8e-6 / 0.0491 / 0.9524  backbone.net.conv_3.weight (norm: conv_2.bias)
    ("t_k6", 0):           (0.003,  5e-05,   0.03,  0.993),    # 5.3e-4 / 8.2e-6 / 0.0060 / 0.9983  object_encoder.dense0.weight
    ("t_nostack", 0):      (0.003,  5e-05,   0.05,  0.993),    # 5.8e-4 / 7.9e-6 / 0.0092 / 0.9986  object_encoder.dense0.weight
    ("t_deep8", 0):        (0.003,  3e-05,   0.05,  0.945),    # 5.2e-4 / 5.8e-6 / 0.0196 / 0.9508  object_decoder.dense0.weight (norm: conv_0.weight)
    ("t_stack5", 0):       (0.0015, 5e-05,   0.03,  0.993),    # 2.8e-4 / 1.2e-5 / 0.0054 / 0.9988  backbone.net.conv_0.weight
    ("t_stem5", 0):        (0.002,  5e-05,   0.05,  0.989),    # 4.8e-4 / 9.2e-6 / 0.0114 / 0.9942  object_decoder.dense0.weight
    ("t_feat64", 0):       (0.002,  3e-05,   0.05,  0.991),    # 4.9e-4 / 6.9e-6 / 0.0096 / 0.9968  z_network.body.dense0.bias
    ("t_feat128", 0):      (0.002,  2e-05,   0.08,  0.977),    # 4.9e-4 / 4.2e-6 / 0.0334 / 0.9824  object_encoder.dense0.weight (norm: conv_0.bias)
    ("o_attr16", 0):       (0.003,  3e-05,   0.05,  0.990),    # 6.6e-4 / 5.4e-6 / 0.0078 / 0.9951  z_network.body.dense0.weight
    ("o_attr59", 0):       (0.003,  2e-05,   0.05,  0.993),    # 7.5e-4 / 4.4e-6 / 0.0099 / 0.9983  object_encoder.dense0.weight
    ("t_shallow64", 1):    (0.0015, 8e-05,   0.03,  0.992),    # 3.6e-4 / 1.4e-5 / 0.0059 / 0.9970  z_network.body.dense0.weight
    ("t_k3", 1):           (0.0015, 5e-05,   0.08,  0.947),    # 3.2e-4 / 7.6e-6 / 0.0491 / 0.9524  backbone.net.conv_3.weight
    ("t_k6", 1):           (0.003,  5e-05,   0.02,  0.993),    # 5.3e-4 / 8.3e-6 / 0.0040 / 0.9983  object_encoder.dense0.weight
    ("t_nostack", 1):      (0.003,  5e-05,   0.05,  0.993),    # 5.8e-4 / 7.8e-6 / 0.0096 / 0.9986  object_encoder.dense0.weight
    ("t_deep8", 1):        (0.003,  3e-05,   0.05,  0.945),    # 5.2e-4 / 5.7e-6 / 0.0193 / 0.9508  object_decoder.dense0.weight
    ("t_stack5", 1):       (0.0015, 5e-05,   0.02,  0.993),    # 2.8e-4 / 1.2e-5 / 0.0045 / 0.9988  backbone.net.conv_0.weight
    ("t_stem5", 1):        (0.002,  5e-05,   0.05,  0.989),    # 4.8e-4 / 1.1e-5 / 0.0096 / 0.9941  object_decoder.dense0.weight
}
BF16_RUNS = [(n, 0) for n in list(gi.TOPO_CASES) + list(gi.ORACLE_CASES)] + [(n, 1) for n in CHAIN_CASES]


def bf16_figures(name, flags):
    """One bf16 step of a case at SpairStep.flags `flags` against its expected values: the relative loss error, whether everything is finite,
    max |recon - ref|, max |z_where - ref|, and over the parameter tensors the largest | |g| / |g_ref| - 1 | and the smallest cosine (with
    the tensors they belong to), measured as tests/test_engine_gpu.py's bf16 test measures them."""
    z, case = expected_of(name)
    with engine_config(case, flags):
        m = build_model(case, "bf16")
        assert m.step_plan(case["B"])["chain"] == (name in CHAIN_CASES and not flags & 1)
        x = torch.from_numpy(np.asarray(z["x"])).cuda()
        noise = {k: torch.from_numpy(np.asarray(z[k])).cuda() for k in ("eps_box", "eps_attr", "eps_depth", "u_pres")}
        m.zero_grad()
        loss, recon, z_where, z_pres = m(x, int(z["global_step"]), noise=noise)
        loss.backward()
        fig = dict(loss=abs(loss.item() - float(z["loss"])) / abs(float(z["loss"])),
                   finite=all(bool(torch.isfinite(t).all()) for t in (loss, recon, z_where, z_pres, m.loss_terms(), m.flat_gradients())),
                   recon=float(np.abs(recon.cpu().numpy() - z["recon_x"]).max()), z_where=float(np.abs(z_where.cpu().numpy() - z["z_where"]).max()),
                   norm=(0.0, None), cos=(1.0, None))
        for k, p in m.named_parameters():
            if k.startswith("attn."):
                continue
            gn = float(p.grad.double().norm().item())
            ref_n = float(z["gradnorm_" + k])
            dev = max(abs(gn - ref_n) - 1e-5, 0.0) / max(ref_n, 1e-30)
            if dev > fig["norm"][0]:
                fig["norm"] = (dev, k)
            # direction: the full tensor where the expected values hold it, the fixed sample of elements otherwise
            g = p.grad.detach().double().cpu().flatten().numpy()
            if "grad_" + k in z:
                ref = np.asarray(z["grad_" + k], np.float64).flatten()
            else:
                g, ref = g[z["gradidx_" + k]], np.asarray(z["gradsample_" + k], np.float64)
            if np.linalg.norm(ref) > 1e-6 * max(1.0, ref_n):
                cos = float(np.dot(g, ref) / (np.linalg.norm(g) * np.linalg.norm(ref) + 1e-30))
                if cos < fig["cos"][0]:
                    fig["cos"] = (cos, k)
    return fig


@pytest.mark.parametrize("name,flags", BF16_RUNS, ids=["%s-f%d" % r for r in BF16_RUNS])
def test_bf16_step_within_north_star_tolerance(name, flags):
    fig = bf16_figures(name, flags)
    print("\n[bf16 %s flags %d] loss %.2e  recon %.2e  z_where %.2e  norm %.4f (%s)  cos %.4f (%s)"
          % (name, flags, fig["loss"], fig["recon"], fig["z_where"], fig["norm"][0], fig["norm"][1], fig["cos"][0], fig["cos"][1]))
    assert fig["finite"]
    assert fig["loss"] <= 1e-3
    tol_recon, tol_zw, tol_norm, min_cos = BF16_BOUNDS[(name, flags)]
    assert fig["recon"] < tol_recon and fig["z_where"] < tol_zw
    assert fig["norm"][0] <= tol_norm, fig["norm"]
    assert fig["cos"][0] >= min_cos, fig["cos"]


def test_a_ninth_backbone_layer_is_refused_when_the_model_is_built():
    """More layers than SpairDims holds: the same refusal as any other unsupported configuration, raised before a parameter layout is made."""
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd.models import SPAIR
    case = dict(I=48, B=2, topology=((128, 4, 2),) * 3 + ((128, 1, 1),) * 6)
    with engine_config(case):
        with pytest.raises(L.SpairHipError, match="unsupported configuration"):
            SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
