"""The gradient of the step with respect to its input image (``x.requires_grad_()``; SpairStepIO.grad_x, csrc/input_grad.hip).

* Kernel units against float64: the glimpse adjoint against the oracle's stn() autograd with respect to the image (border pile-up,
  tiny and 48-px boxes, align_corners 0 / 1, P 24 / 28 / 32, C 1 / 3), the stem's data gradient against conv2d's input gradient (k4 with
  s2 / s3, C 1 / 3, fp32 / bf16 d act0).  Both are gathers without atomics: two runs are bit-identical.
* The fp32 step against the reference fixtures (tests/golden/xgrad_*.npz) and the oracle: the network path (a term on z_where / z_pres
  alone) to 2e-3 of max|dx| per element and in norm; after loss.backward(), inf exactly where recon is 0 and the network part within 2e-3.
* The bf16 step (fused chain, fused decoder, matrix-core renderer): network-path cosine / norm within the step's BF16_BOUNDS.
* Nothing else moves: with x.requires_grad every parameter gradient, the loss and the outputs equal the run without it (conv_0's weight
  and bias to fp32 rounding: its unfused weight gradient sums in another order); x.grad repeats bit for bit; a retained-graph second
  backward doubles it exactly; an fp16 / non-contiguous x gets its gradient through the cast.
* Full size (B = 256, 128 x 128, bf16): the step runs, x.grad is finite where recon is in (0, 1) and repeats."""
import numpy as np
import pytest
import torch

from helpers import case_noise, case_weights, load_case, oracle_cfg
from oracle import spair_oracle as orc
from test_engine_gpu import BF16_BOUNDS
from test_input_grad_cpu import load_xgrad
from test_output_grads_gpu import build as _build_model
from test_output_grads_gpu import spair_cfg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

FP32_CASES = ["c2_b2_step1001", "ref_default_b2_step1001", "c1_b8_step7001", "c4_b1_step1001", "rgb_c1_b4_step1001",
              "lb2_c1_b4_step1001", "p24_c1_b4_step1001"]
# bf16 network-path bounds (norm, min cosine): BF16_BOUNDS' where the table has the fixture; colour / N_LOOKBACK 2 / P 24 run the
# per-wavefront bf16 step, held to the bounds of test_rgb_gpu.py / test_lookback_gpu.py
BF16_NET = {n: (BF16_BOUNDS[n][3], BF16_BOUNDS[n][4]) for n in FP32_CASES if n in BF16_BOUNDS}
BF16_NET.update({"rgb_c1_b4_step1001": (0.03, 0.99), "lb2_c1_b4_step1001": (0.03, 0.99), "p24_c1_b4_step1001": (0.03, 0.99)})


def _lib():
    from spair_pytorch_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _object_shape():
    from spair_pytorch_amd import config as cfg
    old = list(cfg.OBJECT_SHAPE)
    yield
    cfg.OBJECT_SHAPE[:] = old


def build(case, dtype, cfg, differentiable=True):
    """test_output_grads_gpu.build with the case's object size (the p24 fixture)."""
    cfg.OBJECT_SHAPE[:] = [case.get("obj_px", 28)] * 2
    return _build_model(case, dtype, cfg, differentiable=differentiable)


# ---------------------------------------------------------------------------------------------------------------------------------------
# kernel units
def glimpse_boxes(n, I, seed):
    g = torch.Generator().manual_seed(seed)
    nb = torch.stack([torch.rand(n, generator=g) * 1.2 - 0.1, torch.rand(n, generator=g) * 1.2 - 0.1,
                      torch.rand(n, generator=g) * 0.5 + 0.05, torch.rand(n, generator=g) * 0.5 + 0.05], 1)
    nb[0] = torch.tensor([-0.05, 0.97, 0.3, 0.4])              # partly outside: the border clip piles samples onto the edge pixels
    nb[1] = torch.tensor([0.5, 0.5, 3.0 / I, 2.0 / I])          # a box of a few pixels
    nb[2] = torch.tensor([0.3, 0.6, 48.0 / I, 48.0 / I])        # 48-pixel box
    nb[3] = torch.tensor([1.02, -0.03, 0.2, 0.25])             # centre outside the image
    return nb


@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("P", [24, 28, 32])
@pytest.mark.parametrize("C", [1, 3])
def test_glimpse_adjoint_unit(ac, P, C):
    L = _lib()
    B, ncell, I = 3, 7, 64
    R = B * ncell
    nbox = glimpse_boxes(R, I, 10 * P + C + ac)
    g = torch.Generator().manual_seed(P + C)
    x = torch.rand(B, C, I, I, generator=g, dtype=torch.float64).requires_grad_()
    dG = torch.randn(R, C, P, P, generator=g).float()
    rows_b = torch.arange(R) % B                                 # row r = k * B + b
    out = orc.stn(x[rows_b], nbox.double(), (P, P), align_corners=bool(ac))
    (ref,) = torch.autograd.grad((out * dG.double()).sum(), [x])
    ld = C * P * P + 8
    dgl = torch.zeros(R, ld)
    dgl[:, :C * P * P] = dG.reshape(R, -1)
    dgl, nb = dgl.cuda(), nbox.float().contiguous().cuda()
    got = [torch.full((B, C, I, I), float("nan"), device="cuda") for _ in range(2)]
    for o in got:
        L.check(L.lib().spair_input_grad_glimpse(L.ptr(nb), B, ncell, L.ptr(dgl), ld, L.ptr(o), C, I, P, ac, L.stream()),
                "spair_input_grad_glimpse")
    torch.cuda.synchronize()
    assert torch.equal(got[0], got[1])
    err = (got[0].cpu().double() - ref).abs().max().item()
    assert err <= 1e-4 * ref.abs().max().item(), err
    # the edge column / row under box 0 carries the pile-up
    assert ref[0, :, :, 0].abs().max() > 0


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("bf16", [0, 1])
def test_stem_dgrad_unit(s, C, bf16):
    L = _lib()
    B, I, k, Cout, pre, post = 2, 40, 4, 128, 1, 2
    Ip = I + pre + post
    Hout = (Ip - k) // s + 1
    g = torch.Generator().manual_seed(s * 10 + C + bf16)
    dact = torch.randn(B, Hout, Hout, Cout, generator=g)
    if bf16:
        dact = dact.bfloat16()
    w = torch.randn(Cout, C, k, k, generator=g) * 0.1
    add = torch.randn(B, C, I, I, generator=g)
    dxp = torch.nn.grad.conv2d_input((B, C, Ip, Ip), w.double(), dact.double().permute(0, 3, 1, 2), stride=s)
    ref = dxp[:, :, pre:pre + I, pre:pre + I] + add.double()
    dd, wd, ad = dact.contiguous().cuda(), w.contiguous().cuda(), add.cuda()
    got = [torch.full((B, C, I, I), float("nan"), device="cuda") for _ in range(2)]
    for o in got:
        L.check(L.lib().spair_input_grad_stem(L.ptr(dd), bf16, L.ptr(wd), B, C, I, pre, k, s, Hout, Cout, L.ptr(ad), L.ptr(o), L.stream()),
                "spair_input_grad_stem")
    torch.cuda.synchronize()
    assert torch.equal(got[0], got[1])
    err = (got[0].cpu().double() - ref).abs().max().item()
    assert err <= 1e-5 * ref.abs().max().item(), err


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole step
def model_xgrads(m, z, ref):
    """(x.grad after loss.backward(), x.grad after the network-path term alone, recon) of the engine."""
    step, noise = int(z["global_step"]), {k: torch.from_numpy(np.asarray(z[k])).cuda() for k in ("eps_box", "eps_attr", "eps_depth", "u_pres")}
    wz, wp = torch.from_numpy(ref["wz"]).cuda(), torch.from_numpy(ref["wp"]).cuda()
    res = []
    for what in ("loss", "net"):
        m.zero_grad()
        x = torch.from_numpy(np.asarray(z["x"])).cuda().requires_grad_()
        loss, recon, z_where, z_pres = m(x, step, noise=noise)
        ((wz * z_where).sum() + (wp * z_pres).sum() if what == "net" else loss).backward()
        res.append(x.grad.detach().double().cpu().numpy())
    return res[0], res[1], recon.detach().double().cpu().numpy()


def oracle_xgrads(z, case, ref):
    x = torch.from_numpy(z["x"]).clone().requires_grad_()
    out = orc.forward(case_weights(case, requires_grad=True), x, int(z["global_step"]), case_noise(z), oracle_cfg(case))
    (g_loss,) = torch.autograd.grad(out["loss"], [x], retain_graph=True)
    term = (torch.from_numpy(ref["wz"]) * out["z_where"]).sum() + (torch.from_numpy(ref["wp"]) * out["z_pres"]).sum()
    (g_net,) = torch.autograd.grad(term, [x])
    return g_loss.double().numpy(), g_net.double().numpy(), out["recon_x"].detach().double().numpy()


def bce_target(r):
    with np.errstate(divide="ignore"):
        return np.log1p(-r) - np.log(r)


def close(got, ref, what, rel=2e-3):
    err = np.abs(got - ref).max()
    assert err <= rel * np.abs(ref).max(), "%s: max err %.3e vs max|ref| %.3e" % (what, err, np.abs(ref).max())
    gn, rn = np.linalg.norm(got), np.linalg.norm(ref)
    assert abs(gn - rn) <= rel * rn, "%s: norm %.6e vs %.6e" % (what, gn, rn)


@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_input_gradient(name, spair_cfg):  # noqa: F811
    z, case = load_case(name)
    ref = load_xgrad(name)
    m = build(case, "f32", spair_cfg, differentiable=True)
    g_loss, g_net, recon = model_xgrads(m, z, ref)
    o_loss, o_net, o_recon = oracle_xgrads(z, case, ref)
    close(g_net, ref["xgrad_net"], name + " network path vs reference")
    close(g_net, o_net, name + " network path vs oracle")
    # after loss.backward(): +inf exactly where the model's recon is 0, and no NaN
    assert np.array_equal(np.isinf(g_loss), (recon == 0) | (recon == 1)) and (g_loss[recon == 0] > 0).all()
    assert not np.isnan(g_loss).any()
    inner = (recon > 0) & (recon < 1) & (o_recon > 0) & (o_recon < 1)
    net_got, net_orc = g_loss - bce_target(recon), o_loss - bce_target(o_recon)
    tol = 2e-3 * np.abs(net_orc[inner]).max() + 1e-6 * np.abs(bce_target(recon[inner]))
    assert (np.abs(net_got[inner] - net_orc[inner]) <= tol).all(), np.abs(net_got[inner] - net_orc[inner]).max()
    assert m.step_status() == 0          # the infinities are the gradient's, not the loss's


def test_fp32_conv_object_encoder_input_gradient(spair_cfg):  # noqa: F811
    """The convolutional object encoder (per-wavefront launches, dGl from its own first conv's data gradient) against the oracle only."""
    import golden_inputs as gi
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import SPAIR
    I, B, step, strides = 48, 3, 1500, (2, 2, 2, 1, 1, 1)
    topo = [(32, 4, 2), (32, 3, 2), (32, 3, 2), (32, 1, 1)]
    spair_cfg.set_grid(I, strides)
    spair_cfg.INPUT_IMAGE_SHAPE[0] = 1
    spair_cfg.N_LOOKBACK = 1
    torch.manual_seed(5)
    m = SPAIR([1, I, I], None, torch.device("cuda"), compute_dtype="f32", object_encoder="conv", differentiable_outputs=True).to("cuda")
    G = gi.grid_side(I, strides)
    x = torch.from_numpy(scattered_digits(21, B, I, 4)[0])
    noise = {k: torch.from_numpy(v) for k, v in gi.make_noise(9, B, G).items()}
    rng = np.random.default_rng(11)
    ref = dict(wz=rng.standard_normal((B, 4, G, G)).astype(np.float32), wp=rng.standard_normal((B, 1, G, G)).astype(np.float32))
    z = dict(x=x.numpy(), global_step=step, **{k: v.numpy() for k, v in noise.items()})
    p = {k: v.detach().cpu().clone().requires_grad_(not k.startswith("attn.")) for k, v in m.state_dict().items()}
    g_loss, g_net, recon = model_xgrads(m, z, ref)
    xo = x.clone().requires_grad_()
    out = orc.forward(p, xo, step, noise,
                      orc.OracleConfig(image_shape=(1, I, I), conv_strides=strides, object_conv=topo))
    term = (torch.from_numpy(ref["wz"]) * out["z_where"]).sum() + (torch.from_numpy(ref["wp"]) * out["z_pres"]).sum()
    (o_net,) = torch.autograd.grad(term, [xo])
    close(g_net, o_net.double().numpy(), "conv encoder network path vs oracle")
    assert np.array_equal(np.isinf(g_loss), (recon == 0) | (recon == 1)) and not np.isnan(g_loss).any()


@pytest.mark.parametrize("name", FP32_CASES)
def test_bf16_input_gradient(name, spair_cfg):  # noqa: F811
    z, case = load_case(name)
    ref = load_xgrad(name)
    m = build(case, "bf16", spair_cfg, differentiable=True)
    g_loss, g_net, recon = model_xgrads(m, z, ref)
    r = ref["xgrad_net"].astype(np.float64).ravel()
    g = g_net.ravel()
    tol_norm, min_cos = BF16_NET[name]
    cos = float(g @ r / (np.linalg.norm(g) * np.linalg.norm(r)))
    assert cos >= min_cos, cos
    assert abs(np.linalg.norm(g) - np.linalg.norm(r)) <= tol_norm * np.linalg.norm(r)
    assert np.array_equal(np.isinf(g_loss), (recon == 0) | (recon == 1)) and not np.isnan(g_loss).any()


def _step(m, x, step, noise, requires_grad):
    m.zero_grad()
    xx = x.clone().requires_grad_(requires_grad)
    loss, recon, z_where, z_pres = m(xx, step, noise=noise)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return loss.detach().clone(), recon.clone(), z_where.clone(), z_pres.clone(), grads, (None if xx.grad is None else xx.grad.clone())


@pytest.mark.parametrize("name", ["c2_b2_step1001", "ref_default_b2_step1001"])
def test_bf16_nothing_else_moves(name, spair_cfg):  # noqa: F811
    z, case = load_case(name)
    m = build(case, "bf16", spair_cfg, differentiable=False)
    x = torch.from_numpy(z["x"]).cuda()
    step, noise = int(z["global_step"]), {k: v.cuda() for k, v in case_noise(z).items()}
    a = _step(m, x, step, noise, False)
    b = _step(m, x, step, noise, True)
    c = _step(m, x, step, noise, True)
    assert a[5] is None and b[5] is not None
    for i in range(4):
        assert torch.equal(a[i], b[i]), i
    for k in a[4]:
        if k.startswith("backbone.net.conv_0."):
            assert torch.allclose(b[4][k], a[4][k], rtol=1e-5, atol=1e-5 * a[4][k].abs().max().item()), k
        else:
            assert torch.equal(a[4][k], b[4][k]), k
    assert torch.equal(b[5], c[5])                    # bit-identical across two identical steps


def test_retain_graph_doubles_and_cast_input(spair_cfg):  # noqa: F811
    name = "c2_b2_step1001"
    z, case = load_case(name)
    m = build(case, "bf16", spair_cfg, differentiable=True)
    step, noise = int(z["global_step"]), {k: v.cuda() for k, v in case_noise(z).items()}
    x = torch.from_numpy(z["x"]).cuda().requires_grad_()
    m.zero_grad()
    loss, recon, z_where, z_pres = m(x, step, noise=noise)
    term = loss + z_where.sum()
    term.backward(retain_graph=True)
    first = x.grad.clone()
    term.backward()
    fin = torch.isfinite(first)
    assert torch.equal(x.grad[fin], 2 * first[fin]) and torch.equal(torch.isinf(x.grad), ~fin)
    # an fp16, non-contiguous input gets its gradient through forward's .contiguous().float()
    xh = torch.from_numpy(z["x"]).cuda().half().transpose(2, 3).requires_grad_()
    m.zero_grad()
    loss, *_ = m(xh.transpose(2, 3), step, noise=noise)
    loss.backward()
    assert xh.grad is not None and xh.grad.dtype == torch.float16 and xh.grad.shape == xh.shape


def test_full_size_step(spair_cfg):  # noqa: F811
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.data import scattered_digits
    from spair_pytorch_amd.models import SPAIR
    I, B = 128, 256
    cfg.set_grid(I, (2, 2, 2, 1, 1, 1))
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.N_LOOKBACK = 1
    torch.manual_seed(3)
    m = SPAIR([1, I, I], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
    x = torch.from_numpy(scattered_digits(1234, B, I, 11)[0]).cuda()
    e = m._engine(B)
    noise = {k: torch.randn_like(v) if k != "u_pres" else torch.rand_like(v) for k, v in e["noise"].items()}
    out = []
    for _ in range(2):
        m.zero_grad()
        xx = x.clone().requires_grad_()
        loss, recon, _, _ = m(xx, 2000, noise=noise)
        loss.backward()
        out.append((xx.grad.clone(), recon.clone()))
    g, r = out[0]
    inner = (r > 0) & (r < 1)
    assert torch.isfinite(g[inner]).all() and g[inner].abs().max() > 0
    assert torch.equal(torch.isinf(g), (r == 0) | (r == 1))
    assert torch.equal(out[0][0], out[1][0])
