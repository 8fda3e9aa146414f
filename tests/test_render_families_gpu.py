"""The renderer and STN kernels the suite's default configuration never reaches (P = 28, align_corners = 0 accepts every fast path), each
through its C-ABI entry point, against the oracle's composite and spatial transformer evaluated in FLOAT64 with autograd:

* align_corners = 1: k_render_fwd3<*, 0, 1, 0>, k_render_bwd2<0, 1, 0, false>, k_render_bwd<false> and the colour kernels with ac = 1;
* other object sizes: the tap kernels without the P = 28 specialisation (P = 24, 32), the first-generation forward k_render_fwd
  (8-byte fp32 texels with odd P, 4-byte fp16 texels with P % 4 != 0), the first-generation backward with fp16 sprites and bf16
  d-logits (P = 26, and P = 32 whose adjoint tile exceeds k_render_bwd2's LDS budget);
* the STN glimpse (border padding) and inverse (zeros padding) at ac = 0 / 1 and P = 24 / 28, with boxes that sample outside the source;
* the matrix-core forward's loud refusal of what it does not implement.

Which kernel each case runs is fixed by the families' _supported predicates (csrc/render.hip, render2.hip); the step-level selection is
pinned by tests/test_render_plan_cpu.py.  Bounds are those of the P = 28 tests in test_kernels_gpu.py."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import spair_oracle as orc

pytestmark = pytest.mark.gpu


def _L():
    from spair_pytorch_amd import _lib as L
    return L


def _f(v):
    return ctypes.c_float(v)


def objects(seed, B, HW, I, P, C=1, smin=0.08, srange=0.5, degenerate=False, f16=False):
    """Sprites [N,P,P,C+1] after the sigmoid (fp16-representable with f16), boxes, presence, depth and a target image, float64 leaves."""
    g = torch.Generator().manual_seed(seed)
    N = B * HW
    logits = torch.randn(N, P, P, C + 1, generator=g)
    logits[..., C] += 1.0
    S = torch.sigmoid(logits)
    if f16:
        S = S.half().float()
    nbox = torch.stack([torch.rand(N, generator=g) * 1.2 - 0.1, torch.rand(N, generator=g) * 1.2 - 0.1,
                        torch.rand(N, generator=g) * srange + smin, torch.rand(N, generator=g) * srange + smin], 1)
    pres = torch.rand(N, generator=g)
    depth = torch.rand(N, generator=g) * 4
    if degenerate and N > 4:    # off-screen, vanishing, absent, half off the edge
        nbox[0] = torch.tensor([5.0, 5.0, 0.2, 0.2]); nbox[1] = torch.tensor([0.5, 0.5, 1e-12, 0.3]); pres[2] = 0.0
        nbox[3] = torch.tensor([-0.2, 0.98, 0.5, 0.5])
    x = (torch.rand(B, C, I, I, generator=g) > 0.7).float() * torch.rand(B, C, I, I, generator=g)
    return [t.double().requires_grad_(True) for t in (S, nbox, pres, depth)] + [x.double()]


def composite64(S, nbox, pres, depth, x, B, HW, I, ac):
    """The oracle's composite (oracle.render on given sprites, closed-form inverse affine) in float64: recon and the BCE sum; rows
    r = k * B + b."""
    N, C = B * HW, S.shape[-1] - 1
    alpha = S[..., C] * pres.view(N, 1, 1)
    imp = torch.clamp(alpha * depth.view(N, 1, 1), min=0.01)
    objs = torch.cat([S[..., :C].permute(0, 3, 1, 2), alpha[:, None], imp[:, None]], 1)
    t = orc.stn(objs, nbox, (I, I), inverse=True, align_corners=bool(ac), inverse_mode="closed")
    t = t.view(HW, B, C + 2, I, I).permute(1, 0, 2, 3, 4)
    colour, al, im = t[:, :, :C], t[:, :, C:C + 1], t[:, :, C + 1:C + 2] + 1e-9
    im = im / im.sum(1, keepdim=True)
    rec = torch.clamp((al * colour * im).sum(1), 0, 1)
    return rec, F.binary_cross_entropy(rec, x, reduction="sum")


def reference(B, HW, I, ac, S, nbox, pres, depth, x):
    rec, bce = composite64(S, nbox, pres, depth, x, B, HW, I, ac)
    bce.backward()
    C = S.shape[-1] - 1
    s = S.detach()
    dlog = (S.grad * s * (1 - s) * torch.tensor([2.0] * C + [0.1], dtype=torch.float64)).reshape(B * HW, -1)
    return rec.detach(), bce.item(), dlog, nbox.grad, pres.grad, depth.grad


def close(name, got, want, tol):
    got, want = got.detach().double().cpu(), want.detach().double()
    err = (got - want).abs().max().item()
    bound = tol * want.abs().max().item() + 1e-7
    assert err <= bound, (name, err, bound)


def device_inputs(nbox, pres, depth, x):
    return [t.detach().float().contiguous().cuda() for t in (nbox, pres, depth, x)]


def nblocks(B, I):
    return B * ((I + 15) // 16) ** 2


# ---- grey, fp32 sprites and d-logits (spair_render_fwd / _bwd: the fp32 step's renderer) ------------------------------------------------
# (P, ac, B, G, I, smin, srange): forward k_render_fwd3<false, 0, ac, 0> for even P, k_render_fwd<false> for odd P; backward k_render_bwd<false>
GREY32 = [
    (28, 1, 2, 3, 64, 0.08, 0.5),
    (28, 1, 1, 2, 96, 0.7, 0.5),       # magnified
    (24, 0, 2, 4, 72, 0.08, 0.5),
    (24, 1, 2, 4, 96, 0.02, 0.1),      # minified
    (25, 0, 2, 3, 64, 0.08, 0.5),
    (27, 1, 2, 3, 72, 0.08, 0.5),
    (25, 0, 1, 2, 96, 0.7, 0.5),       # magnified, first-generation forward
    (32, 0, 2, 3, 64, 0.08, 0.5),
]


@pytest.mark.parametrize("P,ac,B,G,I,smin,srange", GREY32)
def test_render_fp32_families_vs_float64(P, ac, B, G, I, smin, srange):
    L = _L()
    HW = G * G
    N = B * HW
    S, nbox, pres, depth, x = objects(100 + P + I + ac, B, HW, I, P, smin=smin, srange=srange, degenerate=True)
    rec_o, bce_o, dlog_o, dnb_o, dpr_o, ddp_o = reference(B, HW, I, ac, S, nbox, pres, depth, x)
    Sd = S.detach().float().reshape(N, -1).contiguous().cuda()
    nb, pr, dp, xd = device_inputs(nbox, pres, depth, x)
    ld = P * P * 2
    recon = torch.zeros(B, 1, I, I, device="cuda")
    aux = torch.zeros(B, I, I, 2, device="cuda")
    part = torch.zeros(nblocks(B, I), device="cuda")
    L.check(L.lib().spair_render_fwd(L.ptr(Sd), ld, L.ptr(nb), L.ptr(pr), L.ptr(dp), L.ptr(xd), L.ptr(recon), L.ptr(aux), L.ptr(part),
                                     B, HW, 1, I, P, ac, L.stream()), "render fwd")
    assert (recon.cpu().double() - rec_o).abs().max().item() < 2e-5
    assert abs(part.sum().item() - bce_o) <= 2e-5 * bce_o
    gl = torch.ones((), device="cuda")
    dlog = torch.zeros(N, ld, device="cuda")
    dnb, dpr, ddp = torch.zeros(N, 4, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    L.check(L.lib().spair_render_bwd(L.ptr(Sd), ld, L.ptr(nb), L.ptr(pr), L.ptr(dp), L.ptr(aux), L.ptr(gl), L.ptr(dlog), L.ptr(dnb),
                                     L.ptr(dpr), L.ptr(ddp), B, HW, 1, I, P, ac, _f(2.0), _f(0.1), L.stream()), "render bwd")
    close("dlogits", dlog, dlog_o, 2e-4)
    close("dpres", dpr, dpr_o, 2e-4)
    close("ddepth", ddp, ddp_o, 2e-4)
    close("dnbox", dnb, dnb_o, 1e-3)
    assert N <= 4 or (dnb[0] == 0).all()         # the off-screen object


# ---- grey, fp16 sprites and bf16 d-logits (spair_render_fwd16 / _bwd16: the bf16 step's renderer) ------------------------------------------
# P = 28 ac = 1: k_render_fwd3<true, 0, 1, 0> + k_render_bwd2<0, 1, 0, false>;  P = 24: both tap kernels without the P = 28 specialisation;
# P = 26: k_render_fwd<true> + k_render_bwd<true> (bf16 d-logits);  P = 32: k_render_fwd3 + k_render_bwd<true>
GREY16 = [
    (28, 1, 2, 4, 64, 0.08, 0.5),
    (28, 1, 2, 4, 96, 0.02, 0.1),
    (24, 0, 2, 4, 72, 0.08, 0.5),
    (24, 1, 1, 2, 64, 0.7, 0.5),
    (26, 0, 2, 3, 64, 0.08, 0.5),
    (26, 1, 2, 4, 96, 0.02, 0.1),
    (32, 0, 2, 3, 64, 0.08, 0.5),
    (32, 1, 1, 2, 72, 0.7, 0.5),
]


@pytest.mark.parametrize("P,ac,B,G,I,smin,srange", GREY16)
def test_render_16bit_families_vs_float64(P, ac, B, G, I, smin, srange):
    """The oracle runs on the SAME fp16-rounded sprites.  Forward fp32 math (2e-5); the d-logits leave as bf16 (1e-2 of the largest
    element, cosine >= 0.9999), d pres / d depth 1e-2, d z_where 1e-3 -- test_render16_fwd_bwd_vs_oracle's bounds."""
    L = _L()
    HW = G * G
    N = B * HW
    S, nbox, pres, depth, x = objects(200 + P + I + ac, B, HW, I, P, smin=smin, srange=srange, degenerate=True, f16=True)
    rec_o, bce_o, dlog_o, dnb_o, dpr_o, ddp_o = reference(B, HW, I, ac, S, nbox, pres, depth, x)
    Sd = S.detach().reshape(N, -1).half().contiguous().cuda()
    nb, pr, dp, xd = device_inputs(nbox, pres, depth, x)
    ld = P * P * 2
    recon = torch.zeros(B, 1, I, I, device="cuda")
    aux = torch.zeros(B, I, I, 2, device="cuda")
    part = torch.zeros(nblocks(B, I), device="cuda")
    L.check(L.lib().spair_render_fwd16(L.ptr(Sd), ld, L.ptr(nb), L.ptr(pr), L.ptr(dp), L.ptr(xd), L.ptr(recon), L.ptr(aux), L.ptr(part),
                                       B, HW, 1, I, P, ac, L.stream()), "render fwd16")
    assert (recon.cpu().double() - rec_o).abs().max().item() < 2e-5
    assert abs(part.sum().item() - bce_o) <= 2e-5 * bce_o
    gl = torch.ones((), device="cuda")
    dlog = torch.zeros(N, ld, device="cuda", dtype=torch.bfloat16)
    dnb, dpr, ddp = torch.zeros(N, 4, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    L.check(L.lib().spair_render_bwd16(L.ptr(Sd), ld, L.ptr(nb), L.ptr(pr), L.ptr(dp), L.ptr(aux), L.ptr(gl), L.ptr(dlog), L.ptr(dnb),
                                       L.ptr(dpr), L.ptr(ddp), B, HW, 1, I, P, ac, _f(2.0), _f(0.1), L.stream()), "render bwd16")
    got = dlog.float().cpu().double()
    close("dlogits", got, dlog_o, 1e-2)
    cos = float((got * dlog_o).sum() / (got.norm() * dlog_o.norm() + 1e-30))
    assert cos >= 0.9999, cos
    close("dnbox", dnb, dnb_o, 1e-3)
    close("dpres", dpr, dpr_o, 1e-2)
    close("ddepth", ddp, ddp_o, 1e-2)
    assert N <= 4 or (dnb[0] == 0).all()


# ---- colour (render_c.hip) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,P,ac,B,G,I,smin,srange", [(3, 28, 1, 2, 3, 48, 0.08, 0.5), (2, 28, 1, 1, 2, 72, 0.7, 0.5),
                                                       (3, 24, 0, 2, 4, 64, 0.02, 0.3), (2, 24, 1, 2, 3, 64, 0.08, 0.5)])
def test_render_rgb_families_vs_float64(C, P, ac, B, G, I, smin, srange):
    """test_render_rgb_fwd_bwd_vs_oracle's bounds (forward 2e-5, gradients 2e-4, d z_where 1e-3) and its run-to-run bit identity."""
    L = _L()
    HW = G * G
    N = B * HW
    S, nbox, pres, depth, x = objects(300 + C + P + I + ac, B, HW, I, P, C=C, smin=smin, srange=srange, degenerate=True)
    rec_o, bce_o, dlog_o, dnb_o, dpr_o, ddp_o = reference(B, HW, I, ac, S, nbox, pres, depth, x)
    Sd = S.detach().float().reshape(N, -1).contiguous().cuda()
    nb, pr, dp, xd = device_inputs(nbox, pres, depth, x)
    ld = P * P * (C + 1)
    gl = torch.ones((), device="cuda")
    outs = []
    for _ in range(2):
        recon = torch.zeros(B, C, I, I, device="cuda")
        aux = torch.zeros(B, C, I, I, 2, device="cuda")
        part = torch.zeros(nblocks(B, I), device="cuda")
        L.check(L.lib().spair_render_fwd_rgb(L.ptr(Sd), ld, L.ptr(nb), L.ptr(pr), L.ptr(dp), L.ptr(xd), L.ptr(recon), L.ptr(aux), L.ptr(part),
                                             B, HW, C, I, P, ac, L.stream()), "render fwd rgb")
        dlog = torch.zeros(N, ld, device="cuda")
        dnb, dpr, ddp = torch.zeros(N, 4, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        L.check(L.lib().spair_render_bwd_rgb(L.ptr(Sd), ld, L.ptr(nb), L.ptr(pr), L.ptr(dp), L.ptr(aux), L.ptr(gl), L.ptr(dlog), L.ptr(dnb),
                                             L.ptr(dpr), L.ptr(ddp), B, HW, C, I, P, ac, _f(2.0), _f(0.1), L.stream()), "render bwd rgb")
        outs.append([t.cpu() for t in (recon, part, dlog, dnb, dpr, ddp)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    recon, part, dlog, dnb, dpr, ddp = outs[0]
    assert (recon.double() - rec_o).abs().max().item() < 2e-5
    assert abs(part.sum().item() - bce_o) <= 2e-5 * bce_o
    close("dlogits", dlog, dlog_o, 2e-4)
    close("dpres", dpr, dpr_o, 2e-4)
    close("ddepth", ddp, ddp_o, 2e-4)
    close("dnbox", dnb, dnb_o, 1e-3)


# ---- the matrix-core forward refuses what it does not implement, and writes nothing ---------------------------------------------------------
@pytest.mark.parametrize("P,ac", [(28, 1), (24, 0), (32, 0), (26, 1)])
def test_render_mma_refuses_other_geometry(P, ac):
    L = _L()
    B, HW, I = 2, 9, 64
    N = B * HW
    nb = torch.tensor([[0.5, 0.5, 0.3, 0.3]] * N, device="cuda")
    pr, dp = torch.full((N,), 0.5, device="cuda"), torch.ones(N, device="cuda")
    x = torch.rand(B, 1, I, I, device="cuda")
    recs = torch.full((N * 16,), 7, device="cuda", dtype=torch.int32)
    assert L.lib().spair_render_prep(L.ptr(nb), L.ptr(pr), L.ptr(dp), L.ptr(recs), B, HW, I, P, ac, L.stream()) == -4
    Sd = torch.rand(N, P * P * 2, device="cuda").half()
    recon = torch.full((B, 1, I, I), 3.0, device="cuda")
    aux = torch.full((B, I, I, 2), 3.0, device="cuda")
    part = torch.full((nblocks(B, I),), 3.0, device="cuda")
    assert L.lib().spair_render_fwd16m(L.ptr(Sd), P * P * 2, L.ptr(recs), L.ptr(x), L.ptr(recon), L.ptr(aux), L.ptr(part),
                                       B, HW, 1, I, P, ac, L.stream()) == -4
    torch.cuda.synchronize()
    assert (recs == 7).all() and (recon == 3.0).all() and (aux == 3.0).all() and (part == 3.0).all()


# ---- STN glimpse / inverse against float64 affine_grid + grid_sample ------------------------------------------------------------------------
def _theta(nbox, inverse):
    """(xt, yt, xs, ys) -> [N,2,3]; the inverse in closed form (the kernels' and the oracle's `closed` mode)."""
    xt, yt, xs, ys = nbox.unbind(-1)
    tx, ty = 2 * xt - 1, 2 * yt - 1
    z = torch.zeros_like(xs)
    if inverse:
        return torch.stack([torch.stack([1 / xs, z, -tx / xs], -1), torch.stack([z, 1 / ys, -ty / ys], -1)], 1)
    return torch.stack([torch.stack([xs, z, tx], -1), torch.stack([z, ys, ty], -1)], 1)


def stn64(src, nbox, out_side, inverse, ac):
    N, C = nbox.shape[0], src.shape[1]
    grid = F.affine_grid(_theta(nbox, inverse), [N, C, out_side, out_side], align_corners=bool(ac))
    return F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros" if inverse else "border", align_corners=bool(ac))


def _boxes(g, n):
    """Centres from -0.3 to 1.3 and scales up to 1.4: many glimpses reach past the image (border clip, zero clip gradient)."""
    return torch.stack([torch.rand(n, generator=g) * 1.6 - 0.3, torch.rand(n, generator=g) * 1.6 - 0.3,
                        torch.rand(n, generator=g) * 1.35 + 0.05, torch.rand(n, generator=g) * 1.35 + 0.05], 1).double()


@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("P,I,C", [(28, 64, 1), (24, 48, 1), (24, 72, 3)])
def test_stn_glimpse_vs_float64(P, I, C, ac):
    L = _L()
    B, R = 3, 12                                    # row r samples image r % B
    g = torch.Generator().manual_seed(400 + P + I + C + ac)
    img = torch.rand(B, C, I, I, generator=g).double()
    nbox = _boxes(g, R).requires_grad_(True)
    out = stn64(img[torch.arange(R) % B], nbox, P, False, ac)
    gw = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * gw).sum().backward()
    assert (nbox.detach()[:, 0] * 2 - 1 + nbox.detach()[:, 2] > 1).any()       # some glimpses are clipped
    x, nb = img.float().contiguous().cuda(), nbox.detach().float().cuda()
    gl = torch.zeros(R, C * P * P, device="cuda")
    L.check(L.lib().spair_stn_glimpse_fwd(L.ptr(x), L.ptr(nb), B, L.ptr(gl), C * P * P, R, C, I, P, ac, L.stream()), "stn fwd")
    assert (gl.cpu().double().view(R, C, P, P) - out.detach()).abs().max().item() < 1e-5
    dgl = gw.float().reshape(R, -1).contiguous().cuda()
    dnb = torch.zeros(R, 4, device="cuda")
    L.check(L.lib().spair_stn_glimpse_bwd(L.ptr(x), L.ptr(nb), B, L.ptr(dgl), C * P * P, L.ptr(dnb), R, C, I, P, ac, L.stream()), "stn bwd")
    close("dnbox", dnb, nbox.grad, 3e-4)


@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("P,I,C", [(28, 64, 3), (24, 48, 1), (24, 80, 2)])
def test_stn_inverse_vs_float64(P, I, C, ac):
    L = _L()
    N = 10
    g = torch.Generator().manual_seed(500 + P + I + C + ac)
    spr = torch.rand(N, C, P, P, generator=g).double().requires_grad_(True)
    nbox = _boxes(g, N)
    nbox[:, 2:] = nbox[:, 2:] * 0.6 + 0.05                                      # objects from 5 % to 90 % of the image
    nbox.requires_grad_(True)
    out = stn64(spr, nbox, I, True, ac)
    gw = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * gw).sum().backward()
    sp, nb = spr.detach().float().contiguous().cuda(), nbox.detach().float().cuda()
    o = torch.zeros(N, C, I, I, device="cuda")
    L.check(L.lib().spair_stn_inverse_fwd(L.ptr(sp), L.ptr(nb), L.ptr(o), N, C, P, I, ac, L.stream()), "stn inverse fwd")
    assert (o.cpu().double() - out.detach()).abs().max().item() < 1e-5
    go = gw.float().contiguous().cuda()
    dsp, dnb = torch.zeros(N, C, P, P, device="cuda"), torch.zeros(N, 4, device="cuda")
    L.check(L.lib().spair_stn_inverse_bwd(L.ptr(sp), L.ptr(nb), L.ptr(go), L.ptr(dsp), L.ptr(dnb), N, C, P, I, ac, L.stream()),
            "stn inverse bwd")
    close("dsprites", dsp, spr.grad, 1e-4)
    close("dnbox", dnb, nbox.grad, 5e-4)
