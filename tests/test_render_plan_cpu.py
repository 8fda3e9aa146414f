"""The kernel plan of the training step (spair_step_plan: the host arithmetic make_ctx runs -- render_plan,
chain_fwd_supported, dec_fused_supported, the backbone's and the decoder backward's predicates) for the configurations the suite covers.
CPU only: the workspace is an address that is never dereferenced.

A predicate edit that moves one of these configurations to another renderer family, turns the fused chain or the fused decoder on or
off, or changes a sprite / d-logit format fails here; tests/test_object_geometry_gpu.py runs each of them against the oracle.  The same
holds for the backbone's kernels per layer, the gate each data gradient reads, where the stem's weight gradient is taken, and the decoder
backward's kernels and stream."""
import pytest

WS = 1 << 30          # a 256-byte-aligned fake workspace base (the workspace's buffers share its alignment)
STRIDES = (2, 2, 2, 1, 1, 1)


def dims(dtype, C, P, ac, I, B, strides=STRIDES, object_conv=False):
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.models import make_dims
    topo = [dict(t) for t in cfg.DEFAULT_BACKBONE_TOPOLOGY]
    for layer, s in zip(topo, strides):
        layer["stride"] = s
    old = list(cfg.OBJECT_SHAPE), cfg.ALIGN_CORNERS
    cfg.OBJECT_SHAPE[:] = [P, P]
    cfg.ALIGN_CORNERS = bool(ac)
    try:
        return make_dims(B, [C, I, I], topo, dtype, [dict(t) for t in cfg.CONV_OBJECT_ENCODER_TOPOLOGY] if object_conv else None)
    finally:
        cfg.OBJECT_SHAPE[:], cfg.ALIGN_CORNERS = old


def plan(dtype, C, P, ac, I, B, flags=0, **kw):
    from spair_pytorch_amd import _lib as L
    return L.step_plan(dims(dtype, C, P, ac, I, B, **kw), WS, flags)


def expect(fwd, bwd, rec=False, s16=False, chain=False, dec_fused=False):
    return dict(fwd=fwd, bwd=bwd, rec=rec, s16=s16, g16=s16, chain=chain, dec_fused=dec_fused)


BF16_28 = expect("MMA", "GEN2", rec=True, s16=True, chain=True, dec_fused=True)
# (dtype, C, P, align_corners, I, B, flags) -> plan
PLANS = {
    # the default configurations: the bench geometry, the fixtures' 48 x 48, the reference's 11 x 11 grid, fp32
    ("bf16", 1, 28, 0, 128, 32, 0): BF16_28,
    ("bf16", 1, 28, 0, 48, 4, 0): BF16_28,
    ("bf16", 1, 28, 0, 256, 1, 0): BF16_28,
    ("f32", 1, 28, 0, 48, 4, 0): expect("GEN2", "GEN1"),
    ("f32", 1, 28, 0, 128, 2, 0): expect("GEN2", "GEN1"),
    # SpairStep.flags: bit 0 the per-wavefront cell path, bit 4 the decoder forward unfused -- the renderer stays
    ("bf16", 1, 28, 0, 48, 4, 1): dict(BF16_28, chain=False),
    ("bf16", 1, 28, 0, 48, 4, 16): dict(BF16_28, dec_fused=False),
    # align_corners: no records (render_prep refuses), so the tap forward; the chain and the fused decoder still run
    ("bf16", 1, 28, 1, 64, 4, 0): expect("GEN2", "GEN2", s16=True, chain=True, dec_fused=True),
    ("bf16", 1, 28, 1, 64, 4, 1): expect("GEN2", "GEN2", s16=True, chain=False, dec_fused=True),
    # other object sizes: the chain needs P = 28; the fused decoder needs 2 P^2 % 32 == 0 and at most 64 column pairs
    ("bf16", 1, 24, 0, 48, 4, 0): expect("GEN2", "GEN2", s16=True, dec_fused=True),             # 36 pairs
    ("bf16", 1, 26, 0, 48, 3, 0): expect("GEN1", "GEN1", s16=True),                             # P % 4 != 0: first generation, g16
    ("bf16", 1, 32, 0, 64, 2, 0): expect("GEN2", "GEN1", s16=True, dec_fused=True),             # 64 pairs; P^2 * 4 > RB2_ADJ_BYTES
    ("f32", 1, 28, 1, 48, 4, 0): expect("GEN2", "GEN1"),
    ("f32", 1, 25, 0, 48, 3, 0): expect("GEN1", "GEN1"),                                        # odd P: 8-byte texels not 16-byte rows
    ("f32", 1, 24, 0, 48, 4, 0): expect("GEN2", "GEN1"),
    # colour
    ("f32", 3, 24, 1, 48, 2, 0): expect("COLOUR", "COLOUR"),
    ("bf16", 3, 24, 1, 48, 2, 0): expect("COLOUR", "COLOUR"),
    ("bf16", 3, 28, 0, 48, 4, 0): expect("COLOUR", "COLOUR"),
    ("f32", 2, 28, 0, 48, 4, 0): expect("COLOUR", "COLOUR"),
}


@pytest.mark.parametrize("key", list(PLANS), ids=lambda k: "%s-C%d-P%d-ac%d-I%d-B%d-f%d" % k)
def test_step_plan(key):
    dtype, C, P, ac, I, B, flags = key
    assert plan(dtype, C, P, ac, I, B, flags) == PLANS[key]


def test_step_plan_conv_object_nets():
    """The convolutional object encoder / decoder: fp32 sprites and d-logits in either dtype, no chain, no fused decoder."""
    assert plan("bf16", 1, 28, 0, 48, 4, object_conv=True) == expect("GEN2", "GEN1")


def test_step_plan_refuses_what_the_engine_refuses():
    from spair_pytorch_amd import _lib as L
    d = dims("bf16", 1, 28, 0, 48, 4)
    d.C = 4
    with pytest.raises(L.SpairHipError, match="code -4"):
        L.step_plan(d, WS)
    with pytest.raises(L.SpairHipError, match="code -1"):
        L.step_plan(dims("bf16", 1, 28, 0, 48, 4), 0)


# spair_step_plan: the default topology's layers 1 .. 6 are conv_1, conv_2 (4x4, stride 2 here) and four 1x1 layers (conv_3 .. conv_out),
# which run as the fused 1x1 stack in the bf16 step
PW4 = ("PW_STACK",) * 4


def expect_n(fwd=("PATCH", "PATCH"), dgrad=("PATCH", "PATCH"), bits=(True, True), stem="PATCH", side=True, dec_dgrad_fused=True,
             dec_wgrad_grouped=True, dec_wgrad_late=True):
    return dict(side=side, dec_dgrad_fused=dec_dgrad_fused, dec_wgrad_grouped=dec_wgrad_grouped, dec_wgrad_late=dec_wgrad_late, pw0=3,
                stem=stem, fwd=tuple(fwd) + PW4, dgrad=tuple(dgrad) + PW4, gate_bits=tuple(bits) + (False,) * 4)


BENCH = expect_n()      # patch-resident conv_1 / conv_2 both ways, their gates as sign bits, the stem's weight gradient in conv_1's dgrad
# fp32: no 1x1 stack (pw0 = n_conv + 1), the per-class data gradient of the strided layers, the stem's weight gradient as a TN GEMM
F32 = dict(expect_n(stem="GENERIC", dec_dgrad_fused=False, dec_wgrad_grouped=False, dec_wgrad_late=False), pw0=7, fwd=("GEMM",) * 6,
           dgrad=("PER_CLASS", "PER_CLASS") + ("GEMM",) * 4, gate_bits=(False,) * 6)
S11 = (3, 2, 2, 1, 1, 1)
# (dtype, C, I, B, strides, flags, input_grad) -> plan
PLANS_N = {
    ("bf16", 1, 128, 32, STRIDES, 0, 0): BENCH,
    ("bf16", 1, 48, 4, STRIDES, 0, 0): BENCH,
    ("bf16", 1, 256, 1, STRIDES, 0, 0): BENCH,
    # the reference's 11 x 11 grid: stride-3 stem (no sign bits; the fused stem needs an even stride), conv_1's patch dgrad without it
    ("bf16", 1, 128, 32, S11, 0, 0): expect_n(bits=(False, True), stem="WGRAD16"),
    ("bf16", 1, 128, 8, S11, 0, 1): expect_n(bits=(False, True), stem="WGRAD16"),
    # an image gradient keeps d act0 in HBM: no stem fusion
    ("bf16", 1, 128, 32, STRIDES, 0, 1): expect_n(stem="WGRAD16"),
    ("f32", 1, 48, 4, STRIDES, 0, 0): F32,
    ("f32", 1, 128, 2, STRIDES, 0, 1): F32,
    # SpairStep.flags: bit 0 no fused chain (the decoder's weight gradients at once), bit 2 no helper stream, bit 3 no stem fusion, bit 5 no
    # patch-resident kernels (the stem fused into conv_1's implicit-GEMM dgrad instead), bit 6 the decoder's data gradients as three GEMMs
    ("bf16", 1, 128, 32, STRIDES, 1, 0): expect_n(dec_wgrad_late=False),
    ("bf16", 1, 128, 32, STRIDES, 4, 0): expect_n(side=False, dec_wgrad_late=False),
    ("bf16", 1, 128, 32, STRIDES, 8, 0): expect_n(stem="WGRAD16"),
    ("bf16", 1, 128, 32, STRIDES, 32, 0): expect_n(fwd=("GEMM", "GEMM"), dgrad=("GEMM", "GEMM"), bits=(False, False), stem="GEMM"),
    ("bf16", 1, 128, 32, STRIDES, 40, 0): expect_n(fwd=("GEMM", "GEMM"), dgrad=("GEMM", "GEMM"), bits=(False, False), stem="WGRAD16"),
    ("bf16", 1, 128, 32, STRIDES, 64, 0): expect_n(dec_dgrad_fused=False),
    ("bf16", 1, 48, 4, STRIDES, 4 | 8 | 64, 0): expect_n(side=False, stem="WGRAD16", dec_dgrad_fused=False, dec_wgrad_late=False),
    # conv_1's input past the patch kernels' 32-bit offsets (B Hin^2 128 >= 2^31): its implicit-GEMM forward / class-batched dgrad, too
    # many tiles for the fused stem; conv_2 keeps the patch kernels, its gate as the activation
    ("bf16", 1, 128, 3600, STRIDES, 0, 0): expect_n(fwd=("GEMM", "PATCH"), dgrad=("GEMM", "PATCH"), bits=(False, False), stem="WGRAD16"),
    # colour: the generic-channel stem (no sign bits), the decoder's weight gradients at once (no fused chain)
    ("bf16", 3, 48, 4, STRIDES, 0, 0): expect_n(bits=(False, True), stem="GENERIC", dec_wgrad_late=False),
}


@pytest.mark.parametrize("key", list(PLANS_N), ids=lambda k: "%s-C%d-I%d-B%d-s%d-f%d-x%d" % (k[:4] + (k[4][0],) + k[5:]))
def test_step_plan_n(key):
    from spair_pytorch_amd import _lib as L
    dtype, C, I, B, strides, flags, input_grad = key
    assert L.step_plan_n(dims(dtype, C, 28, 0, I, B, strides=strides), WS, flags, input_grad) == PLANS_N[key]


def test_step_plan_n_odd_conv1_input():
    """Two more padding columns make conv_1's input odd (71 x 71 for 34 x 34 out): no patch kernel, the per-class data gradient, the stem's
    weight gradient on its own; conv_2 keeps the patch kernels but gates with the activation (conv_1 left no sign bits)."""
    from spair_pytorch_amd import _lib as L
    d = dims("bf16", 1, 28, 0, 128, 4)
    d.pad_post += 2
    assert L.step_plan_n(d, WS) == expect_n(fwd=("GEMM", "PATCH"), dgrad=("PER_CLASS", "PATCH"), bits=(False, False), stem="WGRAD16")


def test_step_plan_n_conv_object_nets():
    """The convolutional object decoder: none of the MLP decoder's backward kernels; the backbone as with the MLP nets."""
    from spair_pytorch_amd import _lib as L
    assert L.step_plan_n(dims("bf16", 1, 28, 0, 48, 4, object_conv=True), WS) == expect_n(dec_dgrad_fused=False, dec_wgrad_grouped=False,
                                                                                         dec_wgrad_late=False)


def test_step_plan_writes_the_first_n_ints():
    """spair_step_plan writes min(n, SPAIR_STEP_PLAN_INTS) ints: step_plan reads the first 8 of them (out[7] = 0), step_plan_n all."""
    import ctypes
    from spair_pytorch_amd import _lib as L
    d = ctypes.byref(dims("bf16", 1, 28, 1, 64, 4))
    n = L.STEP_PLAN_INTS
    full, head, part = (ctypes.c_int * (n + 2))(*[-7] * (n + 2)), (ctypes.c_int * 8)(), (ctypes.c_int * n)(*[-7] * n)
    L.check(L.lib().spair_step_plan(d, ctypes.c_void_p(WS), 16, 0, full, n + 2), "spair_step_plan")
    L.check(L.lib().spair_step_plan(d, ctypes.c_void_p(WS), 16, 0, head, 8), "spair_step_plan")
    L.check(L.lib().spair_step_plan(d, ctypes.c_void_p(WS), 16, 0, part, 10), "spair_step_plan")
    assert list(full)[n:] == [-7, -7]
    assert list(head) == list(full)[:8] and full[7] == 0
    assert list(part) == list(full)[:10] + [-7] * (n - 10)
