"""The kernel plan of the training step (spair_step_plan: the host arithmetic make_ctx runs -- render_plan, chain_fwd_supported,
dec_fused_supported) for the configurations the suite covers.  CPU only: the workspace is an address that is never dereferenced.

A predicate edit that moves one of these configurations to another renderer family, turns the fused chain or the fused decoder on or
off, or changes a sprite / d-logit format fails here; tests/test_object_geometry_gpu.py runs each of them against the oracle."""
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
