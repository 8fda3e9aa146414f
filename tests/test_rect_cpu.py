"""Rectangular images ([C, H, W], H != W) on the host side: the per-axis geometry make_dims derives (the reference's own padding and grid,
modules.py:68-105), the kernel plan a rectangular step gets (spair_step_plan: host arithmetic, no GPU), the geometry the C ABI refuses and
the ABI version check."""
import ctypes

import pytest

WS = 1 << 30          # a 256-byte-aligned fake workspace base (never read)
S2 = (2, 2, 2, 1, 1, 1)


def dims(dtype, shape, B, strides=None, lookback=1):
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.models import make_dims
    topo = [dict(t) for t in cfg.DEFAULT_BACKBONE_TOPOLOGY]
    for layer, s in zip(topo, strides or ()):
        layer["stride"] = s
    return make_dims(B, list(shape), topo, dtype, None, lookback)


def geometry(d):
    return (d.I, d.Iw, d.G, d.Gw, d.pad_pre, d.pad_post, d.pad_post_w)


def test_make_dims_matches_the_reference_padding_and_grid():
    # the reference's ZeroPad2d (left, right, top, bottom) and grid for these images with its default topology
    assert geometry(dims("f32", [1, 128, 96], 2)) == (128, 96, 11, 8, 9, 14, 10)
    assert geometry(dims("f32", [1, 48, 80], 2)) == (48, 80, 4, 7, 9, 10, 14)
    assert geometry(dims("f32", [3, 60, 36], 2)) == (60, 36, 5, 3, 9, 10, 10)
    # a square image leaves the width fields at 0: the C ABI's "same as I, G, pad_post"
    d = dims("f32", [1, 128, 128], 2)
    assert (d.Iw, d.Gw, d.pad_post_w) == (0, 0, 0)


def test_set_grid_keeps_its_meaning():
    from spair_pytorch_amd import config as cfg
    old, strides = list(cfg.INPUT_IMAGE_SHAPE), [t["stride"] for t in cfg.DEFAULT_BACKBONE_TOPOLOGY]
    try:
        cfg.set_grid(64, S2)
        assert cfg.INPUT_IMAGE_SHAPE[1:] == [64, 64]
        cfg.set_grid(48, S2, image_width=80)
        assert cfg.INPUT_IMAGE_SHAPE[1:] == [48, 80]
    finally:
        cfg.INPUT_IMAGE_SHAPE[:] = old
        for t, s in zip(cfg.DEFAULT_BACKBONE_TOPOLOGY, strides):
            t["stride"] = s


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape,B,strides", [([1, 128, 96], 64, None), ([1, 48, 80], 4, S2), ([1, 96, 160], 8, S2)])
def test_rectangular_grey_plan_runs_the_general_kernels(dtype, shape, B, strides):
    from spair_pytorch_amd import _lib as L
    p = L.step_plan(dims(dtype, shape, B, strides), WS)
    assert not p["chain"] and not p["rec"]
    assert p["fwd"] == "GEN1" and p["bwd"] == "GEN1"
    n = L.step_plan_n(dims(dtype, shape, B, strides), WS)
    assert "PATCH" not in n["fwd"] and "PATCH" not in n["dgrad"] and not any(n["gate_bits"])
    assert n["stem"] == "GENERIC"
    # an image gradient does not change that
    n = L.step_plan_n(dims(dtype, shape, B, strides), WS, 0, True)
    assert "PATCH" not in n["fwd"] and "PATCH" not in n["dgrad"] and n["stem"] == "GENERIC"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rectangular_colour_plan(dtype):
    from spair_pytorch_amd import _lib as L
    p = L.step_plan(dims(dtype, [3, 40, 64], 2, S2), WS)
    assert p["fwd"] == "COLOUR" and p["bwd"] == "COLOUR" and not p["chain"] and not p["rec"]


def test_square_plans_are_unchanged():
    """A few of test_render_plan_cpu.py's square plans again: the bf16 step at the benchmark shape keeps the fused chain, the records, the
    matrix-core forward, the patch-resident convs and the stem fused into conv_1's data gradient."""
    from spair_pytorch_amd import _lib as L
    d = dims("bf16", [1, 128, 128], 64, S2)
    p = L.step_plan(d, WS)
    assert p["chain"] and p["rec"] and p["fwd"] == "MMA" and p["bwd"] == "GEN2" and p["s16"] and p["g16"]
    n = L.step_plan_n(d, WS)
    assert n["fwd"][:2] == ("PATCH", "PATCH") and n["dgrad"][:2] == ("PATCH", "PATCH") and n["stem"] == "PATCH"
    p = L.step_plan(dims("f32", [1, 48, 48], 4, S2), WS)
    assert not p["chain"] and p["fwd"] == "GEN2" and p["bwd"] == "GEN1"
    # flags bit 0 (no fused chain) on the square image: the same path the rectangular step runs, except the renderer / convs it may keep
    p = L.step_plan(d, WS, 1)
    assert not p["chain"] and p["fwd"] == "MMA"


def _workspace_bytes(d):
    from spair_pytorch_amd import _lib as L
    f = L.lib().spair_workspace_bytes
    f.restype = ctypes.c_int64
    return f(ctypes.byref(d))


def test_out_of_range_geometry_is_refused():
    # G * Gw + 1 > 1025 (the count-prior KL's one workgroup): 33 x 32 cells of 8 px
    assert _workspace_bytes(dims("f32", [1, 256, 264], 1, S2)) < 0
    assert _workspace_bytes(dims("f32", [1, 256, 256], 1, S2)) > 0
    # N_LOOKBACK > 1 needs max(G, Gw) <= 32: 8 x 40 cells
    assert _workspace_bytes(dims("f32", [1, 64, 320], 1, S2, lookback=2)) < 0
    assert _workspace_bytes(dims("f32", [1, 64, 320], 1, S2, lookback=1)) > 0
    assert _workspace_bytes(dims("f32", [1, 64, 256], 1, S2, lookback=2)) > 0
    # a width chain that does not reach Gw
    d = dims("f32", [1, 48, 80], 2, S2)
    d.Gw += 1
    assert _workspace_bytes(d) < 0


def test_workspace_of_a_rectangle_is_between_its_squares():
    small, rect, big = (_workspace_bytes(dims("f32", s, 4, S2)) for s in ([1, 48, 48], [1, 48, 80], [1, 80, 80]))
    assert 0 < small < rect < big


def test_abi_version_3_matches():
    """Version 3: the step's entry points take SpairStepIO (include/spair_hip.h); the binding and the library agree on it."""
    from spair_pytorch_amd import _lib as L
    assert L.lib().spair_abi_version() == L.ABI_VERSION == 3
