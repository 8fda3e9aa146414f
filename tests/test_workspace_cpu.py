"""The step workspace (spair_workspace_bytes) against the kernel plan (spair_step_plan).  The engine allocates an optional
buffer only where the plan of SpairStep.flags 0, no image gradient and an aligned base reads it; flags, an image gradient and a misaligned
base may only turn kernels off.  CPU only: host arithmetic, the workspace is an address that is never dereferenced."""
import ctypes

import pytest

WS = 1 << 30          # a 256-byte-aligned fake workspace base (never read)
S2 = (2, 2, 2, 1, 1, 1)
S11 = (3, 2, 2, 1, 1, 1)


def dims(dtype, shape, B, strides=S2, P=28, ac=0, object_conv=False, lookback=1, extra_pad=0):
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.models import make_dims
    topo = [dict(t) for t in cfg.DEFAULT_BACKBONE_TOPOLOGY]
    for layer, s in zip(topo, strides):
        layer["stride"] = s
    old = list(cfg.OBJECT_SHAPE), cfg.ALIGN_CORNERS
    cfg.OBJECT_SHAPE[:] = [P, P]
    cfg.ALIGN_CORNERS = bool(ac)
    try:
        d = make_dims(B, list(shape), topo, dtype, [dict(t) for t in cfg.CONV_OBJECT_ENCODER_TOPOLOGY] if object_conv else None, lookback)
    finally:
        cfg.OBJECT_SHAPE[:], cfg.ALIGN_CORNERS = old
    d.pad_post += extra_pad
    return d


# name -> (dims arguments, workspace bytes of the engine before the workspace was allocated from the plan)
CONFIGS = {
    "bench": (("bf16", [1, 128, 128], 256), {}),                        # BASELINE configs[1]
    "configs3": (("bf16", [1, 256, 256], 64), {}),                      # BASELINE configs[3]: 32 x 32 grid, the chain in bands
    "fp32": (("f32", [1, 128, 128], 256), {}),
    "fp32_48": (("f32", [1, 48, 48], 4), {}),
    "bf16_48": (("bf16", [1, 48, 48], 4), {}),
    "colour_bf16": (("bf16", [3, 48, 48], 4), {}),
    "colour_fp32": (("f32", [3, 48, 48], 2), dict(P=24, ac=1)),
    "rect_bf16": (("bf16", [1, 128, 96], 64, (2, 2, 2, 1, 1, 1)), {}),
    "rect_fp32": (("f32", [1, 48, 80], 4), {}),
    "lookback2": (("bf16", [1, 128, 128], 32), dict(lookback=2)),
    "lookback3": (("f32", [1, 128, 128], 8), dict(lookback=3)),
    "objconv_bf16": (("bf16", [1, 48, 48], 4), dict(object_conv=True)),
    "objconv_fp32": (("f32", [1, 48, 48], 4), dict(object_conv=True)),
    "P24": (("bf16", [1, 48, 48], 4), dict(P=24)),
    "P32": (("bf16", [1, 64, 64], 2), dict(P=32)),
    "odd_conv1_input": (("bf16", [1, 128, 128], 4), dict(extra_pad=2)),
    "grid11": (("bf16", [1, 128, 128], 32, S11), {}),
    "conv1_past_patch": (("bf16", [1, 128, 128], 3600), {}),
}
PARENT_BYTES = {
    "bench": 4114196992,
    "configs3": 4080929024,
    "fp32": 5094756864,
    "fp32_48": 224779264,
    "bf16_48": 219594496,
    "colour_bf16": 226131456,
    "colour_fp32": 223450368,
    "rect_bf16": 896389120,
    "rect_fp32": 232030976,
    "lookback2": 756158208,
    "lookback3": 423427840,
    "objconv_bf16": 230422272,
    "objconv_fp32": 235142144,
    "P24": 215486208,
    "P32": 217380864,
    "odd_conv1_input": 271713024,
    "grid11": 447932160,
    "conv1_past_patch": 55107428352,
}
# exact: every optional buffer of these workspaces is read by the step that runs on them
EXACT = ("bench", "configs3")


def workspace_bytes(d):
    from spair_pytorch_amd import _lib as L
    f = L.lib().spair_workspace_bytes
    f.restype = ctypes.c_int64
    return f(ctypes.byref(d))


def config_dims(name):
    args, kw = CONFIGS[name]
    return dims(*args, **kw)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_workspace_never_grows(name):
    n = workspace_bytes(config_dims(name))
    assert n > 0
    if name in EXACT:
        assert n == PARENT_BYTES[name]
    else:
        assert n <= PARENT_BYTES[name]


def test_fp32_workspace_drops_the_bf16_copies():
    """An fp32 step carries no bf16 copy of the decoder input and of d feat: the workspace is smaller than it was."""
    assert workspace_bytes(config_dims("fp32")) < PARENT_BYTES["fp32"]


def test_unused_sign_bits_are_not_allocated():
    """B = 3600: conv_1's input is past the patch-resident kernels' 32-bit offsets, so conv_1 runs as an implicit GEMM and leaves no sign
    bits -- nor is there room for them."""
    from spair_pytorch_amd import _lib as L
    d = config_dims("conv1_past_patch")
    assert L.step_plan_n(d, WS)["fwd"][0] == "GEMM"
    assert workspace_bytes(d) < PARENT_BYTES["conv1_past_patch"]


FLAGS = (0, 1, 4, 8, 16, 32, 64, 127)


def selected(p, n):
    """What a plan selects that reads an optional buffer (or is only sound on a workspace laid out for it)."""
    return dict(chain=p["chain"], rec=p["rec"], dec_fused=p["dec_fused"], gate_bits=n["gate_bits"], stem_fused=n["stem"] in ("PATCH", "GEMM"),
                fwd_patch=tuple(k == "PATCH" for k in n["fwd"]), dgrad_patch=tuple(k == "PATCH" for k in n["dgrad"]))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_plan_is_covered_by_the_workspace_plan(name):
    """Whatever a step plan selects, for any SpairStep.flags, image gradient or base alignment, the flags-0, aligned plan of the same dims
    (the one the workspace is allocated from) selects too; the sprite and d-logit formats do not change."""
    from spair_pytorch_amd import _lib as L
    d = config_dims(name)

    def plan(base, flags, input_grad):
        p = L.step_plan(d, base, flags)
        return p, selected(p, L.step_plan_n(d, base, flags, input_grad))
    p0, s0 = plan(WS, 0, False)
    for base in (WS, WS + 4):
        for flags in FLAGS:
            for input_grad in (False, True):
                p, s = plan(base, flags, input_grad)
                assert (p["s16"], p["g16"]) == (p0["s16"], p0["g16"])
                for k, v in s.items():
                    if isinstance(v, tuple):
                        assert all(not a or b for a, b in zip(v, s0[k])), (k, base, flags, input_grad)
                    else:
                        assert not v or s0[k], (k, base, flags, input_grad)
