"""spair_workspace_view (host arithmetic): every named buffer of the step's workspace resolves, lies inside spair_workspace_bytes, overlaps no
other one, and carries the element type the step plan (spair_step_plan) writes it in.  CPU only: the workspace is an
address that is never dereferenced.  The GPU side of the same view: tests/test_step_operands_gpu.py."""
import pytest
import torch

from test_workspace_cpu import WS, dims, workspace_bytes

CONFIGS = {
    "bench": ("bf16", [1, 128, 128], 256),          # BASELINE configs[1]
    "configs3": ("bf16", [1, 256, 256], 64),        # BASELINE configs[3]: 32 x 32 grid, the chain in bands
    "b37": ("bf16", [1, 128, 128], 37),
    "fp32": ("f32", [1, 128, 128], 32),
    "colour_bf16": ("bf16", [3, 48, 48], 4),
}
CELL_ROWS = ("Xb", "Hb1", "Hb2", "Ob", "glimpse", "He1", "He2", "Oe", "Xz", "Hz1", "Hz2", "Oz", "Xo", "Ho1", "Ho2", "Oo")
HEADS = ("Ob", "Oe", "Oz", "Oo")
LINS = ("box_network.body.dense0", "box_network.body.dense1", "box_network.output_layers.0", "box_network.output_layers.1",
        "object_encoder.dense0", "object_encoder.dense1", "object_encoder.out", "z_network.body.dense0", "z_network.body.dense1",
        "z_network.output_layers.0", "z_network.output_layers.1", "obj_network.dense0", "obj_network.dense1", "obj_network.out",
        "object_decoder.dense0", "object_decoder.dense1", "object_decoder.out")


def expected_names(d):
    from spair_pytorch_amd import _lib as L
    n = d.n_conv
    names = list(CELL_ROWS) + ["d" + r if r != "glimpse" else "dGl" for r in CELL_ROWS] + ["Za"]
    names += ["Hd1", "Hd2", "dHd1", "dHd2", "S", "dLog", "xpad", "feat", "dfeat"]
    names += ["act%d" % i for i in range(n)] + ["dact%d" % i for i in range(n)]
    if d.dtype == 1:
        names += ["Za16", "dfeat16"]
        if not L.step_plan(d, WS)["g16"]:
            names.append("dLog16")
    for i in range(1, n + 1):
        k, s = (d.conv_k[i], d.conv_s[i]) if i < n else (1, 1)
        names.append("conv_wf%d" % i)
        names += ["conv_wd%d_%d" % (i, q) for q in range(s * s if k > 1 else 1)]
    names += ["lin_wf." + x for x in LINS] + ["lin_wt." + x for x in LINS]
    return names


def views(d, flags):
    from spair_pytorch_amd import _lib as L
    return {nm: L.workspace_view(d, WS, nm, flags) for nm in L.workspace_view_names(d)}


@pytest.mark.parametrize("flags", (0, 1))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_buffer_resolves_inside_the_workspace_without_overlap(name, flags):
    from spair_pytorch_amd import _lib as L
    d = dims(*CONFIGS[name])
    total = workspace_bytes(d)
    v = views(d, flags)
    assert sorted(v) == sorted(set(expected_names(d)))
    spans = []
    for nm, x in v.items():
        es = torch.empty((), dtype=x["dtype"]).element_size()
        assert x["rows"] > 0 and 0 < x["cols"] <= x["ld"], nm
        lo, hi = x["offset"], x["offset"] + x["rows"] * x["ld"] * es
        if nm.startswith("lin_wt.") and nm.endswith("output_layers.0"):
            # a head's second layer: the columns behind the first one's in each row of their shared [in][pass | lat] matrix
            first = v[nm[:-1] + "1"]
            assert (x["ld"], x["rows"]) == (first["ld"], first["rows"]) and first["cols"] + x["cols"] <= x["ld"], nm
            assert x["offset"] == first["offset"] + first["cols"] * es, nm
            continue
        assert lo % 16 == 0 and 0 <= lo < hi <= total, nm
        spans.append((lo, hi, nm))
    spans.sort()
    for (lo0, hi0, a), (lo1, hi1, b) in zip(spans, spans[1:]):
        assert hi0 <= lo1, (a, b)
    with pytest.raises(L.SpairHipError):
        L.workspace_view(d, WS, "no_such_buffer", flags)
    with pytest.raises(L.SpairHipError):
        L.workspace_view(d, WS, "act%d" % d.n_conv, flags)       # conv_out writes feat: no act<n_conv>


@pytest.mark.parametrize("flags", (0, 1, 8, 16 | 32 | 64))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_element_types_follow_the_step_plan(name, flags):
    from spair_pytorch_amd import _lib as L
    d = dims(*CONFIGS[name])
    p, n = L.step_plan(d, WS, flags), L.step_plan_n(d, WS, flags)
    v = views(d, flags)
    b16 = d.dtype == 1
    act = torch.bfloat16 if b16 else torch.float32
    row = torch.bfloat16 if p["chain"] else torch.float32
    for r in CELL_ROWS:
        assert v[r]["dtype"] == (torch.float32 if r in HEADS else row) and v[r]["written"], r
        dr = "dGl" if r == "glimpse" else "d" + r
        assert v[dr]["dtype"] == (torch.float32 if r == "glimpse" else row), dr
        assert v[dr]["written"] == (not p["chain"] or r not in ("Xb", "Xz", "Xo", "glimpse")), dr
    assert v["S"]["dtype"] == (torch.float16 if p["s16"] else torch.float32)
    assert v["dLog"]["dtype"] == (torch.bfloat16 if p["g16"] else torch.float32)
    assert "dLog16" not in v or v["dLog16"]["dtype"] == torch.bfloat16
    for nm in ("Hd1", "Hd2", "dHd1", "dHd2") + tuple("act%d" % i for i in range(d.n_conv)) + tuple("dact%d" % i for i in range(d.n_conv)):
        assert v[nm]["dtype"] == act, nm
    assert v["dact0"]["written"] == (n["stem"] not in ("PATCH", "GEMM"))
    assert all(v["dact%d" % i]["written"] for i in range(1, d.n_conv))
    assert v["feat"]["dtype"] == v["dfeat"]["dtype"] == v["xpad"]["dtype"] == torch.float32
    assert v["dfeat"]["written"] == (not p["chain"])
    assert v["Za"]["written"] == (not p["chain"])
    for nm in v:
        if nm.startswith(("conv_w", "lin_w")):
            assert v[nm]["dtype"] == act and v[nm]["written"], nm
    # an image gradient: the fused chain's d glimpse is stored for it, and the stem's weight gradient reads a stored d act0
    vi = {nm: L.workspace_view(d, WS, nm, flags, input_grad=True) for nm in ("dGl", "dact0")}
    assert vi["dGl"]["written"] and vi["dact0"]["written"]


def test_view_shapes_follow_the_model():
    """The columns the model's definition gives each buffer (reference concatenation order: features, context, passthrough, box, attr, depth)."""
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd import config as cfg
    d = dims(*CONFIGS["bench"])
    v = views(d, 0)
    F, A, NP, N = d.F, d.A, d.NP, d.B * d.G * d.G
    ctx = 4 * (4 + A + 2)
    assert (v["Xb"]["rows"], v["Xb"]["cols"]) == (N, F + ctx)
    assert v["Xz"]["cols"] == F + ctx + NP + 4 + A and v["Xo"]["cols"] == F + ctx + NP + 4 + A + 1
    assert v["glimpse"]["cols"] == cfg.OBJECT_SHAPE[0] ** 2 and v["Ob"]["cols"] == NP + 8
    assert (v["lin_wf.box_network.output_layers.0"]["offset"] - v["lin_wf.box_network.output_layers.1"]["offset"]
            == NP * v["lin_wf.box_network.output_layers.1"]["ld"] * 2)
    assert (v["lin_wt.z_network.output_layers.0"]["offset"] - v["lin_wt.z_network.output_layers.1"]["offset"]) == NP * 2
    assert v["act1"]["rows"] == d.B * 34 * 34 and v["act1"]["cols"] == 128
    assert v["conv_wd1_3"]["rows"] == 128 and v["conv_wd1_3"]["cols"] == 4 * 128
