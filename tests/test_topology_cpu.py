"""Other backbone topologies and network sizes (golden_inputs.TOPO_CASES / ORACLE_CASES), host side: the kernels spair_step_plan picks for each,
the parameter layout, the workspace's regions and the shapes of the prepared conv weight copies -- and what validate() refuses.  CPU only: the
workspace is an address that is never dereferenced.

Each case is there for a branch of the plan (the T = 3 / T = 1 weight packs, cin = 64 in tap-parity order, a 1x1 stack of 2 or 3 layers, a 1x1
layer left outside the stack, conv_out alone behind patch-resident layers, the stem's weight gradient in a k = 6 conv_1's data gradient, a
patch data gradient gated by the stored activation, the per-wavefront chain behind the patch-resident backbone, k_gauss_kl at 64 lanes).  A
predicate edit that silently moves a case off its branch fails here; tests/test_topology_gpu.py runs every case against the reference's
fixture (or the oracle)."""
import ctypes

import pytest
import torch

import golden_inputs as gi
from helpers import case_engine_topology, engine_config

WS = 1 << 30          # a 256-byte-aligned fake workspace base
ALL = dict(gi.TOPO_CASES, **gi.ORACLE_CASES)
PW = "PW_STACK"
#        chain   pw0  stem       conv kernels, layers 1 .. n_conv (conv_out last): forward = data gradient           gate_bits
BF16 = {
    "t_shallow64": (True, 4, "GENERIC", ("GEMM", "GEMM", "GEMM"), (0, 0, 0)),                                         # cin = 64: no stack
    "t_k3": (True, 3, "GENERIC", ("GEMM", "GEMM", PW, PW, PW), (0,) * 5),                                              # T = 3 and T = 1 packs
    "t_k6": (True, 3, "GEMM", ("GEMM", "PATCH", PW, PW), (0,) * 4),      # k = 6 conv_1 takes the stem's wgrad; conv_2's patch dgrad gates with act1
    "t_nostack": (True, 4, "PATCH", ("PATCH", "PATCH", "GEMM"), (1, 1, 0)),                                        # conv_out alone, a 1x1 GEMM
    "t_deep8": (True, 6, "GENERIC", ("GEMM",) * 5 + (PW,) * 3, (0,) * 8),                                              # a stack of 3 behind a 72-wide layer
    "t_stack5": (True, 3, "PATCH", ("PATCH", "GEMM", PW, PW, PW, PW), (1, 0, 0, 0, 0, 0)),                             # the fifth 1x1 layer outside the stack
    "t_stem5": (True, 2, "GENERIC", ("GEMM", PW, PW), (0,) * 3),                                                      # a stack of 2
    "t_feat64": (False, 3, "PATCH", ("PATCH", "PATCH", PW, PW, PW, PW), (1, 1, 0, 0, 0, 0)),
    "t_feat128": (False, 3, "PATCH", ("PATCH", "PATCH", PW, PW, PW, PW), (1, 1, 0, 0, 0, 0)),
    "o_attr16": (False, 3, "PATCH", ("PATCH", "PATCH", PW, PW, PW, PW), (1, 1, 0, 0, 0, 0)),
    "o_attr59": (False, 3, "PATCH", ("PATCH", "PATCH", PW, PW, PW, PW), (1, 1, 0, 0, 0, 0)),
}
CHAIN_CASES = [n for n, v in BF16.items() if v[0]]


def dims(name, dtype):
    from spair_pytorch_amd.models import make_dims
    case = ALL[name]
    with engine_config(case):
        return make_dims(case["B"], [1, case["I"], case["I"]], case_engine_topology(case), dtype)


def expected(name, dtype, flags):
    """(step_plan, step_plan_n) of a case."""
    topo = gi.case_topology(ALL[name])
    n = len(topo)
    if dtype == "f32":      # everywhere: the implicit-GEMM forward, the per-class data gradient of every k > 1 layer, the stem as a TN GEMM
        kinds = tuple("PER_CLASS" if k > 1 else "GEMM" for _, k, _ in topo[1:]) + ("GEMM",)
        return (dict(fwd="GEN2", bwd="GEN1", rec=False, s16=False, g16=False, chain=False, dec_fused=False),
                dict(side=True, dec_dgrad_fused=False, dec_wgrad_grouped=False, dec_wgrad_late=False, pw0=n + 1, stem="GENERIC",
                     fwd=("GEMM",) * n, dgrad=kinds, gate_bits=(False,) * n))
    chain, pw0, stem, kinds, bits = BF16[name]
    chain = chain and not flags & 1
    return (dict(fwd="MMA", bwd="GEN2", rec=True, s16=True, g16=True, chain=chain, dec_fused=True),
            dict(side=True, dec_dgrad_fused=True, dec_wgrad_grouped=True, dec_wgrad_late=chain, pw0=pw0, stem=stem, fwd=kinds, dgrad=kinds,
                 gate_bits=tuple(bool(b) for b in bits)))


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(ALL))
def test_step_plan_of_every_case(name, dtype, flags):
    from spair_pytorch_amd import _lib as L
    d = dims(name, dtype)
    want = expected(name, dtype, flags)
    assert L.step_plan(d, WS, flags) == want[0]
    assert L.step_plan_n(d, WS, flags) == want[1]


def test_the_cases_cover_the_branches_they_are_there_for():
    """The table above, read back: what each case is in the suite for."""
    n_stack = {n: len(gi.case_topology(ALL[n])) + 1 - v[1] for n, v in BF16.items()}
    assert (n_stack["t_stem5"], n_stack["t_deep8"], n_stack["t_stack5"], n_stack["t_nostack"], n_stack["t_shallow64"]) == (2, 3, 4, 0, 0)
    assert BF16["t_k6"][2] == "GEMM" and BF16["t_k6"][3][1] == "PATCH" and not BF16["t_k6"][4][1]
    assert BF16["t_stack5"][3][1] == "GEMM" and gi.case_topology(ALL["t_stack5"])[2][1] == 1
    assert len(CHAIN_CASES) == 7 and gi.ORACLE_CASES["o_attr59"]["A"] + 5 == 64
    assert sorted({k // s for n in ALL for _, k, s in gi.case_topology(ALL[n])[1:] if k > 1}) == [1, 2, 3]      # T = k / s of the weight packs


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(ALL))
def test_param_layout_is_the_state_dict(name, dtype):
    from spair_pytorch_amd import _lib as L
    d = dims(name, dtype)
    lib = L.lib()
    lib.spair_param_total.restype = ctypes.c_int64
    buf, off, ndim, shape = ctypes.create_string_buffer(128), ctypes.c_int64(), ctypes.c_int(), (ctypes.c_int64 * 4)()
    got, end = [], 0
    for i in range(lib.spair_param_count(ctypes.byref(d))):
        L.check(lib.spair_param_info(ctypes.byref(d), i, buf, 128, ctypes.byref(off), shape, ctypes.byref(ndim)), "spair_param_info")
        shp = tuple(int(shape[k]) for k in range(ndim.value))
        got.append((buf.value.decode(), shp))
        n = 1
        for v in shp:
            n *= v
        assert off.value >= end and off.value + n <= lib.spair_param_total(ctypes.byref(d)), buf.value      # in order, no overlap, inside
        end = off.value + n
    assert got == list(gi.param_shapes(**gi.case_net(ALL[name])).items())


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(ALL))
def test_workspace_regions_are_disjoint_and_inside(name, dtype):
    from spair_pytorch_amd import _lib as L
    d = dims(name, dtype)
    lib = L.lib()
    lib.spair_workspace_bytes.restype = ctypes.c_int64
    total = lib.spair_workspace_bytes(ctypes.byref(d))
    assert total > 0
    names = L.workspace_view_names(d)
    assert len(names) == len(set(names)) and len(names) > 60
    spans = []
    for nm in names:
        v = L.workspace_view(d, WS, nm)
        es = torch.empty((), dtype=v["dtype"]).element_size()
        assert v["rows"] > 0 and 0 < v["cols"] <= v["ld"], (nm, v)
        lo, hi = v["offset"], v["offset"] + ((v["rows"] - 1) * v["ld"] + v["cols"]) * es
        assert 0 <= lo and hi <= total, (nm, v, total)
        if nm.startswith("lin_wt.") and nm.endswith("output_layers.0"):
            # by design inside its head's transposed matrix: the columns behind output_layers.1's, in the same rows
            h = L.workspace_view(d, WS, nm[:-1] + "1")
            assert v["ld"] == h["ld"] and v["rows"] == h["rows"] and v["offset"] == h["offset"] + h["cols"] * es and h["cols"] + v["cols"] <= h["ld"]
            continue
        spans.append((lo, hi, nm))
    spans.sort()
    for (lo0, hi0, n0), (lo1, hi1, n1) in zip(spans, spans[1:]):
        assert hi0 <= lo1, (n0, n1)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(ALL))
def test_prepared_conv_weight_shapes(name, dtype):
    """include/spair_hip.h, spair_workspace_view: conv_wf<i> is [cout][k k cin], conv_wd<i>_<q> [cin][T T cout] per output-parity class
    q < s s (T = k / s), a 1x1 layer's single conv_wd<i>_0 [cin][cout]; leading dimensions: the columns, rounded up to 8 elements."""
    from spair_pytorch_amd import _lib as L
    d = dims(name, dtype)
    case = ALL[name]
    layers = list(gi.case_topology(case)) + [(gi.case_net(case)["n_features"], 1, 1)]
    want = {}
    for i in range(1, len(layers)):
        (cout, k, s), cin = layers[i], layers[i - 1][0]
        want["conv_wf%d" % i] = (cout, k * k * cin, (k * k * cin + 7) // 8 * 8)
        if k == 1:
            want["conv_wd%d_0" % i] = (cin, cout, (cout + 7) // 8 * 8)
        else:
            T = k // s
            for q in range(s * s):
                want["conv_wd%d_%d" % (i, q)] = (cin, T * T * cout, T * T * cout)
    got = {}
    for nm in L.workspace_view_names(d):
        if nm.startswith("conv_w"):
            v = L.workspace_view(d, WS, nm)
            assert v["dtype"] == (torch.bfloat16 if dtype == "bf16" else torch.float32)
            got[nm] = (v["rows"], v["cols"], v["ld"])
    assert got == want


# ---- what validate() refuses ----------------------------------------------------------------------------------------------------------------------
DEFAULT = ((128, 4, 2), (128, 4, 2), (128, 4, 2), (128, 1, 1), (128, 1, 1), (128, 1, 1))


def _with_layer(i, layer):
    return DEFAULT[:i] + (layer,) + DEFAULT[i + 1:]


REFUSED = {
    "inner_k3_s2": dict(topology=_with_layer(1, (128, 3, 2))),          # k % s != 0
    "inner_k1_s2": dict(topology=_with_layer(3, (128, 1, 2))),          # a strided 1x1 layer
    "inner_k3_s3": dict(topology=_with_layer(1, (128, 3, 3))),          # an inner stride above 2
    "filters_60": dict(topology=_with_layer(2, (60, 4, 2))),            # filter counts are multiples of 8
    "A_60": dict(topology=DEFAULT, A=60),                               # A + 5 > 64 lanes of k_gauss_kl
    "F_102": dict(topology=DEFAULT, F=102),                             # F and NP are multiples of 4
    "nine_layers": dict(topology=DEFAULT + ((128, 1, 1),) * 3),         # more layers than SpairDims holds
}


def _workspace_bytes(case, dtype):
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd.models import make_dims
    case = dict(dict(I=48, B=4), **case)
    with engine_config(case):
        d = make_dims(case["B"], [1, case["I"], case["I"]], case_engine_topology(case), dtype)
    lib = L.lib()
    lib.spair_workspace_bytes.restype = ctypes.c_int64
    lib.spair_param_total.restype = ctypes.c_int64
    return lib.spair_workspace_bytes(ctypes.byref(d)), lib.spair_param_total(ctypes.byref(d)), lib.spair_param_count(ctypes.byref(d))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_configurations(what, dtype):
    assert _workspace_bytes(dict(topology=DEFAULT), dtype)[0] > 0          # (the network each of them is one edit away from runs)
    nbytes, total, count = _workspace_bytes(REFUSED[what], dtype)
    assert nbytes <= 0
    if what == "nine_layers":      # ... and no layout is made of a struct whose layer count runs past its arrays
        assert total <= 0 and count <= 0


def test_eight_layers_are_the_most():
    assert _workspace_bytes(dict(topology=DEFAULT + ((128, 1, 1),) * 2), "bf16")[0] > 0


# ---- the inputs of the earlier fixtures ---------------------------------------------------------------------------------------------------------
# sha256 over (key, shape, dtype, bytes) of every array make_weights / make_noise return, recorded before those functions took a topology and
# network sizes: the fixtures under tests/golden/ were produced from exactly these streams and are not regenerated
STREAMS = {
    "c1_b8_step7001": ("bba0d41deda6a47eeeef15cdc9d03710165677b03df9128fdd770d11490a141e", "4cef26eed47e90aa43bfcf00b6fda7952629603fa0fa70033a4954e9a577d2a3"),
    "lb2_i80_b2_step1": ("2f82293fde584e4c085b8e54d1c6a17694686d8a84b1e8127571246ba1de6399", "91fddde7ef5545daa44198148f2f30666281d34bf87696d84b34c1ced1329fa5"),
    "rgb_c1_b4_step1001": ("c8810c883ed262be1a48b3810530d03eee3fac367efeff264f2ae02a003e4b04", "72e77b3831ff78143d7e0db4b16a5a6186ffe1400bf19073eef04a53f3a20b44"),
    "p24_c1_b4_step1001": ("eca529bf7dc67c339bd22cbd0159c2745c1decf6e24fb7725b07c2a547489bf0", "53968306bd63bffd5a6ee5ec325fae002a87c10d3ff6bbc5de3e7354a22e410d"),
}


def _sha(arrays):
    import hashlib
    m = hashlib.sha256()
    for k, v in arrays.items():
        m.update(k.encode()); m.update(str(v.shape).encode()); m.update(v.dtype.str.encode()); m.update(v.tobytes())
    return m.hexdigest()


@pytest.mark.parametrize("name", list(STREAMS))
def test_input_streams_of_the_earlier_fixtures_did_not_move(name):
    import numpy as np
    from helpers import load_case
    z, c = load_case(name)
    w = gi.make_weights(c["wseed"], c["wscale"], in_chan=c.get("in_chan", 1), lookback=c.get("lookback", 1), obj_px=c.get("obj_px", gi.OBJ_PX))
    noise = gi.make_noise(200 + c["wseed"], c["B"], gi.grid_side(c["I"], c["strides"]))
    assert (_sha(w), _sha(noise)) == STREAMS[name]
    # the generalised entry point gives the same arrays, and they are the ones the committed fixture was made with
    w2, x2, n2 = gi.case_inputs(c)
    assert _sha(w2) == STREAMS[name][0] and _sha(n2) == STREAMS[name][1]
    assert all(np.array_equal(n2[k], z[k]) for k in n2) and np.array_equal(x2, z["x"])
