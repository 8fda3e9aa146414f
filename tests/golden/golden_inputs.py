"""Deterministic (numpy-Generator) inputs shared by the golden-vector generator and the tests.

Nothing here touches the reference.  numpy's ``default_rng`` (PCG64) streams are stable
across numpy versions and platforms, so weights / noise / images can be regenerated on the
GPU box from a seed instead of being shipped as megabytes of fixture.

Shapes and key names follow the reference's ``state_dict`` (SURVEY.md §8(b);
/root/reference/spair/models.py:133-167, modules.py:43-66,124-165).
"""
import math

import numpy as np

N_BACKBONE_FEATURES = 100
N_PASSTHROUGH = 100
N_ATTR = 50
OBJ_PX = 28
CONTEXT_DIM = 4 * (4 + N_ATTR + 1 + 1)  # 224 (N_LOOKBACK = 1)


def context_dim(lookback=1, n_attr=N_ATTR):
    """models.py:26: ((2L+1)^2 // 2) records of 4 + A + 2."""
    return (2 * lookback + 1) ** 2 // 2 * (4 + n_attr + 1 + 1)


def param_shapes(in_chan=1, conv_kernels=(4, 4, 4, 1, 1, 1), filters=128, lookback=1, obj_px=OBJ_PX, n_features=N_BACKBONE_FEATURES,
                 n_passthrough=N_PASSTHROUGH, n_attr=N_ATTR):
    """Ordered {key: shape} for every tensor of the reference state_dict.  ``filters``: one count for every backbone layer, or one per
    layer (config.py:7-14 DEFAULT_BACKBONE_TOPOLOGY); ``n_features`` / ``n_passthrough`` / ``n_attr``: config.py:22,24,27."""
    N_BACKBONE_FEATURES, N_PASSTHROUGH, N_ATTR = n_features, n_passthrough, n_attr
    if isinstance(filters, int):
        filters = (filters,) * len(conv_kernels)
    assert len(filters) == len(conv_kernels)
    s = {}
    s["virtual_edge_element"] = (4 + N_ATTR + 2,)
    prev = in_chan
    for i, (f, k) in enumerate(zip(filters, conv_kernels)):
        s[f"backbone.net.conv_{i}.weight"] = (f, prev, k, k)
        s[f"backbone.net.conv_{i}.bias"] = (f,)
        prev = f
    s["backbone.net.conv_out.weight"] = (N_BACKBONE_FEATURES, prev, 1, 1)
    s["backbone.net.conv_out.bias"] = (N_BACKBONE_FEATURES,)

    def mlp(prefix, n_in, hidden, outs, multi):
        p = n_in
        body = prefix + (".body" if multi else "")
        for i, h in enumerate(hidden):
            s[f"{body}.dense{i}.weight"] = (h, p)
            s[f"{body}.dense{i}.bias"] = (h,)
            p = h
        if multi:
            for i, o in enumerate(outs):
                s[f"{prefix}.output_layers.{i}.weight"] = (o, p)
                s[f"{prefix}.output_layers.{i}.bias"] = (o,)
        else:
            s[f"{prefix}.out.weight"] = (outs, p)
            s[f"{prefix}.out.bias"] = (outs,)

    CONTEXT_DIM = context_dim(lookback, N_ATTR)
    box_in = N_BACKBONE_FEATURES + CONTEXT_DIM
    mlp("box_network", box_in, (100, 100), (8, N_PASSTHROUGH), True)
    mlp("object_encoder", obj_px * obj_px * in_chan, (256, 128), 2 * N_ATTR, False)
    z_in = 4 + N_ATTR + N_PASSTHROUGH + CONTEXT_DIM + N_BACKBONE_FEATURES
    mlp("z_network", z_in, (100, 100), (2, N_PASSTHROUGH), True)
    mlp("obj_network", z_in + 1, (100, 100), 1, False)
    mlp("object_decoder", N_ATTR, (128, 256), obj_px * obj_px * (in_chan + 1), False)
    # the dead Self_Attn over one context record without its presence: 4 + A + 1 channels (models.py:167 writes the 55 of A = 50 out; the
    # reference cannot be built with another A, the engine's parameter layout follows the formula)
    ad = 4 + N_ATTR + 1
    s["attn.gamma"] = (1,)
    for nm, o in (("query", ad // 8), ("key", ad // 8), ("value", ad)):
        s[f"attn.{nm}_conv.weight"] = (o, ad, 1, 1)
        s[f"attn.{nm}_conv.bias"] = (o,)
    return s


def make_weights(seed, scale=1.0, in_chan=1, lookback=1, obj_px=OBJ_PX, **net):
    """U(-1/sqrt(fan_in), 1/sqrt(fan_in)) * scale per tensor (PyTorch-default-like
    magnitude), float32.  Returns {key: np.ndarray}.  ``net``: param_shapes' conv_kernels / filters / n_features / n_passthrough / n_attr
    (default: the reference's network, whose streams every earlier fixture was drawn from)."""
    rng = np.random.default_rng(seed)
    out = {}
    shapes = param_shapes(in_chan, lookback=lookback, obj_px=obj_px, **net)
    for key, shp in shapes.items():
        if key == "virtual_edge_element":
            t = rng.standard_normal(shp).astype(np.float32)
            sig = lambda v: 1.0 / (1.0 + np.exp(-v))
            t[:4] = sig(t[:4])
            t[-2:] = sig(t[-2:])
            out[key] = t.astype(np.float32)
            continue
        if key == "attn.gamma":
            out[key] = np.zeros(shp, np.float32)
            continue
        if key.endswith(".weight"):
            fan_in = int(np.prod(shp[1:]))
        else:
            fan_in = int(np.prod(shapes[key[:-4] + "weight"][1:]))
        bound = scale / math.sqrt(fan_in)
        out[key] = rng.uniform(-bound, bound, size=shp).astype(np.float32)
    return out


def make_noise(seed, B, G, n_attr=N_ATTR):
    """The 7 per-cell draws of the reference (models.py:333-336,84,95,402-403), laid out
    as maps.  eps_box channel order = draw order (cy, cx, height, width)."""
    N_ATTR = n_attr
    rng = np.random.default_rng(seed)
    return dict(
        eps_box=rng.standard_normal((B, 4, G, G)).astype(np.float32),
        eps_attr=rng.standard_normal((B, N_ATTR, G, G)).astype(np.float32),
        eps_depth=rng.standard_normal((B, 1, G, G)).astype(np.float32),
        u_pres=rng.uniform(0.0, 1.0, (B, 1, G, G)).astype(np.float32),
    )


def make_image(seed, B, I, max_objects, in_chan=1):
    """Small stand-in for scattered MNIST: k ~ U{0..max_objects} anti-aliased stroke
    blobs of 14..28 px on black, max-composited, values in [0,1]."""
    rng = np.random.default_rng(seed)
    img = np.zeros((B, in_chan, I, I), np.float32)
    yy, xx = np.mgrid[0:I, 0:I].astype(np.float32)
    for b in range(B):
        k = int(rng.integers(0, max_objects + 1))
        for _ in range(k):
            size = float(rng.uniform(14, 28))
            cy, cx = rng.uniform(size / 2, I - size / 2, 2)
            # a "stroke": a ring segment or a bar, softly anti-aliased
            if rng.uniform() < 0.5:
                r = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
                glyph = np.clip(1.5 - np.abs(r - size * 0.3) / 1.5, 0, 1)
            else:
                ang = rng.uniform(0, np.pi)
                d = np.abs((yy - cy) * np.cos(ang) - (xx - cx) * np.sin(ang))
                along = np.abs((yy - cy) * np.sin(ang) + (xx - cx) * np.cos(ang))
                glyph = np.clip(1.5 - d / 1.5, 0, 1) * (along < size * 0.45)
            # colour images: one random colour per object (drawn only then: the greyscale streams are unchanged)
            col = rng.uniform(0.25, 1.0, in_chan).astype(np.float32) if in_chan > 1 else np.ones(1, np.float32)
            for c in range(in_chan):
                img[b, c] = np.maximum(img[b, c], col[c] * glyph.astype(np.float32))
    return img


# name -> dict(I, strides, B, step, wseed, wscale, max_objects)
CASES = {
    # BASELINE.json configs[0]: 48x48, 6x6 grid, batch 16 (wheel on / off / sharp count prior)
    "c1_b16_step1": dict(I=48, strides=(2, 2, 2, 1, 1, 1), B=16, step=1, wseed=11, wscale=1.0, max_objects=3),
    "c1_b8_step1001": dict(I=48, strides=(2, 2, 2, 1, 1, 1), B=8, step=1001, wseed=11, wscale=1.0, max_objects=3),
    "c1_b8_step7001": dict(I=48, strides=(2, 2, 2, 1, 1, 1), B=8, step=7001, wseed=12, wscale=2.0, max_objects=3),
    # configs[1] geometry (128x128, 16x16 grid) as a B=2 slice
    "c2_b2_step1001": dict(I=128, strides=(2, 2, 2, 1, 1, 1), B=2, step=1001, wseed=13, wscale=1.0, max_objects=11),
    # the reference's own default topology (strides 3,2,2 -> 11x11 grid, config.py:7-14)
    "ref_default_b2_step1001": dict(I=128, strides=(3, 2, 2, 1, 1, 1), B=2, step=1001, wseed=14, wscale=1.5, max_objects=11),
    # configs[3] geometry (256x256, 32x32 grid) as a B=1 slice
    "c4_b1_step1001": dict(I=256, strides=(2, 2, 2, 1, 1, 1), B=1, step=1001, wseed=15, wscale=1.0, max_objects=11),
}
# N_LOOKBACK = 2 (config.py:31; 12 context neighbours, models.py:292-320): kept apart from CASES -- the fused bf16 kernels are built for
# N_LOOKBACK = 1, these run on the per-wavefront launches (tests/test_lookback_gpu.py)
LOOKBACK_CASES = {
    "lb2_c1_b4_step1001": dict(I=48, strides=(2, 2, 2, 1, 1, 1), B=4, step=1001, wseed=16, wscale=1.0, max_objects=3, lookback=2),
    "lb2_i80_b2_step1": dict(I=80, strides=(2, 2, 2, 1, 1, 1), B=2, step=1, wseed=17, wscale=1.5, max_objects=5, lookback=2),
    "lb3_c1_b3_step7001": dict(I=48, strides=(2, 2, 2, 1, 1, 1), B=3, step=7001, wseed=18, wscale=1.0, max_objects=3, lookback=3),
}
# colour images (config.py:4 INPUT_IMAGE_SHAPE[0] = 3; models.py:150,163,480,524, modules.py:24,239): the fp32 per-wavefront step with the
# generic-channel renderer (tests/test_rgb_gpu.py)
RGB_CASES = {
    "rgb_c1_b4_step1001": dict(I=48, strides=(2, 2, 2, 1, 1, 1), B=4, step=1001, wseed=21, wscale=1.0, max_objects=3, in_chan=3),
    "rgb_i80_b2_step1": dict(I=80, strides=(2, 2, 2, 1, 1, 1), B=2, step=1, wseed=22, wscale=1.5, max_objects=5, in_chan=3),
}


# other object sizes (config.py:33 OBJECT_SHAPE; models.py:149,387,462): the renderer's fallback families and the decoder at 36 / 64 column
# pairs (tests/test_object_geometry_gpu.py)
OBJ_CASES = {
    "p24_c1_b4_step1001": dict(I=48, strides=(2, 2, 2, 1, 1, 1), B=4, step=1001, wseed=23, wscale=1.0, max_objects=3, obj_px=24),
    "p32_i64_b2_step1": dict(I=64, strides=(2, 2, 2, 1, 1, 1), B=2, step=1, wseed=24, wscale=1.0, max_objects=4, obj_px=32),
}


# other backbone topologies and network sizes (config.py:7-14 DEFAULT_BACKBONE_TOPOLOGY, :22 N_BACKBONE_FEATURES, :24 N_PASSTHROUGH_FEATURES):
# `topology` = (filters, kernel, stride) per layer, F / NP / A = features / passthrough / attributes; what is absent is the default network
# (tests/test_topology_cpu.py pins the kernels each one runs, tests/test_topology_gpu.py runs them)
_S2 = (2, 2, 2, 1, 1, 1)
TOPO_CASES = {
    "t_shallow64": dict(I=32, topology=((64, 4, 2), (64, 4, 2), (64, 1, 1)), B=4, step=1001, wseed=31, wscale=1.0, max_objects=3),
    "t_k3": dict(I=48, topology=((128, 3, 2), (128, 3, 1), (128, 2, 2), (128, 1, 1), (128, 1, 1)), B=2, step=1001, wseed=32, wscale=1.0,
                 max_objects=3),
    "t_k6": dict(I=48, topology=((128, 4, 2), (128, 6, 2), (128, 4, 2), (128, 1, 1)), B=4, step=1001, wseed=33, wscale=1.0, max_objects=3),
    "t_nostack": dict(I=48, topology=((128, 4, 2), (128, 4, 2), (128, 4, 2)), B=4, step=1001, wseed=34, wscale=1.0, max_objects=3),
    "t_deep8": dict(I=48, topology=((32, 4, 2), (64, 4, 2), (128, 4, 2), (128, 1, 1), (72, 1, 1), (128, 1, 1), (128, 1, 1), (128, 1, 1)),
                    B=2, step=1001, wseed=35, wscale=1.0, max_objects=3),
    # (wseed 36 put one decoder hidden unit's pre-activation 9e-9 from its ReLU kink, inside fp32 summation-order noise: which side it falls on,
    # and with it that unit's gradient, is then decided by the order of a sum, not by the model -- the other cases' smallest is 6e-7 .. 8e-5)
    "t_stack5": dict(I=32, topology=((128, 4, 2), (128, 4, 2)) + ((128, 1, 1),) * 4, B=4, step=1001, wseed=45, wscale=1.0, max_objects=3),
    "t_stem5": dict(I=48, topology=((128, 5, 4), (128, 2, 2), (128, 1, 1)), B=4, step=1001, wseed=37, wscale=1.0, max_objects=3),
    "t_feat64": dict(I=48, strides=_S2, F=64, NP=36, B=4, step=1001, wseed=38, wscale=1.0, max_objects=3),
    "t_feat128": dict(I=48, strides=_S2, F=128, NP=64, B=4, step=1001, wseed=39, wscale=1.0, max_objects=3),
}
# N_ATTRIBUTES other than 50 (config.py:27): the reference cannot run them (models.py:66,167 write 55 context channels out), so there is no
# fixture -- the oracle, pinned to the reference on every other case, stands in for it (tests/test_topology_gpu.py)
ORACLE_CASES = {
    "o_attr16": dict(I=48, strides=_S2, A=16, B=4, step=1001, wseed=40, wscale=1.0, max_objects=3),
    "o_attr59": dict(I=48, strides=_S2, A=59, B=2, step=1001, wseed=41, wscale=1.0, max_objects=3),
}


def all_cases():
    d = dict(CASES)
    d.update(LOOKBACK_CASES)
    d.update(RGB_CASES)
    d.update(OBJ_CASES)
    d.update(TOPO_CASES)
    return d


def case_topology(case):
    """(filters, kernel, stride) per backbone layer of a case: its `topology`, or the default network with the case's strides."""
    if "topology" in case:
        return tuple(tuple(int(v) for v in layer) for layer in case["topology"])
    return tuple((128, k, int(s)) for k, s in zip((4, 4, 4, 1, 1, 1), case["strides"]))


def case_net(case):
    """The keyword arguments of param_shapes / make_weights that a case's topology and sizes stand for."""
    topo = case_topology(case)
    return dict(conv_kernels=tuple(k for _, k, _ in topo), filters=tuple(f for f, _, _ in topo), n_features=case.get("F", N_BACKBONE_FEATURES),
                n_passthrough=case.get("NP", N_PASSTHROUGH), n_attr=case.get("A", N_ATTR))


def case_strides(case):
    return tuple(s for _, _, s in case_topology(case))


def case_grid(case):
    return grid_side(case["I"], case_strides(case))


def case_inputs(case):
    """(weights, image, noise) of a case, as make_golden.py feeds them to the reference."""
    w = make_weights(case["wseed"], case["wscale"], in_chan=case.get("in_chan", 1), lookback=case.get("lookback", 1),
                     obj_px=case.get("obj_px", OBJ_PX), **case_net(case))
    x = make_image(100 + case["wseed"], case["B"], case["I"], case["max_objects"], in_chan=case.get("in_chan", 1))
    noise = make_noise(200 + case["wseed"], case["B"], case_grid(case), n_attr=case.get("A", N_ATTR))
    return w, x, noise


def grid_side(I, strides, kernels=None):
    """Cells per side: ceil(I / product of the strides) (modules.py:68-105; the kernels only move the padding)."""
    cell = 1
    for s in strides:
        cell *= s
    return int(math.ceil(I / cell))
