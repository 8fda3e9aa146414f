"""ctypes binding of libspair_hip.so (C ABI in include/spair_hip.h).

There is NO fallback: if the library is missing or a call returns an error code, a
RuntimeError is raised.  ``import torch`` happens first so that the HIP runtime torch ships
(libamdhip64.so.7) is the one the library binds to -- streams and device pointers are then
shared between torch and these kernels.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede CDLL: see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPAIR_HIP_LIB") or os.path.join(_HERE, "libspair_hip.so")     # the override is for A/B builds of the same ABI

_ERR = {-1: "bad shape", -2: "unsupported dtype", -3: "kernel launch failed", -4: "unsupported configuration",
        -5: "misaligned leading dimension / size"}

_lib = None
ABI_VERSION = 3          # SPAIR_ABI_VERSION (include/spair_hip.h)


class SpairHipError(RuntimeError):
    pass


# mirrors of the structs of include/spair_hip.h (tests/test_abi_layout_cpu.py holds them to the header's sizes and offsets)
class SpairDims(ctypes.Structure):
    """include/spair_hip.h :: SpairDims"""
    _fields_ = [("B", ctypes.c_int), ("C", ctypes.c_int), ("I", ctypes.c_int), ("G", ctypes.c_int),
                ("P", ctypes.c_int), ("A", ctypes.c_int), ("F", ctypes.c_int), ("NP", ctypes.c_int),
                ("n_conv", ctypes.c_int), ("conv_k", ctypes.c_int * 8), ("conv_s", ctypes.c_int * 8),
                ("conv_c", ctypes.c_int * 8), ("pad_pre", ctypes.c_int), ("pad_post", ctypes.c_int),
                ("cell_px", ctypes.c_int), ("dtype", ctypes.c_int), ("align_corners", ctypes.c_int),
                ("anchor", ctypes.c_float), ("max_yx", ctypes.c_float), ("min_yx", ctypes.c_float),
                ("max_hw", ctypes.c_float), ("min_hw", ctypes.c_float), ("obj_logit_scale", ctypes.c_float),
                ("alpha_logit_scale", ctypes.c_float), ("alpha_logit_bias", ctypes.c_float),
                ("vae_beta", ctypes.c_float), ("prior_mean", ctypes.c_float * 6), ("prior_std", ctypes.c_float * 6),
                ("obj_conv", ctypes.c_int), ("oc_n", ctypes.c_int), ("oc_k", ctypes.c_int * 4), ("oc_s", ctypes.c_int * 4),
                ("oc_c", ctypes.c_int * 4), ("lookback", ctypes.c_int),
                ("Iw", ctypes.c_int), ("Gw", ctypes.c_int), ("pad_post_w", ctypes.c_int)]


class SpairStep(ctypes.Structure):
    """include/spair_hip.h :: SpairStep"""
    _fields_ = [("wheel", ctypes.c_float), ("count_prior_prob", ctypes.c_float), ("kl_scale", ctypes.c_float),
                ("train", ctypes.c_int), ("flags", ctypes.c_int), ("draw_noise", ctypes.c_int), ("noise_seed", ctypes.c_uint64),
                ("status", ctypes.c_void_p), ("status_host", ctypes.c_void_p)]


class SpairStepIO(ctypes.Structure):
    """include/spair_hip.h :: SpairStepIO (an unset field is NULL)"""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "params", "x", "eps_box", "eps_attr", "eps_depth", "u_pres", "workspace",
        "loss_out", "recon", "z_where", "z_pres", "inv_den",
        "grad_loss", "grads", "ev_decoder", "ev_cells", "ev_backbone",
        "grad_recon", "grad_z_where", "grad_z_pres", "aux_scratch", "grad_x", "x_scratch")] + [("bce_target", ctypes.c_int)]


_STEP_ARGS = [ctypes.POINTER(SpairDims), ctypes.POINTER(SpairStep), ctypes.POINTER(SpairStepIO), ctypes.c_void_p]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SpairHipError(
                "libspair_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python -m spair_pytorch_amd._build`. There is no CPU/PyTorch fallback." % LIB_PATH)
        h = ctypes.CDLL(LIB_PATH)
        # the structs this package passes must be the ones the library reads: a stale build with a shorter SpairDims would read past
        # the end of the caller's struct
        got = h.spair_abi_version() if hasattr(h, "spair_abi_version") else None
        if got != ABI_VERSION:
            raise SpairHipError("%s has ABI version %s, this package needs %d: rebuild it (python -m spair_pytorch_amd._build)"
                                % (LIB_PATH, got, ABI_VERSION))
        for f, args in ((h.spair_forward, _STEP_ARGS), (h.spair_backward, _STEP_ARGS),
                        (h.spair_step_plan, [ctypes.POINTER(SpairDims), ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int), ctypes.c_int])):
            f.argtypes, f.restype = args, ctypes.c_int
        _declare_parse(h)
        _declare_compose(h)
        _declare_prior(h)
        _declare_evaluate(h)
        _declare_segmentation(h)
        _declare_detection(h)
        _declare_gradnorm(h)
        _lib = h
    return _lib


def _declare_parse(h):
    """Argument lists of the scene-parse entry points (include/spair_hip.h, "scene parse"): they take a float by value."""
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    h.spair_render_owner.argtypes = [vp, i, i, i, vp, vp, vp, vp, f, vp, vp, vp, vp, i, i, i, i, i, i, vp]
    h.spair_parse_owner.argtypes = [ctypes.POINTER(SpairDims), vp, i, f, vp, vp, vp, vp, vp]
    h.spair_cell_rows.argtypes = [ctypes.POINTER(SpairDims), vp, vp, vp]
    for fn in (h.spair_render_owner, h.spair_parse_owner, h.spair_cell_rows):
        fn.restype = i


def _declare_compose(h):
    """Argument lists of the scene-composition entry points (include/spair_hip.h, "scene composition")."""
    vp, i = ctypes.c_void_p, ctypes.c_int
    h.spair_compose.argtypes = [ctypes.POINTER(SpairDims), vp, vp, i, vp, vp, vp, vp, vp, vp, vp]
    h.spair_render_layers.argtypes = [ctypes.POINTER(SpairDims), vp, i, vp, i, vp, vp, vp, vp]
    h.spair_render_layers_rows.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp, i, vp, vp, vp, i, i, i, i, i, i, vp]
    for fn in (h.spair_compose, h.spair_render_layers, h.spair_render_layers_rows):
        fn.restype = i


def _declare_prior(h):
    """Argument lists of the scene-generation entry points (include/spair_hip.h, "scene generation"): a float by value, a 64-bit seed."""
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    h.spair_prior_presence.argtypes = [vp, i, i, f, vp, vp, vp, vp, vp]
    h.spair_prior_sample.argtypes = [ctypes.POINTER(SpairDims), f, vp] + [vp] * 11
    h.spair_noise_fill.argtypes = [ctypes.POINTER(SpairDims), ctypes.c_uint64, vp, vp, vp, vp, vp]
    for fn in (h.spair_prior_presence, h.spair_prior_sample, h.spair_noise_fill):
        fn.restype = i


def _declare_evaluate(h):
    """Argument lists of the evaluation entry points (include/spair_hip.h, "evaluation"): floats by value, a 64-bit count returned."""
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    h.spair_sample_terms_scratch_floats.argtypes = [i, i, i, i]
    h.spair_sample_terms_scratch_floats.restype = ctypes.c_longlong
    h.spair_sample_terms_rows.argtypes = [vp, i] * 8 + [vp, vp, vp, f, vp, vp] + [i] * 6 + [vp, vp, vp, vp, i, f, vp]
    h.spair_eval_terms.argtypes = [ctypes.POINTER(SpairDims), vp, i, vp, vp, f, vp, vp, vp, vp, i, f, vp]
    for fn in (h.spair_sample_terms_rows, h.spair_eval_terms):
        fn.restype = i


def _declare_segmentation(h):
    """Argument lists of the instance-mask and segmentation-metric entry points (include/spair_hip.h): 64-bit seed, first sample, HW."""
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    h.spair_scenes_generate_masks.argtypes = [ctypes.c_uint64, ll, i, i, i, i, i, vp, vp, vp, vp, vp, vp]
    h.spair_segmentation.argtypes = [vp, vp, i, ll, i, i, vp, vp, vp, vp, vp]
    for fn in (h.spair_scenes_generate_masks, h.spair_segmentation):
        fn.restype = i


def _declare_detection(h):
    """Argument lists of the detection-metric entry points (include/spair_hip.h, "detection metrics"): a float by value, a 64-bit count."""
    vp, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    h.spair_det_match.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, f, i, vp, vp, vp, vp, vp, vp, vp, vp]
    h.spair_det_ap.argtypes = [vp, ll, i, vp, vp, vp]
    for fn in (h.spair_det_match, h.spair_det_ap):
        fn.restype = i


def _declare_gradnorm(h):
    """Argument lists of the gradient-norm and clipped-Adam entry points (include/spair_hip.h, "gradient norm and clipping"): floats by
    value, 64-bit counts."""
    vp, i, f, ll, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_int64
    h.spair_grad_chunk.argtypes = []
    h.spair_grad_norm_items.argtypes = [vp, vp, i, i64, vp]
    h.spair_grad_norm_items.restype = ll
    h.spair_grad_norm.argtypes = [vp, vp, ll, i, vp, vp, vp, f, f, vp, vp]
    h.spair_adam_clipped.argtypes = [vp, vp, vp, vp, i64, f, f, f, f, i, vp, vp, vp, vp]
    for fn in (h.spair_grad_chunk, h.spair_grad_norm, h.spair_adam_clipped):
        fn.restype = i
    h.spair_status_exchange.argtypes = [vp, vp, vp, i, vp]
    h.spair_status_exchange.restype = i


def check(rc, what):
    if rc != 0:
        raise SpairHipError("%s failed: %s (code %d)" % (what, _ERR.get(rc, "unknown"), rc))


def ptr(t):
    """Device pointer of a (contiguous-enough) torch tensor, or NULL for None."""
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


RENDER_FAMILIES = ("MMA", "GEN2", "GEN1", "COLOUR")     # SPAIR_RENDER_* (include/spair_hip.h)


def step_plan(dims, workspace, flags=0):
    """spair_step_plan: the kernels a step with these SpairDims, workspace address (an int; never read) and SpairStep.flags runs, as
    {fwd, bwd: a name of RENDER_FAMILIES; rec, s16, g16, chain, dec_fused: bool}.  Host only: no GPU is needed."""
    out = (ctypes.c_int * 8)()
    check(lib().spair_step_plan(ctypes.byref(dims), int(workspace), int(flags), 0, out, 8), "spair_step_plan")
    return dict(fwd=RENDER_FAMILIES[out[0]], bwd=RENDER_FAMILIES[out[1]], rec=bool(out[2]), s16=bool(out[3]), g16=bool(out[4]),
                chain=bool(out[5]), dec_fused=bool(out[6]))


CONV_KERNELS = ("GEMM", "PATCH", "PER_CLASS", "PW_STACK")      # SPAIR_CONV_*
STEM_WGRADS = ("PATCH", "GEMM", "WGRAD16", "GENERIC")          # SPAIR_STEM_*
STEP_PLAN_INTS = 38                                            # SPAIR_STEP_PLAN_INTS


def step_plan_n(dims, workspace, flags=0, input_grad=False):
    """spair_step_plan: the rest of the plan step_plan reports, for a step with these SpairDims, workspace address, SpairStep.flags and
    (backward) image gradient, as {side, dec_dgrad_fused, dec_wgrad_grouped, dec_wgrad_late: bool; pw0: first layer of the fused 1x1 stack
    (n_conv + 1: none); stem: where the stem's weight gradient is taken, a name of STEM_WGRADS; fwd, dgrad: per backbone layer 1 .. n_conv
    (conv_out last) a name of CONV_KERNELS; gate_bits: per layer, whether its data gradient reads the sign bits the layer below left}."""
    out = (ctypes.c_int * STEP_PLAN_INTS)()
    check(lib().spair_step_plan(ctypes.byref(dims), int(workspace), int(flags), int(bool(input_grad)), out, STEP_PLAN_INTS),
          "spair_step_plan")
    layers = range(dims.n_conv)
    return dict(side=bool(out[8]), dec_dgrad_fused=bool(out[9]), dec_wgrad_grouped=bool(out[10]), dec_wgrad_late=bool(out[11]), pw0=out[12],
                stem=STEM_WGRADS[out[13]], fwd=tuple(CONV_KERNELS[out[14 + i]] for i in layers),
                dgrad=tuple(CONV_KERNELS[out[22 + i]] for i in layers), gate_bits=tuple(bool(out[30 + i]) for i in layers))


VIEW_DTYPES = (torch.float32, torch.bfloat16, torch.float16)     # spair_workspace_view's element types 0, 1, 2


def workspace_view_names(dims):
    """Every buffer name spair_workspace_view resolves on these SpairDims (the buffers their workspace allocates).  Host only."""
    f, buf, names = lib().spair_workspace_view_name, ctypes.create_string_buffer(128), []
    while f(ctypes.byref(dims), len(names), buf, 128) == 0:
        names.append(buf.value.decode())
    return names


def workspace_view(dims, workspace, name, flags=0, input_grad=False):
    """spair_workspace_view: where buffer ``name`` lies in a workspace at address ``workspace`` (an int; never read) for the step plan of
    SpairStep.flags ``flags`` and an image gradient or not, as {offset (bytes), rows, cols, ld (elements), dtype (a torch dtype), written}.
    Host only: no GPU is needed."""
    out = (ctypes.c_longlong * 6)()
    check(lib().spair_workspace_view(ctypes.byref(dims), ctypes.c_void_p(int(workspace)), int(flags), int(bool(input_grad)),
                                     name.encode(), out), "spair_workspace_view(%s)" % name)
    return dict(offset=out[0], rows=out[1], cols=out[2], ld=out[3], dtype=VIEW_DTYPES[out[4]], written=bool(out[5]))


def render_owner(sprites, channels, nbox, pres, depth, B, HW, I, Iw, P, align_corners=False, threshold=0.5, cell_rows=None):
    """spair_render_owner on torch tensors: ``sprites`` [B*HW, >= P*P*channels] fp16 or fp32 (its row stride is the leading dimension),
    ``channels`` elements per texel with alpha last, ``nbox`` [B*HW, 4], ``pres`` / ``depth`` [B*HW]; cell k of sample b is row
    ``(cell_rows[k] if cell_rows is not None else k) * B + b``.  Returns (owner int32 [B,I,Iw], owner_weight, coverage fp32 [B,I,Iw],
    area int32 [B,HW])."""
    if sprites.dtype not in (torch.float16, torch.float32) or sprites.stride(1) != 1:
        raise SpairHipError("sprites must be fp16 or fp32 rows")
    dev = sprites.device
    owner = torch.empty(B, I, Iw, device=dev, dtype=torch.int32)
    weight, cover = (torch.empty(B, I, Iw, device=dev, dtype=torch.float32) for _ in range(2))
    area = torch.empty(B, HW, device=dev, dtype=torch.int32)
    nbox, pres, depth = (t.contiguous().float() for t in (nbox, pres, depth))
    rows = None if cell_rows is None else cell_rows.to(device=dev, dtype=torch.int32).contiguous()
    if sprites.shape[0] != B * HW or nbox.numel() != 4 * B * HW or pres.numel() != B * HW or depth.numel() != B * HW or \
            (rows is not None and rows.numel() != HW):
        raise SpairHipError("render_owner: operands do not have B * HW rows")
    check(lib().spair_render_owner(ptr(sprites), int(sprites.stride(0)), int(sprites.dtype == torch.float16), int(channels), ptr(nbox),
                                   ptr(pres), ptr(depth), ptr(rows), float(threshold), ptr(owner), ptr(weight), ptr(cover), ptr(area),
                                   int(B), int(HW), int(I), int(Iw), int(P), int(bool(align_corners)), stream()), "spair_render_owner")
    return owner, weight, cover, area


def render_layers(sprites, channels, nbox, pres, depth, cells, inv_den, B, HW, I, Iw, P, align_corners=False, cell_rows=None):
    """spair_render_layers_rows on torch tensors: operands as for ``render_owner``; ``cells`` int [B,K] (row-major cell index, anything
    outside [0, HW) = an all-zero layer), ``inv_den`` fp32 [B,I,Iw] (the composite's 1/D per pixel).  Returns (layers fp32
    [B,K,channels-1,I,Iw], layer_weight fp32 [B,K,I,Iw])."""
    if sprites.dtype not in (torch.float16, torch.float32) or sprites.stride(1) != 1:
        raise SpairHipError("sprites must be fp16 or fp32 rows")
    dev = sprites.device
    cells = cells.to(device=dev, dtype=torch.int32).contiguous()
    K = int(cells.shape[1])
    nbox, pres, depth, inv_den = (t.contiguous().float() for t in (nbox, pres, depth, inv_den))
    rows = None if cell_rows is None else cell_rows.to(device=dev, dtype=torch.int32).contiguous()
    if sprites.shape[0] != B * HW or nbox.numel() != 4 * B * HW or pres.numel() != B * HW or depth.numel() != B * HW or \
            cells.shape[0] != B or inv_den.numel() != B * I * Iw or (rows is not None and rows.numel() != HW):
        raise SpairHipError("render_layers: operands do not have B * HW rows / B * I * Iw pixels")
    layers = torch.empty(B, K, int(channels) - 1, I, Iw, device=dev, dtype=torch.float32)
    weight = torch.empty(B, K, I, Iw, device=dev, dtype=torch.float32)
    check(lib().spair_render_layers_rows(ptr(sprites), int(sprites.stride(0)), int(sprites.dtype == torch.float16), int(channels), ptr(nbox),
                                         ptr(pres), ptr(depth), ptr(rows), ptr(cells), K, ptr(inv_den), ptr(layers), ptr(weight), int(B),
                                         int(HW), int(I), int(Iw), int(P), int(bool(align_corners)), stream()), "spair_render_layers_rows")
    return layers, weight


def prior_presence(u, prob, count=None):
    """spair_prior_presence on torch tensors: ``u`` fp32 [B,HW] uniform draws in [0, 1) on the device, ``prob`` the count prior's
    probability (strictly inside (0, 1); not read when ``count`` is given), ``count`` None, an int or an int tensor [B]: that many
    objects exactly, clamped to [0, HW].  Returns (z_pres fp32 [B,HW], hard; p_z fp32 [B,HW]; n_present int32 [B])."""
    if not u.is_cuda or u.dim() != 2:
        raise SpairHipError("prior_presence: u must be a [B,HW] tensor on the MI355X")
    u = u.contiguous().float()
    B, HW = (int(v) for v in u.shape)
    dev = u.device
    if count is not None:
        if torch.is_tensor(count):
            count = count.to(device=dev).clamp(-1, HW + 1).to(torch.int32).contiguous()
        else:
            count = torch.full((B,), max(-1, min(int(count), HW + 1)), device=dev, dtype=torch.int32)
        if count.numel() != B:
            raise SpairHipError("prior_presence: count must hold B values")
    z = torch.empty(B, HW, device=dev, dtype=torch.float32)
    pz = torch.empty(B, HW, device=dev, dtype=torch.float32)
    n = torch.empty(B, device=dev, dtype=torch.int32)
    check(lib().spair_prior_presence(ptr(u), B, HW, float(prob), ptr(count), ptr(z), ptr(pz), ptr(n), stream()), "spair_prior_presence")
    return z, pz, n


def sample_terms(z_pres, p_z, mu_box, sd_box, mu_attr, sd_attr, mu_depth, sd_depth, priors, beta, recon, x, rows=None, maps=True,
                 out=None, accumulate=False, scale=1.0):
    """spair_sample_terms_rows on torch tensors.  Per-row operands: 2-D fp32 device tensors [N, cols] with N = HW * B rows
    (row = rows[k] * B + b for cell k, ``rows`` an int32 [HW] tensor or None = identity) and unit stride along the columns -- a column
    slice of a wider buffer is fine, its row stride is passed as the leading dimension; z_pres / p_z / mu_depth / sd_depth one column,
    mu_box / sd_box four (cy, cx, height, width), mu_attr / sd_attr A.  ``priors``: six (mean, std).  recon, x fp32 [B,C,I,Iw].
    Returns (terms [B,9], kl_map [B,7,HW] or None, bce_map [B,I,Iw] or None); ``out`` = such a triple to write into (with
    ``accumulate`` / ``scale``: map = (accumulate ? map : 0) + scale * value)."""
    ops = (z_pres, p_z, mu_box, sd_box, mu_attr, sd_attr, mu_depth, sd_depth)
    for t in ops + (recon, x):
        if not t.is_cuda or t.dtype != torch.float32:
            raise SpairHipError("sample_terms: fp32 tensors on the MI355X")
    for t in ops:
        if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise SpairHipError("sample_terms: per-row operands are [N, cols] with unit column stride")
    recon, x = recon.contiguous(), x.contiguous()
    B, C, I, Iw = (int(v) for v in x.shape)
    A = int(mu_attr.shape[1])
    HW = int(z_pres.shape[0]) // B
    if any(int(t.shape[0]) != HW * B for t in ops) or tuple(recon.shape) != tuple(x.shape):
        raise SpairHipError("sample_terms: inconsistent shapes")
    dev = x.device
    if rows is not None:
        rows = rows.to(device=dev, dtype=torch.int32).contiguous()
    if out is None:
        out = (torch.empty(B, 9, device=dev), torch.empty(B, 7, HW, device=dev) if maps else None,
               torch.empty(B, I, Iw, device=dev) if maps else None)
    terms, kl_map, bce_map = out
    n = int(lib().spair_sample_terms_scratch_floats(B, HW, I, Iw))
    if n <= 0:
        raise SpairHipError("sample_terms: unsupported shape (B=%d, HW=%d, image %dx%d)" % (B, HW, I, Iw))
    scratch = torch.empty(n, device=dev, dtype=torch.float32)
    pm = (ctypes.c_float * 6)(*(float(m) for m, _ in priors))
    ps = (ctypes.c_float * 6)(*(float(s) for _, s in priors))
    args = []
    for t in ops:
        args += [ptr(t), int(t.stride(0))]
    check(lib().spair_sample_terms_rows(*args, ptr(rows), ctypes.cast(pm, ctypes.c_void_p), ctypes.cast(ps, ctypes.c_void_p), float(beta),
                                        ptr(recon), ptr(x), B, HW, A, C, I, Iw, ptr(terms), ptr(kl_map), ptr(bce_map), ptr(scratch),
                                        int(bool(accumulate)), float(scale), stream()), "spair_sample_terms_rows")
    return terms, kl_map, bce_map
