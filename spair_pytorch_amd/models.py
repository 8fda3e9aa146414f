"""``SPAIR`` -- drop-in for /root/reference/spair/models.py:15-131 on an MI355X.

Same constructor ``SPAIR(image_shape, writer, device)``, same ``forward(x, global_step=0) ->
(loss, recon_x, z_where, z_pres)``, same ``state_dict`` keys and ``spair.config``
hyper-parameters, so the reference's train.py loop (zero_grad / forward / backward / Adam
step, train.py:64-67) runs unchanged.  All arithmetic of the step is in libspair_hip.so
(hand-written gfx950 kernels behind the C ABI of include/spair_hip.h):

* parameters live in ONE flat fp32 device buffer (each nn.Parameter is a view into it), the
  gradients in a second one -- what the RCCL all-reduce and the fused Adam operate on;
* ``forward`` enqueues ``spair_forward`` (backbone -> 3G-2 dependency wavefronts of the
  per-cell encoder -> decoder -> fused inverse-STN compositor -> KL/loss); ``loss.backward()``
  enqueues ``spair_backward`` (hand-written reverse pass) which accumulates into ``p.grad``;
* with ``differentiable_outputs=True`` the recon / z_where / z_pres outputs are autograd tensors
  too, as in the reference: adjoints that reach them are folded into that same reverse pass
  (``SpairStepIO.inv_den`` / ``grad_recon`` / ``grad_z_where`` / ``grad_z_pres``);
* an input ``x`` that requires grad gets the reference's ``x.grad`` (``SpairStepIO.grad_x``): the
  backbone, glimpse and BCE-target terms.  As in torch, the BCE-target term is ``-logit(recon)``
  unclamped: ``x.grad`` is +inf wherever recon is exactly 0 (-inf where it is exactly 1);
* there is no PyTorch/CPU fallback: without the HIP library or a GPU this module raises.
"""
import ctypes
import os
import math
import weakref

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import config as cfg
from ._lib import SpairDims, SpairStep  # noqa: F401  (the C structs' mirrors; exported here as before)
from .modules import Backbone, ObjectConvDecoder, ObjectConvEncoder, build_MLP, exponential_decay

DIST_NAMES = ['cy_logit', 'cx_logit', 'height_logit', 'width_logit', 'attr', 'depth_logit']
NOISE_MAPS = ('eps_box', 'eps_attr', 'eps_depth', 'u_pres')


# bit 0: disable the fused persistent per-cell kernels (tests compare both paths); bit 1: stage stamps; bit 2: no helper stream
STEP_FLAGS = int(os.environ.get("SPAIR_STEP_FLAGS", "0"))

_DTYPES = {'f32': 0, 'fp32': 0, 'float32': 0, 'bf16': 1, 'bfloat16': 1}


def make_dims(batch, image_shape, topology, dtype=None, object_conv_topology=None, lookback=1):
    """``object_conv_topology``: the layer list of the convolutional object encoder / decoder variant (``None`` = the MLP pair).
    ``image_shape`` = [C, H, W]; H != W is a rectangular image (I, G, pad_post: the height axis; Iw, Gw, pad_post_w: the width axis)."""
    from .modules import backbone_geometry, _topology_conv_args
    d = SpairDims()
    C, I, Iw = (int(v) for v in image_shape)
    pre, post, G, cell, _ = backbone_geometry(I, topology)
    pre_w, post_w, Gw, cell_w, _ = backbone_geometry(Iw, topology)
    assert (pre_w, cell_w) == (pre, cell)
    d.B, d.C, d.I, d.G = int(batch), int(C), int(I), int(G)
    if Iw != I:      # (square: the three width fields stay 0 = "the same as I, G, pad_post", the C ABI's square meaning)
        d.Iw, d.Gw, d.pad_post_w = Iw, int(Gw), int(post_w)
    d.P, d.A, d.F, d.NP = int(cfg.OBJECT_SHAPE[0]), int(cfg.N_ATTRIBUTES), int(cfg.N_BACKBONE_FEATURES), int(cfg.N_PASSTHROUGH_FEATURES)
    # (a topology longer than the struct's per-layer arrays keeps its count: the library refuses it -- spair_workspace_bytes <= 0 -- as it
    # refuses any other configuration it does not run)
    d.n_conv = len(topology)
    for i, layer in enumerate(topology[:len(d.conv_k)]):
        d.conv_k[i], d.conv_s[i] = int(layer['kernel_size']), int(layer['stride'])
        d.conv_c[i] = int(layer.get('filters', layer.get('out_channels')))
    d.pad_pre, d.pad_post, d.cell_px = pre, post, cell
    d.dtype = _DTYPES[(dtype or cfg.COMPUTE_DTYPE).lower()]
    d.align_corners = int(bool(cfg.ALIGN_CORNERS))
    d.anchor = float(cfg.ANCHORBOX_SHAPE[0])
    d.max_yx, d.min_yx, d.max_hw, d.min_hw = cfg.MAX_YX, cfg.MIN_YX, cfg.MAX_HW, cfg.MIN_HW
    d.obj_logit_scale, d.alpha_logit_scale, d.alpha_logit_bias = cfg.OBJ_LOGIT_SCALE, cfg.ALPHA_LOGIT_SCALE, cfg.ALPHA_LOGIT_BIAS
    d.vae_beta = float(cfg.VAE_BETA)
    for i, n in enumerate(DIST_NAMES):
        d.prior_mean[i], d.prior_std[i] = float(cfg.PRIORS[n][0]), float(cfg.PRIORS[n][1])
    d.lookback = int(lookback)
    if object_conv_topology is not None:
        if len(object_conv_topology) > 4:
            raise L.SpairHipError("the convolutional object encoder takes at most 4 layers")
        d.obj_conv, d.oc_n = 1, len(object_conv_topology)
        for i, layer in enumerate(object_conv_topology):
            d.oc_c[i], d.oc_k[i], d.oc_s[i] = _topology_conv_args(layer)
    return d


def dims_width(d):
    """(image width, grid width) of SpairDims d: its Iw / Gw, or I / G where those are 0 (a square image)."""
    return (d.Iw or d.I), (d.Gw or d.G)


def step_scalars(global_step, batch, world_size=1, train=True):
    """Host evaluation of the two schedules (models.py:59,186-188) in fp32."""
    st = SpairStep()
    st.wheel = exponential_decay(global_step, None, **cfg.LATENT_VAR_TRAINING_WHEEL_PARAM)
    lo = torch.tensor(exponential_decay(global_step, None, **cfg.OBJ_PRES_COUNT_LOG_PRIOR), dtype=torch.float32)
    st.count_prior_prob = float(1 / ((-lo).exp() + 1))
    st.kl_scale = 1.0 / (batch * world_size)
    st.train = int(train)
    st.flags = int(STEP_FLAGS)
    return st


def parse_boxes(z_where, image_h, image_w, align_corners=False):
    """Pixel boxes of the cells of ``z_where`` [B,4,G,Gw] = (xt, yt, xs, ys): [B, G*Gw, 4] = (x0, y0, x1, y1), cell order k = h * Gw + w.
    The box is the footprint of the sprite's P x P texel square as the renderer places it (centre convention: a pixel centre is at
    index + 0.5): x0 = (xt - xs/2) * Iw, x1 = (xt + xs/2) * Iw, y likewise with yt, ys and I.  With ``align_corners`` the same normalised
    extent g through (g + 1) / 2 * (n - 1) + 0.5.  (``metric.py`` keeps the reference's top-left reading of z_where; this does not.)"""
    B = z_where.shape[0]
    xt, yt, xs, ys = (z_where[:, i].reshape(B, -1) for i in range(4))
    lo_hi = torch.stack((xt - 0.5 * xs, yt - 0.5 * ys, xt + 0.5 * xs, yt + 0.5 * ys), dim=-1)
    if align_corners:
        n = lo_hi.new_tensor([image_w - 1, image_h - 1, image_w - 1, image_h - 1])
        return lo_hi * n + 0.5
    return lo_hi * lo_hi.new_tensor([image_w, image_h, image_w, image_h])


class ParseResult:
    """What ``SPAIR.parse`` returns: the scene as objects and as a per-pixel owner map (device tensors; cell order k = h * Gw + w).

    ``loss_terms`` [9], ``recon`` [B,C,I,Iw], ``z_where`` [B,4,G,Gw], ``z_pres`` / ``z_depth`` [B,1,G,Gw], ``z_what`` [B,A,G,Gw];
    ``boxes`` [B,G*Gw,4] (x0, y0, x1, y1) in pixels (``parse_boxes``);
    ``owner`` int32 [B,I,Iw]: the cell whose weight in the renderer's composite is largest at the pixel (lowest k on a tie), -1 where that
    weight is 0 or below the threshold; ``owner_weight`` [B,I,Iw]: that largest weight, whatever the threshold; ``coverage`` [B,I,Iw]:
    the sum of all cells' weights (in [0, 1]); ``area`` int32 [B,G*Gw]: pixels owned per cell."""
    __slots__ = ("loss_terms", "recon", "z_where", "z_pres", "z_depth", "z_what", "boxes", "owner", "owner_weight", "coverage", "area")

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields[k])

    def __repr__(self):
        return "ParseResult(%s)" % ", ".join("%s=%s" % (k, tuple(getattr(self, k).shape)) for k in self.__slots__)


class ComposeResult:
    """What ``SPAIR.compose`` returns (device tensors): ``recon`` [B,C,I,Iw], ``boxes`` [B,G*Gw,4] (``parse_boxes`` of the given z_where)
    and, when ``layers`` was given, ``layers`` [B,K,C,I,Iw] and ``layer_weight`` [B,K,I,Iw] (else None): per requested cell k its
    coefficient in the composite, ``a_k (m_k + 1e-9) / D``, and that coefficient times its warped colour.  The layers of all cells sum
    to ``recon`` (before its clamp to [0, 1], which never acts)."""
    __slots__ = ("recon", "boxes", "layers", "layer_weight")

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields[k])

    def __repr__(self):
        return "ComposeResult(%s)" % ", ".join("%s=%s" % (k, None if getattr(self, k) is None else tuple(getattr(self, k).shape))
                                               for k in self.__slots__)


class GenerateResult:
    """What ``SPAIR.generate`` returns (device tensors; cell order k = h * Gw + w): the drawn latents ``z_where`` [B,4,G,Gw] = (xt, yt,
    xs, ys), ``z_what`` [B,A,G,Gw], ``z_depth`` and ``z_pres`` [B,1,G,Gw] (``z_pres`` hard: 0.0 or 1.0), ``p_z`` [B,1,G,Gw]: the count
    prior's probability of each cell given the cells before it; ``count`` int32 [B]: the number of present cells; and what ``compose``
    returns on those latents: ``recon`` [B,C,I,Iw], ``boxes`` [B,G*Gw,4], ``layers`` / ``layer_weight`` (None without ``layers=``).
    It qualifies as a ``scene`` of ``SPAIR.compose``."""
    __slots__ = ("z_where", "z_what", "z_depth", "z_pres", "p_z", "count", "recon", "boxes", "layers", "layer_weight")

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields[k])

    def __repr__(self):
        return "GenerateResult(%s)" % ", ".join("%s=%s" % (k, None if getattr(self, k) is None else tuple(getattr(self, k).shape))
                                                for k in self.__slots__)


class EvalResult:
    """What ``SPAIR.evaluate`` returns (device tensors; cell order k = h * Gw + w; nats per image, unscaled).

    ``loss`` [B] = ``terms[:, 0]``: the negative single-sample ELBO of each image, BCE + VAE_BETA * (the seven KLs);
    ``terms`` [B,9]: total, reconstruction BCE, KL cy, cx, height, width, attr, depth, presence -- the mean over the draws;
    ``terms_draws`` [K,B,9]: the same per draw;
    ``kl_map`` [B,7,G,Gw]: the seven KLs per cell, ``bce_map`` [B,I,Iw]: the BCE per pixel summed over the channels -- means over the
    draws, None with ``maps=False``;
    ``recon`` [B,C,I,Iw], ``z_where`` [B,4,G,Gw], ``z_pres`` [B,1,G,Gw] and ``loss_terms`` [9] (the batch scalars ``forward`` reports):
    those of the LAST draw.  ``loss_terms[1] = terms[:, 1].sum()`` and ``loss_terms[2 + j] = terms[:, 2 + j].sum() / (B * world_size)``
    for a single draw."""
    __slots__ = ("loss", "terms", "terms_draws", "kl_map", "bce_map", "recon", "z_where", "z_pres", "loss_terms")

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields[k])

    def __repr__(self):
        return "EvalResult(%s)" % ", ".join("%s=%s" % (k, None if getattr(self, k) is None else tuple(getattr(self, k).shape))
                                            for k in self.__slots__)


class _NullWriter:
    def __getattr__(self, name):
        if name.startswith("__"):         # copy / pickle probe for __deepcopy__, __getstate__, ...: a writer has none of them
            raise AttributeError(name)
        return lambda *a, **k: None


class _Engine(dict):
    """One batch size's workspace + noise maps + dims (a dict that can be weakly referenced)."""
    __slots__ = ("__weakref__",)


class _StepFn(torch.autograd.Function):
    """Ties the hand-written backward into autograd.  ``anchor`` is a dummy differentiable leaf:
    the parameter gradients are accumulated straight into the flat gradient buffer (the views
    behind every ``p.grad``) by ``spair_backward`` instead of being returned one tensor at a time.
    recon / z_where / z_pres are differentiable only with ``model.differentiable_outputs``; their
    adjoints then enter the same reverse pass (``SpairStepIO.grad_recon`` / ``grad_z_where`` /
    ``grad_z_pres``).  When ``x`` requires grad the same pass also returns its gradient
    (``SpairStepIO.grad_x``)."""

    @staticmethod
    def forward(ctx, anchor, model, x, step, noise):
        loss_terms, recon, z_where, z_pres = model._run_forward(x, step, noise, train=True)
        ctx.model, ctx.x, ctx.step, ctx.noise = model, x, step, noise
        # the saved activations live in the engine's workspace, not in autograd: remember WHICH forward filled it, so a backward through
        # a workspace that a later forward has overwritten (or that the engine cache has dropped) raises instead of being silently wrong.
        # A weak reference: the graph must not keep a multi-GB workspace alive after the cache evicted it.
        ctx.engine_ref = weakref.ref(model._last["engine"])
        ctx.generation = model._last["engine"]["generation"]
        if not model.differentiable_outputs:
            ctx.mark_non_differentiable(recon, z_where, z_pres)
        # otherwise autograd zero-fills a gradient for each output nothing reached (17 MB per step): an absent adjoint stays None and
        # launches nothing
        ctx.set_materialize_grads(False)
        model._loss_terms = loss_terms
        # a view, not a copy: `loss_terms` is a fresh buffer of this forward (a device copy here is 6 us + a launch gap between the loss
        # kernel and the backward's first kernel).  Slot 9 is the kernel's SECOND copy of the total: an in-place op on the returned loss
        # (`loss /= accum_steps`) does not change what loss_terms() and the logging helpers report (slots 0..8)
        return loss_terms[9], recon, z_where, z_pres

    @staticmethod
    def backward(ctx, g_loss, g_recon, g_zw, g_zp):
        if g_loss is None and g_recon is None and g_zw is None and g_zp is None:
            return None, None, None, None, None
        engine = ctx.engine_ref()
        if engine is None or engine["generation"] != ctx.generation:
            raise L.SpairHipError(
                "backward() of a SPAIR forward whose saved activations were overwritten by a later forward of the same batch size, or "
                "whose workspace the engine cache has dropped (the engine keeps ONE set of activations per batch size and "
                "`max_engines` batch sizes; call backward before the next forward of that size)")
        # a backward through the outputs alone: the loss terms (KL scale included) get a zero adjoint, and the loss's BCE-target term
        # is left out of x's gradient (as in torch, where the loss is then not part of the graph: no 0 * inf)
        bce_target = g_loss is not None
        if g_loss is None:
            g_loss = torch.zeros((), device=ctx.x.device, dtype=torch.float32)
        outs = [None if g is None else g.contiguous().float() for g in (g_recon, g_zw, g_zp)]
        grad_x = torch.empty_like(ctx.x) if ctx.needs_input_grad[2] else None
        ctx.model._run_backward(ctx.x, ctx.step, ctx.noise, g_loss.contiguous().float(), engine, *outs, grad_x=grad_x, bce_target=bce_target)
        return None, None, grad_x, None, None      # the parameter gradients went straight into the flat buffer


class SPAIR(nn.Module):
    def __init__(self, image_shape, writer=None, device=None, compute_dtype=None, object_encoder=None, differentiable_outputs=False):
        """``object_encoder``: 'mlp' (the reference's live configuration, models.py:152,165) or 'conv' -- the convolutional encoder /
        decoder pair of ``cfg.CONV_OBJECT_ENCODER_TOPOLOGY`` (config.py:15-20) that models.py:606-665 sketches but cannot run
        (parity unpinned); default ``cfg.OBJECT_ENCODER``.  The conv pair runs on the per-wavefront launches in either compute dtype (its
        own convolutions in fp32; the fused bf16 per-cell kernels are built for the MLP pair).

        ``differentiable_outputs``: with grad enabled, ``recon``, ``z_where`` and ``z_pres`` require grad as in the reference
        (models.py:35-131) and a user term on them trains through the model (box supervision, a count loss, a masked recon loss).
        Off by default: the outputs are then plain tensors (``.numpy()`` works on them directly) and the step is unchanged.  On, it
        costs one [B,I,I] store in the renderer forward, plus two elementwise kernels in a backward that receives such an adjoint."""
        super().__init__()
        self.differentiable_outputs = bool(differentiable_outputs)
        self.object_encoder_kind = (object_encoder or cfg.OBJECT_ENCODER).lower()
        if self.object_encoder_kind not in ('mlp', 'conv'):
            raise ValueError("object_encoder must be 'mlp' or 'conv'")
        self.image_shape = list(image_shape)
        self.writer = writer if writer is not None else _NullWriter()
        self.B = 1
        self.device = torch.device(device) if device is not None else torch.device('cuda')
        self.compute_dtype = (compute_dtype or cfg.COMPUTE_DTYPE).lower()
        self.world_size = 1          # set by spair_pytorch_amd.ddp for the sharded loss
        self.context_dim = (cfg.N_LOOKBACK * 2 + 1) ** 2 // 2 * (4 + cfg.N_ATTRIBUTES + 1 + 1)
        self.lookback = int(cfg.N_LOOKBACK)
        if not 1 <= self.lookback <= 3:
            raise L.SpairHipError("N_LOOKBACK must be 1, 2 or 3 (4, 12 or 24 context neighbours)")
        self._build_networks()
        self._build_edge_element()
        self._build_indep_prior()
        self.pixels_per_cell = tuple(int(i) for i in self.backbone.grid_cell_size)
        self._flat = None
        self._flat_grad = None
        self._engines = {}
        # workspaces kept alive (one per batch size, least recently used dropped).  None = automatic: a second one (eval batch / last
        # partial batch beside the training batch) only while all live workspaces together stay under a quarter of the device's
        # memory, otherwise exactly one (they are ~5 GB each at B=256 / 128x128)
        self.max_engines = None
        self._grad_buckets = None    # set by spair_pytorch_amd.ddp.attach: readiness events for the overlapped all-reduce
        self._anchor = None
        self._loss_terms = None
        # failed / non-finite steps (SpairStep.status, status_host): two device ints [sticky bits, this step's bits] and one host word the
        # loss kernel stores to when a step fails -- owned by the model, so they outlive a workspace that is evicted or re-zeroed
        self._status_dev = None
        self._status_host = None
        self.raise_on_nonfinite = True     # forward() raises if an EARLIER step's loss was non-finite (no synchronisation: a host load)
        self.dist_param, self.dist = {}, {}
        self.training_wheel = None
        self.global_step = 0

    # ---- construction: same order of RNG consumption as models.py:133-167,273-290 -------------
    def _build_networks(self):
        self.backbone = Backbone(self.image_shape, cfg.N_BACKBONE_FEATURES)
        self.feature_space_dim = self.backbone.compute_output_shape()
        n_pass = cfg.N_PASSTHROUGH_FEATURES
        n_feat = self.feature_space_dim[0]
        self.box_network = build_MLP(n_feat + self.context_dim, multiple_output=(8, n_pass))
        obj_dim, chan = cfg.OBJECT_SHAPE[0], cfg.INPUT_IMAGE_SHAPE[0]
        if self.object_encoder_kind == 'conv':
            self.object_conv_topology = [dict(t) for t in cfg.CONV_OBJECT_ENCODER_TOPOLOGY]
            self.object_encoder = ObjectConvEncoder([chan, obj_dim, obj_dim], 2 * cfg.N_ATTRIBUTES, self.object_conv_topology)
        else:
            self.object_conv_topology = None
            self.object_encoder = build_MLP(obj_dim * obj_dim * chan, 2 * cfg.N_ATTRIBUTES, hidden_layers=[256, 128])
        z_in = 4 + cfg.N_ATTRIBUTES + n_pass + self.context_dim + cfg.N_BACKBONE_FEATURES
        self.z_network = build_MLP(z_in, multiple_output=(2, n_pass))
        self.obj_network = build_MLP(z_in + 1, 1)
        if self.object_encoder_kind == 'conv':
            self.object_decoder = ObjectConvDecoder(cfg.N_ATTRIBUTES, chan + 1, self.object_encoder.shapes, self.object_conv_topology)
        else:
            self.object_decoder = build_MLP(cfg.N_ATTRIBUTES, obj_dim * obj_dim * (chan + 1), hidden_layers=[128, 256])
        # dead in the reference (models.py:120,167); kept for state_dict parity.  One context record without its presence: the 55 channels
        # the reference writes out for N_ATTRIBUTES = 50, as the library's parameter layout sizes it for any N_ATTRIBUTES
        self.attn = _SelfAttnParams(4 + cfg.N_ATTRIBUTES + 1)

    def _build_edge_element(self):
        sizes = [4, cfg.N_ATTRIBUTES, 1, 1]
        t = torch.randn(sum(sizes))
        loc, attr, depth, pres = torch.split(t, sizes)
        elem = torch.cat((torch.sigmoid(loc), attr, torch.sigmoid(depth), torch.sigmoid(pres)))
        self.register_parameter('virtual_edge_element', nn.Parameter(elem))

    def _build_indep_prior(self):
        from torch.distributions import Normal
        self.kl_priors = {n: Normal(m, s) for n, (m, s) in cfg.PRIORS.items()}

    # ---- flat parameter / gradient buffers ---------------------------------------------------------
    def _dims(self, batch):
        return make_dims(batch, self.image_shape, self.backbone.topology, self.compute_dtype, self.object_conv_topology, self.lookback)

    def _flatten(self):
        """(Re)build the flat buffers on ``self.device`` and re-point every Parameter into them."""
        lib = L.lib()
        d = self._dims(1)
        lib.spair_param_total.restype = ctypes.c_int64
        total = lib.spair_param_total(ctypes.byref(d))
        n = lib.spair_param_count(ctypes.byref(d))
        if total <= 0 or n <= 0:
            raise L.SpairHipError("unsupported configuration for the HIP engine (image=%s, topology=%s)" % (self.image_shape, self.backbone.topology))
        named = dict(self.named_parameters())
        dev = self.device
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self._slices = {}
        name = ctypes.create_string_buffer(128)
        off, ndim = ctypes.c_int64(), ctypes.c_int()
        shape = (ctypes.c_int64 * 4)()
        seen = set()
        for i in range(n):
            L.check(lib.spair_param_info(ctypes.byref(d), i, name, 128, ctypes.byref(off), shape, ctypes.byref(ndim)), "spair_param_info")
            key = name.value.decode()
            shp = tuple(int(shape[k]) for k in range(ndim.value))
            p = named[key]
            if tuple(p.shape) != shp:
                raise L.SpairHipError("parameter %s: module shape %s != library layout %s" % (key, tuple(p.shape), shp))
            cnt = int(np.prod(shp))
            view = flat[off.value:off.value + cnt].view(shp)
            view.copy_(p.data.to(dev))
            p.data = view
            p.grad = None
            self._slices[key] = (off.value, cnt, shp)
            seen.add(key)
        missing = set(named) - seen
        if missing:
            raise L.SpairHipError("parameters without a slot in the flat layout: %s" % sorted(missing))
        self._flat, self._flat_grad = flat, flat_grad
        self._params_by_key = named
        self._anchor = torch.zeros((), device=dev, requires_grad=True)
        self._engines = {}
        self._status_dev = torch.zeros(2, dtype=torch.int32, device=dev)
        if self._status_host is None:
            word = ctypes.POINTER(ctypes.c_int)()
            L.check(lib.spair_host_word_alloc(ctypes.byref(word)), "spair_host_word_alloc")
            self._status_host = word
            weakref.finalize(self, lib.spair_host_word_free, word)

    # ---- copies: copy.deepcopy(model), pickle, torch.save(model) -------------------------------------------
    # what belongs to THIS object's device state and holds raw pointers, events or a multi-GB workspace
    _PER_INSTANCE = ("_flat", "_flat_grad", "_slices", "_params_by_key", "_anchor", "_engines", "_last", "_loss_terms", "_status_dev",
                     "_status_host", "_status_xchg", "_grad_buckets", "_grad_norm_tables", "dist_param", "dist")

    def __getstate__(self):
        """A copy (an EMA or evaluation model, a pickled checkpoint) takes the parameters, buffers and settings; it gets its OWN flat
        buffers, gradient buffer, engines and status words, built on first use as for a new model -- a failed step on one of the two
        never makes the other raise.  ``ddp.attach`` is per object: attach the copy if it is to train."""
        state = dict(self.__dict__)
        for k in self._PER_INSTANCE:
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._flat = self._flat_grad = self._anchor = self._loss_terms = self._last = None
        self._status_dev = self._status_host = self._grad_buckets = None
        self._engines, self.dist_param, self.dist = {}, {}, {}

    def _apply(self, fn, recurse=True):
        # .to(device)/.cuda()/.float(): let nn.Module move the tensors, then re-flatten on the new device
        out = super()._apply(fn, recurse)
        p0 = next(self.parameters())
        if p0.is_cuda:
            self.device = p0.device
            self._flatten()
        else:
            self._flat = None
        return out

    def flat_parameters(self):
        self._ensure_ready()
        return self._flat

    def flat_gradients(self):
        self._ensure_ready()
        return self._flat_grad

    def _ensure_ready(self):
        if self._flat is None:
            if self.device.type != 'cuda':
                raise L.SpairHipError("SPAIR runs on an MI355X only: move the model with .to('cuda') (there is no CPU path)")
            self._flatten()
        # a load_state_dict / optimizer may have swapped .data: detect and re-point (cheap pointer check)
        p = self._params_by_key['virtual_edge_element']
        if p.data_ptr() != self._flat.data_ptr() + 4 * self._slices['virtual_edge_element'][0]:
            self._flatten()

    def _bind_grads(self):
        """Make every p.grad a view of the flat gradient buffer (zeroing slots that were None)."""
        all_none = True
        for key, p in self._params_by_key.items():
            if p.grad is not None:
                all_none = False
                break
        if all_none:
            self._flat_grad.zero_()
        base = self._flat_grad.data_ptr()
        for key, p in self._params_by_key.items():
            off, cnt, shp = self._slices[key]
            if key.startswith('attn.'):
                continue   # never receives a gradient in the reference (grad stays None)
            if p.grad is None:
                if not all_none:
                    self._flat_grad[off:off + cnt].zero_()
                p.grad = self._flat_grad[off:off + cnt].view(shp)
            elif p.grad.data_ptr() != base + 4 * off:
                v = self._flat_grad[off:off + cnt].view(shp)
                v.copy_(p.grad)
                p.grad = v

    # ---- engine ----------------------------------------------------------------------------------------
    def _engine(self, batch):
        e = self._engines.get(batch)
        if e is None:
            lib = L.lib()
            d = self._dims(batch)
            lib.spair_workspace_bytes.restype = ctypes.c_int64
            nbytes = lib.spair_workspace_bytes(ctypes.byref(d))
            if nbytes <= 0:
                raise L.SpairHipError("unsupported configuration for the HIP engine (B=%d, image=%s, topology=%s)" %
                                      (batch, self.image_shape, self.backbone.topology))
            (G, A), Gw = (d.G, d.A), dims_width(d)[1]
            dev = self.device
            limit = self.max_engines
            if limit is None:
                live = sum(int(v["workspace"].numel()) for v in self._engines.values())
                limit = 2 if (live + nbytes) <= torch.cuda.get_device_properties(dev).total_memory // 4 else 1
            block = None
            while len(self._engines) >= max(1, limit):      # evict BEFORE allocating: two multi-GB workspaces never coexist needlessly
                old = self._engines.pop(next(iter(self._engines)))
                # `_last` holds a strong reference to the engine of the latest forward: drop it too, or the evicted workspace stays alive
                # until `_run_forward` reassigns `_last` -- i.e. across the allocation below (a pending backward through it raises, as for
                # any evicted engine: the step function only holds a weak reference; export_map and the logging helpers say so too)
                if getattr(self, "_last", None) is not None and self._last.get("engine") is old:
                    self._last = None
                # alternating batch sizes under limit 1 (the partial last batch of every epoch): the evicted block is re-used when the new
                # workspace fits in it -- re-zeroed, no hipFree / hipMalloc / device synchronisation per alternation
                if block is None and int(old["workspace"].numel()) >= nbytes:
                    block = old["workspace"]
                del old
            if block is None and max(1, limit) == 1:
                torch.cuda.empty_cache()                  # the limit-1 case exists because two workspaces do not fit comfortably: return the block
            ws = block.zero_() if block is not None else torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            e = _Engine(dims=d, generation=0,
                     workspace=ws,                                                   # zero-initialised ONCE per engine
                     noise=dict(eps_box=torch.empty(batch, 4, G, Gw, device=dev), eps_attr=torch.empty(batch, A, G, Gw, device=dev),
                                eps_depth=torch.empty(batch, 1, G, Gw, device=dev), u_pres=torch.empty(batch, 1, G, Gw, device=dev)))
            if self.differentiable_outputs:
                self._outgrad_buffers(e)
        else:
            self._engines.pop(batch)
        self._engines[batch] = e         # most recently used last
        return e

    def _outgrad_buffers(self, e):
        """The differentiable outputs' two buffers of engine ``e`` (allocated on first use): the renderer's 1/D per pixel, kept by the
        forward, and the backward's folded copy of the renderer's per-pixel adjoints (+ one float for its unit loss gradient)."""
        if e.get("inv_den") is None:
            d = e['dims']
            Iw = dims_width(d)[0]
            e["inv_den"] = torch.empty(d.B, d.I, Iw, device=self.device, dtype=torch.float32)
            e["aux_scratch"] = torch.empty(2 * d.B * d.C * d.I * Iw + 1, device=self.device, dtype=torch.float32)
        return e["inv_den"], e["aux_scratch"]

    def _input_grad_scratch(self, e):
        """Scratch of the image gradient of engine ``e`` (the glimpse term, [B,C,H,W] fp32), allocated on first use; never part of the
        workspace."""
        if e.get("x_scratch") is None:
            lib = L.lib()
            lib.spair_input_grad_scratch_bytes.restype = ctypes.c_int64
            nbytes = lib.spair_input_grad_scratch_bytes(ctypes.byref(e['dims']))
            if nbytes <= 0:
                raise L.SpairHipError("spair_input_grad_scratch_bytes refused these dims")
            e["x_scratch"] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return e["x_scratch"]

    def _draw_noise(self, e):
        """The 7 per-cell draws (models.py:333-336,84,95,402-403) as whole maps, one launch; the seed
        comes from torch's CPU generator so torch.manual_seed controls it."""
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        # the maps are filled by spair_forward itself (SpairStep.draw_noise), on its helper stream beside the backbone
        return dict(e['noise'], _seed=seed)

    def _run_forward(self, x, step, noise, train):
        e = self._engine(x.shape[0])
        d = e['dims']
        dev = x.device
        (B, G), (Iw, Gw) = (x.shape[0], d.G), dims_width(d)
        loss_terms = torch.empty(16, device=dev, dtype=torch.float32)
        recon = torch.empty(B, d.C, d.I, Iw, device=dev, dtype=torch.float32)
        z_where = torch.empty(B, 4, G, Gw, device=dev, dtype=torch.float32)
        z_pres = torch.empty(B, 1, G, Gw, device=dev, dtype=torch.float32)
        st = step_scalars(step, B, self.world_size, train)
        if noise.get('_seed') is not None:
            st.draw_noise, st.noise_seed = 1, int(noise['_seed'])
        st.status = self._status_dev.data_ptr()
        st.status_host = ctypes.cast(self._status_host, ctypes.c_void_p).value
        e["generation"] += 1              # whatever this workspace held for an earlier forward is gone now
        self._last = dict(engine=e, st=st)
        inv_den = self._outgrad_buffers(e)[0] if train and self.differentiable_outputs else None
        io = self._step_io(e, x, noise, loss_out=loss_terms, recon=recon, z_where=z_where, z_pres=z_pres, inv_den=inv_den)
        L.check(L.lib().spair_forward(ctypes.byref(d), ctypes.byref(st), ctypes.byref(io), L.stream()), "spair_forward")
        return loss_terms, recon, z_where, z_pres

    def _step_io(self, e, x, noise, **buffers):
        """The SpairStepIO of a step on engine ``e``: the buffers both directions read, then ``buffers`` (field name -> tensor or None)."""
        io = L.SpairStepIO(params=self._flat.data_ptr(), x=x.data_ptr(), workspace=e['workspace'].data_ptr())
        for k in NOISE_MAPS:
            setattr(io, k, noise[k].data_ptr())
        for k, t in buffers.items():
            if t is not None:             # (a field left alone is NULL)
                setattr(io, k, t.data_ptr())
        return io

    def _run_backward(self, x, step, noise, g_loss, e=None, g_recon=None, g_z_where=None, g_z_pres=None, grad_x=None, bce_target=True):
        """``g_recon`` / ``g_z_where`` / ``g_z_pres``: contiguous fp32 adjoints of the forward's outputs, or None (nothing launched for them).
        ``grad_x``: a contiguous fp32 tensor shaped like ``x`` that receives the image gradient (overwritten), or None (no image gradient);
        ``bce_target``: include the loss's BCE-target term in it."""
        e = e if e is not None else self._engine(x.shape[0])
        st = step_scalars(step, x.shape[0], self.world_size, True)
        self._bind_grads()
        io = self._step_io(e, x, noise, grad_loss=g_loss, grads=self._flat_grad, inv_den=e.get('inv_den'), grad_recon=g_recon,
                           grad_z_where=g_z_where, grad_z_pres=g_z_pres, aux_scratch=e.get('aux_scratch'), grad_x=grad_x,
                           x_scratch=None if grad_x is None else self._input_grad_scratch(e))
        io.bce_target = int(bool(bce_target))
        gb = self._grad_buckets
        if gb is not None:
            io.ev_decoder, io.ev_cells, io.ev_backbone = gb.handles()
        L.check(L.lib().spair_backward(ctypes.byref(e['dims']), ctypes.byref(st), ctypes.byref(io), L.stream()), "spair_backward")
        if gb is not None:
            gb.pending = True             # ddp.allreduce_gradients(model) consumes the three events

    # ---- public API ------------------------------------------------------------------------------------
    def forward(self, x, global_step=0, noise=None):
        """models.py:35-131.  ``noise`` (optional dict eps_box/eps_attr/eps_depth/u_pres, NCHW maps)
        replaces the internal draws -- used by the parity tests.  An ``x`` that requires grad gets the reference's gradient on backward;
        it is +inf wherever recon is exactly 0 (-inf where exactly 1): torch's BCE gradient with respect to its target is -logit(recon),
        unclamped, and this keeps it."""
        self._ensure_ready()
        if not x.is_cuda:
            raise L.SpairHipError("input must be on the MI355X (got %s); there is no CPU path" % x.device)
        x = x.contiguous().float()
        if list(x.shape[1:]) != list(self.image_shape):
            raise AssertionError("expected input [B,%s], got %s" % (self.image_shape, tuple(x.shape)))
        if self.raise_on_nonfinite and self._status_host[0] != 0:
            raise L.SpairHipError(self._status_text(self._status_host[0]) + " -- seen by a later forward(); clear_step_status() to go on")
        self.global_step = global_step
        self.batch_size = x.shape[0]
        e = self._engine(x.shape[0])
        if noise is None:
            noise = self._draw_noise(e)
        else:
            noise = {k: noise[k].to(x.device).contiguous().float() for k in NOISE_MAPS}
            want = {k: tuple(v.shape) for k, v in e['noise'].items()}      # [B,{4,A,1,1},Gh,Gw]
            for k, v in noise.items():
                if tuple(v.shape) != want[k]:
                    raise AssertionError("noise[%r]: expected %s, got %s" % (k, want[k], tuple(v.shape)))
        self.training_wheel = exponential_decay(global_step, None, **cfg.LATENT_VAR_TRAINING_WHEEL_PARAM)
        if torch.is_grad_enabled():
            loss, recon, z_where, z_pres = _StepFn.apply(self._anchor, self, x, int(global_step), noise)
        else:
            terms, recon, z_where, z_pres = self._run_forward(x, int(global_step), noise, train=False)
            self._loss_terms = terms
            loss = terms[0].clone()
        self._log_scalars()
        self.dist_param, self.dist = _LazyDist(self), _LazyDist(self, as_normal=True)
        return loss, recon, z_where, z_pres

    def _mean_noise(self, e):
        """The posterior mean as noise maps of engine ``e`` (constant, allocated on first use): zero eps_*, u_pres = 0.5, whose logistic
        noise log(u + eps) - log(1 - u + eps) is exactly 0.  Nothing is drawn."""
        if e.get("mean_noise") is None:
            e["mean_noise"] = {k: torch.full_like(v, 0.5 if k == "u_pres" else 0.0) for k, v in e["noise"].items()}
        return e["mean_noise"]

    def parse(self, x, global_step=0, sample=False, threshold=0.5, noise=None):
        """Read the scene out of the model: one ``no_grad`` forward and the renderer's per-pixel assignment, as a ``ParseResult``.

        ``sample=False`` (default) takes the posterior mean (zero eps_*, u_pres = 0.5) from constant maps: the answer is repeatable and
        NOTHING is drawn from torch's generators, so parse calls between training steps leave the training run's noise sequence alone.
        ``sample=True`` draws as ``forward`` does; ``noise`` is the dict ``forward`` takes and wins over both.  ``global_step`` only moves
        the count-prior term of ``loss_terms``.  ``threshold``: a pixel whose largest composite weight is below it (or 0) gets owner -1;
        ``owner_weight`` is the raw maximum either way.

        Like any forward it overwrites the workspace of that batch size: ``backward()`` of an earlier forward of the same batch size
        raises afterwards (the generation check).  As any ``no_grad`` forward it leaves the word ``FusedAdam.step()`` reads as its skip
        flag alone: it may be called anywhere, between ``backward()`` and ``step()`` too (a non-finite loss of its own still sets the
        sticky word and the host word, as ``forward`` does)."""
        self._ensure_ready()
        if not x.is_cuda:
            raise L.SpairHipError("input must be on the MI355X (got %s); there is no CPU path" % x.device)
        x = x.contiguous().float()
        if list(x.shape[1:]) != list(self.image_shape):
            raise AssertionError("expected input [B,%s], got %s" % (self.image_shape, tuple(x.shape)))
        if self.raise_on_nonfinite and self._status_host[0] != 0:
            raise L.SpairHipError(self._status_text(self._status_host[0]) + " -- seen by a later parse(); clear_step_status() to go on")
        e = self._engine(x.shape[0])
        if noise is not None:
            noise = {k: noise[k].to(x.device).contiguous().float() for k in NOISE_MAPS}
            for k, v in noise.items():
                if tuple(v.shape) != tuple(e['noise'][k].shape):
                    raise AssertionError("noise[%r]: expected %s, got %s" % (k, tuple(e['noise'][k].shape), tuple(v.shape)))
        else:
            noise = self._draw_noise(e) if sample else self._mean_noise(e)
        with torch.no_grad():
            terms, recon, z_where, z_pres = self._run_forward(x, int(global_step), noise, train=False)
            self._loss_terms = terms
            d = e['dims']
            (B, I), (Iw, Gw) = (d.B, d.I), dims_width(d)
            owner = torch.empty(B, I, Iw, device=x.device, dtype=torch.int32)
            weight, coverage = (torch.empty(B, I, Iw, device=x.device, dtype=torch.float32) for _ in range(2))
            area = torch.empty(B, d.G * Gw, device=x.device, dtype=torch.int32)
            L.check(L.lib().spair_parse_owner(ctypes.byref(d), L.ptr(e['workspace']), int(STEP_FLAGS), float(threshold), L.ptr(owner),
                                              L.ptr(weight), L.ptr(coverage), L.ptr(area), L.stream()), "spair_parse_owner")
            return ParseResult(loss_terms=terms[:9], recon=recon, z_where=z_where, z_pres=z_pres, z_depth=self.export_map(1),
                               z_what=self.export_map(0), boxes=parse_boxes(z_where, I, Iw, bool(d.align_corners)), owner=owner,
                               owner_weight=weight, coverage=coverage, area=area)

    def compose(self, scene=None, *, z_where=None, z_what=None, z_depth=None, z_pres=None, layers=None):
        """Render a scene from GIVEN latents: the decoder and the renderer of the step, nothing inferred (the reference's ``_render``,
        models.py:452-542, a pure function of the four latents).  Returns a ``ComposeResult``.

        ``scene``: any object with ``z_where`` [B,4,G,Gw] = (xt, yt, xs, ys), ``z_what`` [B,A,G,Gw], ``z_depth`` and ``z_pres``
        [B,1,G,Gw] -- a ``ParseResult`` qualifies; a keyword tensor replaces that field.  Device tensors (converted with
        ``.float().contiguous()``).  The values are taken AS GIVEN: ``z_pres`` and ``z_depth`` are not clamped to [0, 1], box sizes are not
        checked (a zero or negative size gives an empty object).

        ``layers``: optional int tensor [B,K] of cell indices k = h * Gw + w.  The result then also holds, per requested cell,
        ``layer_weight`` = a_k (m_k + 1e-9) / D and ``layers`` = layer_weight * warp(colour_k), with a_k = warp(alpha_k pres_k),
        m_k = warp(max(alpha_k pres_k depth_k, 0.01)) and D the sum of m over ALL cells (+ G Gw 1e-9).  Any value outside [0, G*Gw) means
        "skip" and gives an all-zero layer (nothing is validated on the host: no synchronisation); duplicates are allowed.

        Removing an object means ``z_pres = 0`` for its cell.  That is not the same as dropping the object from the sum: its importance
        floor 0.01 stays in D inside its footprint, exactly as in the reference, so the objects it overlapped stay slightly dimmed there.

        ``no_grad`` and deterministic: nothing is drawn (no torch generator is touched), no loss is computed, and the step-status word
        ``FusedAdam`` reads is NOT written, so -- unlike ``parse`` -- it is safe between ``backward()`` and ``FusedAdam.step()``.  Like any
        forward it overwrites the workspace of that batch size: ``backward()`` of an earlier forward of the same batch size raises
        afterwards (the generation check), and ``export_map`` / ``workspace_view`` then show the composed scene."""
        self._ensure_ready()
        given = dict(z_where=z_where, z_what=z_what, z_depth=z_depth, z_pres=z_pres)
        lat = {}
        for k, v in given.items():
            if v is None:
                v = getattr(scene, k, None)
            if v is None:
                raise AssertionError("compose: no %s (neither in `scene` nor as a keyword)" % k)
            if not torch.is_tensor(v) or not v.is_cuda:
                raise L.SpairHipError("compose: %s must be a tensor on the MI355X; there is no CPU path" % k)
            lat[k] = v.detach().float().contiguous()
        B = int(lat["z_where"].shape[0]) if lat["z_where"].dim() == 4 else 0
        if B < 1:
            raise AssertionError("compose: z_where must be [B,4,G,Gw], got %s" % (tuple(lat["z_where"].shape),))
        e = self._engine(B)
        d = e['dims']
        (I, G), (Iw, Gw) = (d.I, d.G), dims_width(d)
        for k, ch in (("z_where", 4), ("z_what", d.A), ("z_depth", 1), ("z_pres", 1)):
            if tuple(lat[k].shape) != (B, ch, G, Gw):
                raise AssertionError("compose: %s: expected %s, got %s" % (k, (B, ch, G, Gw), tuple(lat[k].shape)))
        cells = None
        if layers is not None:
            if not torch.is_tensor(layers) or not layers.is_cuda:
                raise L.SpairHipError("compose: layers must be an int tensor on the MI355X")
            if layers.dim() != 2 or layers.shape[0] != B or layers.shape[1] < 1 or layers.is_floating_point():
                raise AssertionError("compose: layers: expected an int tensor [%d,K], got %s %s" % (B, layers.dtype, tuple(layers.shape)))
            # (an index beyond int32 is outside the grid either way: it stays outside)
            cells = layers.clamp(-1, G * Gw).to(torch.int32).contiguous()
        dev = lat["z_where"].device
        with torch.no_grad():
            recon = torch.empty(B, d.C, I, Iw, device=dev, dtype=torch.float32)
            inv_den = torch.empty(B, I, Iw, device=dev, dtype=torch.float32) if cells is not None else None
            e["generation"] += 1              # whatever this workspace held for an earlier forward is gone now
            self._last = dict(engine=e, st=None)
            L.check(L.lib().spair_compose(ctypes.byref(d), L.ptr(self._flat), L.ptr(e['workspace']), int(STEP_FLAGS), L.ptr(lat["z_where"]),
                                          L.ptr(lat["z_what"]), L.ptr(lat["z_depth"]), L.ptr(lat["z_pres"]), L.ptr(recon), L.ptr(inv_den),
                                          L.stream()), "spair_compose")
            out_layers = weight = None
            if cells is not None:
                K = int(cells.shape[1])
                out_layers = torch.empty(B, K, d.C, I, Iw, device=dev, dtype=torch.float32)
                weight = torch.empty(B, K, I, Iw, device=dev, dtype=torch.float32)
                L.check(L.lib().spair_render_layers(ctypes.byref(d), L.ptr(e['workspace']), int(STEP_FLAGS), L.ptr(cells), K, L.ptr(inv_den),
                                                    L.ptr(out_layers), L.ptr(weight), L.stream()), "spair_render_layers")
            return ComposeResult(recon=recon, boxes=parse_boxes(lat["z_where"], I, Iw, bool(d.align_corners)), layers=out_layers,
                                 layer_weight=weight)

    def generate(self, batch, global_step=0, *, count=None, seed=None, noise=None, layers=None):
        """Sample ``batch`` scenes from the model's own prior -- the generative process the loss assumes -- and render them: latents drawn by
        ``spair_prior_sample``, then ``compose``.  Returns a ``GenerateResult``.

        Gaussian latents: raw = m + s * eps with (m, s) of ``cfg.PRIORS`` (cy, cx, height, width, attr, depth), then the forward's own
        transforms: cell_y/x = (MAX_YX - MIN_YX) sigmoid(clamp10(raw)) + MIN_YX, height/width likewise with MIN_HW / MAX_HW,
        z_where = (xt, yt, xs, ys) = (cell_px / Iw (cell_x + w), cell_px / I (cell_y + h), width anchor / Iw, height anchor / I),
        z_what = raw, z_depth = 4 sigmoid(clamp10(raw)).  The training wheel plays no part.

        Presence: the sequential count prior of the KL (reference models.py:184-257), cells in row-major order.  The count distribution
        starts from normalise((1 - p) p^c), c = 0 .. G*Gw, with p the count-prior probability of ``global_step`` (the schedule ``forward``
        uses: almost flat over 0 .. G*Gw at step 0, p ~ 0.012 late); cell i gets p_z(i) = sum_c cd_c clamp(c - seen, 0, rem) / rem with
        rem = G*Gw - i, and z_pres = [u < p_z] is HARD (0.0 or 1.0), which is what the recursion conditions on.

        ``count``: None, an int or an int tensor [B] on the device: exactly that many objects per sample, uniformly placed (the same
        recursion from a one-hot count distribution, p_z = (count - seen) / rem exactly).  A value outside [0, G*Gw] is clamped (in the
        kernel: the host does not synchronise to validate it).

        ``noise``: the dict ``forward`` takes (eps_box / eps_attr / eps_depth / u_pres, NCHW maps of batch size ``batch``; u_pres in
        [0, 1)); it wins over ``seed``.  ``seed=int`` fills fresh maps from that seed and touches NO torch generator, so it is safe inside
        a training run; ``seed=None`` draws the seed from torch's CPU generator as ``forward`` does (``torch.manual_seed`` controls it).
        The maps are tensors of this call, not the engine's.

        Everything after the latents IS ``self.compose(...)`` (``layers`` is passed through): ``no_grad``, no loss, the step-status word
        ``FusedAdam`` reads is NOT written, so it is safe between ``backward()`` and ``FusedAdam.step()``; like ``compose`` it advances the
        engine generation of that batch size (``backward()`` of an earlier forward of the same batch size raises afterwards)."""
        self._ensure_ready()
        B = int(batch)
        if B < 1:
            raise AssertionError("generate: batch must be >= 1, got %r" % (batch,))
        e = self._engine(B)
        d = e['dims']
        (G, A), Gw = (d.G, d.A), dims_width(d)[1]
        dev = self.device
        want = {k: tuple(v.shape) for k, v in e['noise'].items()}      # [B,{4,A,1,1},Gh,Gw]
        lib = L.lib()
        if noise is not None:
            noise = {k: noise[k].to(dev).contiguous().float() for k in NOISE_MAPS}
            for k, v in noise.items():
                if tuple(v.shape) != want[k]:
                    raise AssertionError("noise[%r]: expected %s, got %s" % (k, want[k], tuple(v.shape)))
        else:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            noise = {k: torch.empty(want[k], device=dev, dtype=torch.float32) for k in NOISE_MAPS}
            L.check(lib.spair_noise_fill(ctypes.byref(d), int(seed) & (2 ** 64 - 1), *(L.ptr(noise[k]) for k in NOISE_MAPS), L.stream()),
                    "spair_noise_fill")
        cnt = None
        if count is not None:
            if torch.is_tensor(count):
                if not count.is_cuda:
                    raise L.SpairHipError("generate: count must be an int or an int tensor on the MI355X")
                if tuple(count.shape) != (B,) or count.is_floating_point():
                    raise AssertionError("generate: count: expected an int tensor [%d], got %s %s" % (B, count.dtype, tuple(count.shape)))
                cnt = count.clamp(-1, G * Gw + 1).to(torch.int32).contiguous()
            else:
                cnt = torch.full((B,), max(-1, min(int(count), G * Gw + 1)), device=dev, dtype=torch.int32)
        st = step_scalars(global_step, B, self.world_size, False)
        with torch.no_grad():
            z_where = torch.empty(B, 4, G, Gw, device=dev, dtype=torch.float32)
            z_what = torch.empty(B, A, G, Gw, device=dev, dtype=torch.float32)
            z_depth, z_pres, p_z = (torch.empty(B, 1, G, Gw, device=dev, dtype=torch.float32) for _ in range(3))
            n_present = torch.empty(B, device=dev, dtype=torch.int32)
            L.check(lib.spair_prior_sample(ctypes.byref(d), float(st.count_prior_prob), L.ptr(cnt), *(L.ptr(noise[k]) for k in NOISE_MAPS),
                                           L.ptr(z_where), L.ptr(z_what), L.ptr(z_depth), L.ptr(z_pres), L.ptr(p_z), L.ptr(n_present),
                                           L.stream()), "spair_prior_sample")
            r = self.compose(z_where=z_where, z_what=z_what, z_depth=z_depth, z_pres=z_pres, layers=layers)
        return GenerateResult(z_where=z_where, z_what=z_what, z_depth=z_depth, z_pres=z_pres, p_z=p_z, count=n_present, recon=r.recon,
                              boxes=r.boxes, layers=r.layers, layer_weight=r.layer_weight)

    def evaluate(self, x, global_step=0, *, samples=1, sample=True, seed=None, noise=None, maps=True):
        """Score images under the model: the terms of the loss PER IMAGE, per cell and per pixel, as an ``EvalResult`` -- what
        ``loss_terms()`` cannot give (nine batch scalars, the BCE summed over the batch, the KLs divided by B * world_size).  Per draw: one
        ``no_grad`` forward, then ``spair_eval_terms`` on what it left in the workspace (kernel ``k_sample_terms``).

        ``terms[b]`` = (BCE_b + VAE_BETA * sum of the KLs, BCE_b, KL cy, cx, height, width, attr, depth, presence) in nats, unscaled;
        ``world_size`` plays no part in it.  The Gaussian KLs are masked by z_pres as in the loss; the presence KL uses the count prior's
        p_z as the forward stored it, so ``global_step`` moves it (the count-prior schedule) and nothing else.  ``kl_map`` / ``bce_map``
        say which cells spend the nats and which pixels carry the reconstruction error (``maps=False``: not computed).

        Draws: ``samples=K`` averages K draws (``terms``, the maps; ``terms_draws`` keeps each).  ``sample=False`` is the posterior mean
        (zero eps, u_pres = 0.5: constant maps) and needs ``samples == 1``.  ``noise`` is the dict ``forward`` takes, needs
        ``samples == 1`` and wins over ``seed``.  ``seed=int`` fills noise maps of this call's own from that seed (draw k: ``seed + k``)
        and touches NO torch generator, so it is safe inside a training run; ``seed=None`` draws one seed from torch's CPU generator as
        ``forward`` does (``torch.manual_seed`` controls it), then behaves as ``seed=int``.

        Like ``parse`` it overwrites the workspace of that batch size: ``backward()`` of an earlier forward of the same batch size raises
        afterwards (the generation check).  As any ``no_grad`` forward it leaves the word ``FusedAdam.step()`` reads as its skip flag
        alone: it may run between ``backward()`` and ``FusedAdam.step()``.  No gradients flow through it."""
        self._ensure_ready()
        if not x.is_cuda:
            raise L.SpairHipError("input must be on the MI355X (got %s); there is no CPU path" % x.device)
        x = x.contiguous().float()
        if list(x.shape[1:]) != list(self.image_shape):
            raise AssertionError("expected input [B,%s], got %s" % (self.image_shape, tuple(x.shape)))
        K = int(samples)
        if K < 1:
            raise AssertionError("evaluate: samples must be >= 1, got %r" % (samples,))
        if K > 1 and (noise is not None or not sample):
            raise AssertionError("evaluate: samples > 1 needs drawn noise (noise= and sample=False describe one draw)")
        if self.raise_on_nonfinite and self._status_host[0] != 0:
            raise L.SpairHipError(self._status_text(self._status_host[0]) + " -- seen by a later evaluate(); clear_step_status() to go on")
        e = self._engine(x.shape[0])
        d = e['dims']
        dev = x.device
        lib = L.lib()
        want = {k: tuple(v.shape) for k, v in e['noise'].items()}      # [B,{4,A,1,1},Gh,Gw]
        own = None
        if noise is not None:
            noise = {k: noise[k].to(dev).contiguous().float() for k in NOISE_MAPS}
            for k, v in noise.items():
                if tuple(v.shape) != want[k]:
                    raise AssertionError("noise[%r]: expected %s, got %s" % (k, want[k], tuple(v.shape)))
        elif not sample:
            noise = self._mean_noise(e)
        else:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            own = {k: torch.empty(want[k], device=dev, dtype=torch.float32) for k in NOISE_MAPS}
        (B, G), (Iw, Gw) = (d.B, d.G), dims_width(d)
        n_scratch = int(lib.spair_sample_terms_scratch_floats(B, G * Gw, d.I, Iw))
        if n_scratch <= 0:
            raise L.SpairHipError("evaluate: unsupported configuration (B=%d, %dx%d cells)" % (B, G, Gw))
        with torch.no_grad():
            draws = torch.empty(K, B, 9, device=dev, dtype=torch.float32)
            kl_map = torch.empty(B, 7, G, Gw, device=dev, dtype=torch.float32) if maps else None
            bce_map = torch.empty(B, d.I, Iw, device=dev, dtype=torch.float32) if maps else None
            scratch = torch.empty(n_scratch, device=dev, dtype=torch.float32)
            for k in range(K):
                if own is not None:
                    L.check(lib.spair_noise_fill(ctypes.byref(d), (int(seed) + k) & (2 ** 64 - 1), *(L.ptr(own[n]) for n in NOISE_MAPS),
                                                 L.stream()), "spair_noise_fill")
                    noise = own
                terms, recon, z_where, z_pres = self._run_forward(x, int(global_step), noise, train=False)
                L.check(lib.spair_eval_terms(ctypes.byref(d), L.ptr(e['workspace']), int(STEP_FLAGS), L.ptr(x), L.ptr(recon),
                                             float(d.vae_beta), L.ptr(draws[k]), L.ptr(kl_map), L.ptr(bce_map), L.ptr(scratch),
                                             int(k > 0), 1.0 / K, L.stream()), "spair_eval_terms")
            self._loss_terms = terms
            mean = draws.mean(0)
            return EvalResult(loss=mean[:, 0], terms=mean, terms_draws=draws, kl_map=kl_map, bce_map=bce_map, recon=recon,
                              z_where=z_where, z_pres=z_pres, loss_terms=terms[:9])

    def cell_rows(self, batch=None):
        """The cell-to-row table of the workspace of batch size ``batch`` (default: the latest forward's), int32 [G*Gw]: the per-cell rows
        of ``workspace_view`` for cell k = h * Gw + w are ``cell_rows()[k] * B + b`` (spair_cell_rows)."""
        e = self._last_engine() if batch is None else self._engine(batch)
        d = e['dims']
        out = torch.empty(d.G * dims_width(d)[1], device=self.device, dtype=torch.int32)
        L.check(L.lib().spair_cell_rows(ctypes.byref(d), L.ptr(e['workspace']), L.ptr(out), L.stream()), "spair_cell_rows")
        return out

    def _log_scalars(self):
        w = self.writer
        if isinstance(w, _NullWriter):
            return
        t = self._loss_terms
        w.add_scalar('training_wheel', self.training_wheel, self.global_step)
        w.add_scalar('losses/reconst', t[1], self.global_step)
        for i, n in enumerate(DIST_NAMES + ['pres_dist']):
            w.add_scalar('losses/KL{}'.format(n), t[2 + i], self.global_step)
        w.add_scalar('losses/total', t[0], self.global_step)

    def loss_terms(self):
        """Device tensor [9]: total, reconstruction BCE, KL cy,cx,height,width,attr,depth,pres (no sync)."""
        return self._loss_terms[:9]

    def _last_engine(self):
        last = getattr(self, "_last", None)
        if last is None:
            raise L.SpairHipError("no live forward pass: the model has not run yet, or the workspace of its latest forward was evicted by a "
                                  "forward of another batch size (max_engines)")
        return last['engine']

    # ---- failed / non-finite steps -------------------------------------------------------------------------
    @staticmethod
    def _status_text(bits):
        what = []
        if bits & 2:
            what.append("a training step produced a non-finite loss (NaN / inf in a loss term; the reference raises at that point: "
                        "debug_tools.py:245-271)")
        if bits & 1:
            what.append("a band-split hand-off of the per-cell chain timed out (preempted / oversubscribed GPU?): the results of that "
                        "workspace are not to be used -- restart the process, do not retry in place")
        if bits & 4:
            what.append("flagged on another rank: ddp.allreduce_gradients exchanged the step word and every replica left the step out "
                        "(the bits above that this rank did not see itself are the other rank's)")
        return "; ".join(what) or "ok"

    def step_status(self):
        """Bits of every forward of this model so far (sticky): 1 = a band-split hand-off timed out, 2 = a loss term was non-finite,
        4 = another rank flagged a step (ddp.allreduce_gradients; with the other rank's bits); 0 = clean.
        SYNCHRONISES -- call it where the host waits anyway (after ``loss.item()``, at the end of an epoch).  The same word is also
        kept in host memory the loss kernel writes to: ``forward()`` looks at it (a host load, no synchronisation) and raises once a
        failed step has completed, unless ``raise_on_nonfinite`` is off.  ``FusedAdam`` leaves a flagged step out (no NaN parameters)."""
        self._ensure_ready()
        return int(self._status_dev[0].item())

    def check_step_status(self):
        bits = self.step_status()
        if bits:
            raise L.SpairHipError(self._status_text(bits))

    def clear_step_status(self):
        """After a non-finite step that the caller has dealt with (the guarded optimizer skipped it): forget it.  A time-out (bit 1) stays in
        the workspace that saw it and comes back with its next forward."""
        self._ensure_ready()
        self._status_dev.zero_()
        torch.cuda.current_stream().synchronize()
        self._status_host[0] = 0

    def step_plan(self, batch):
        """The kernels a training step of batch size ``batch`` runs on its workspace under the current ``STEP_FLAGS`` (spair_step_plan:
        renderer family per direction, sprite / d-logit formats, fused chain, fused decoder; see ``_lib.step_plan``)."""
        e = self._engine(batch)
        return L.step_plan(e["dims"], e["workspace"].data_ptr(), STEP_FLAGS)

    def workspace_view(self, name, batch=None, padded=False):
        """A torch view (no copy) of buffer ``name`` of the workspace of batch size ``batch`` (default: the latest forward's) as the
        current ``STEP_FLAGS`` lay it out: [rows, cols] of its element type (``padded``: [rows, ld], the padding included).  Names and
        meaning: include/spair_hip.h, spair_workspace_view.  Nothing is aliased in the workspace, so after a step the view holds what that
        step's kernels read and wrote; it is valid until the next forward on that workspace (which overwrites it) or until the engine cache
        drops the workspace.  A diagnostic for tests: it does not synchronise."""
        if padded and name.startswith("lin_wt.") and name.endswith("output_layers.0"):
            raise ValueError("%s starts inside the rows it shares with its head's first layer: it has no padded view of its own" % name)
        e = self._last_engine() if batch is None else self._engine(batch)
        ws = e["workspace"]
        v = L.workspace_view(e["dims"], ws.data_ptr(), name, STEP_FLAGS)
        es = torch.empty((), dtype=v["dtype"]).element_size()
        width = v["ld"] if padded else v["cols"]
        t = ws[v["offset"]:v["offset"] + ((v["rows"] - 1) * v["ld"] + width) * es].view(v["dtype"])     # (no element past the last row)
        return t.as_strided((v["rows"], width), (v["ld"], 1))

    def chain_status(self):
        """Band-split hand-off status of the latest forward's workspace (grids wider than 16 cells): -1 where the chain runs unsplit, 0 = every
        hand-off arrived, 1 = a wait timed out (sticky; that step's loss and every later one is NaN).  SYNCHRONISES -- call it where the
        host waits anyway (after ``loss.item()``, at the end of an epoch); ``check_chain_status()`` raises instead of returning 1."""
        e = self._last_engine()
        out = torch.zeros(1, dtype=torch.int32, device=self.device)
        L.check(L.lib().spair_chain_sync_status(ctypes.byref(e['dims']), L.ptr(e['workspace']), L.ptr(out), L.stream()), "spair_chain_sync_status")
        return int(out.item())

    def check_chain_status(self):
        if self.chain_status() == 1:
            raise L.SpairHipError("a band-split hand-off of the per-cell chain timed out (preempted / oversubscribed GPU?): the results of this "
                                  "workspace are not to be used -- restart the process, do not retry in place")

    def export_map(self, which):
        """Per-cell quantity of the last forward as an NCHW map (see spair_export_map)."""
        e = self._last_engine()
        d = e['dims']
        ch = d.A if which in (0, 6, 12) else {0: 8, 1: 2 * d.A, 2: 2, 3: 1}[which % 100] if which >= 100 else 1
        out = torch.empty(d.B, ch, d.G, dims_width(d)[1], device=self.device, dtype=torch.float32)
        L.check(L.lib().spair_export_map(ctypes.byref(d), L.ptr(e['workspace']), int(which), L.ptr(out), L.stream()), "spair_export_map")
        return out


class _LazyDist(dict):
    """``self.dist_param[name]['mean'|'sigma']`` / ``self.dist[name]`` of the reference
    (models.py:122-125,441-448), materialised from the engine's row buffers on first access."""

    def __init__(self, model, as_normal=False):
        super().__init__()
        self._m, self._n = model, as_normal

    def __missing__(self, name):
        i = DIST_NAMES.index(name)
        mean, sigma = self._m.export_map(2 + i), self._m.export_map(8 + i)
        if self._n:
            from torch.distributions import Normal
            v = Normal(loc=mean, scale=sigma)
        else:
            v = {'mean': mean, 'sigma': sigma}
        self[name] = v
        return v

    def keys(self):
        return DIST_NAMES

    def items(self):
        return [(n, self[n]) for n in DIST_NAMES]


class _SelfAttnParams(nn.Module):
    """Parameter container for the reference's Self_Attn(55) (models.py:667-699).  Its output is
    discarded there and its parameters never get gradients; only the state_dict entries matter."""

    def __init__(self, in_dim):
        super().__init__()
        self.chanel_in = in_dim
        self.query_conv = nn.Conv2d(in_dim, in_dim // 8, kernel_size=1)
        self.key_conv = nn.Conv2d(in_dim, in_dim // 8, kernel_size=1)
        self.value_conv = nn.Conv2d(in_dim, in_dim, kernel_size=1)
        self.gamma = nn.Parameter(torch.zeros(1))
