"""Fused Adam (K9) over the model's flat parameter / gradient buffers: one launch per step.
Numerically torch.optim.Adam(lr) with its defaults (train.py:44).

Guarded (spair_adam_guarded).  The contract of a failed step:
  * ``step()`` leaves the step out whole -- parameters and both moments untouched -- if ANY grad-enabled forward of the model since the
    previous ``step()`` flagged a non-finite or timed-out loss: the loss kernel ORs into one device word per optimizer step
    (``SpairStep.status[1]``), so a flagged micro-batch under gradient accumulation holds whatever the later ones did, and ``step()``
    clears the word behind the Adam kernel.  ``skipped()[0]`` counts such a step once.
  * no ``no_grad`` forward, ``parse``, ``evaluate``, ``compose`` or ``generate`` changes that word, wherever it falls between
    ``backward()`` and ``step()``.
  * data-parallel replicas take the same decision: ``ddp.allreduce_gradients(model)`` exchanges the word, and a step any rank flagged
    is left out on all of them (ddp.py).
  * an element whose gradient is NaN / inf is left out on its own; ``lr * NaN`` never reaches a parameter.
  * a single-process step pays one word-sized device fill for this: no synchronisation, no allocation, and the whole step stays
    capturable in a HIP graph.
``skipped()`` reports both (synchronises), ``model.forward`` raises on the flag by itself once the failed step has completed (models.py).

Clipped (``max_grad_norm``; spair_grad_norm + spair_adam_clipped, csrc/gradnorm.hip): the gradients are scaled by
``min(1, max_grad_norm / (norm + norm_eps))``, norm = the global L2 norm of the flat gradient buffer -- torch.nn.utils.clip_grad_norm_ in
front of the same Adam -- inside the Adam kernel, from a device scalar: three launches, no allocation, no synchronisation, the gradient
buffer is not written.  The norm is summed in float64 in a fixed order (bit-identical from run to run given the same gradient buffer;
finite wherever the true norm is).  A step whose norm is not finite is left out whole.  ``clip_grad_norm_`` and ``grad_norms`` are the
same pass for the stock torch.optim.Adam loop and for looking at where the gradient mass is."""
import ctypes
import math

import torch

from . import _lib as L


def check_max_grad_norm(value, what="max_grad_norm"):
    """``value`` as a float if it is a positive finite number, else ValueError (a bool is not a number here)."""
    ok = isinstance(value, (int, float)) and not isinstance(value, bool) and math.isfinite(value) and value > 0
    if not ok:
        raise ValueError("%s must be a positive finite float (None: no clipping), got %r" % (what, value))
    return float(value)


def _check_norm_eps(value):
    if not isinstance(value, (int, float)) or isinstance(value, bool) or not math.isfinite(value) or value < 0:
        raise ValueError("norm_eps must be a finite float >= 0, got %r" % (value,))
    return float(value)


class _GradNorm:
    """The tables and buffers spair_grad_norm needs for one flat gradient buffer: the segment table (every parameter of
    ``model._slices`` in flat-buffer order), its work items on the device, the per-item and per-segment float64 sums, ``out`` =
    (norm, scale) and the two ``clip`` counters.  Built once per buffer: ``run`` allocates nothing and never synchronises."""

    def __init__(self, model):
        grads = model.flat_gradients()
        segs = sorted((off, off + cnt, key) for key, (off, cnt, _) in model._slices.items())
        self.names = [key for _, _, key in segs]
        self.ranges = [(lo, hi) for lo, hi, _ in segs]
        self.nseg = len(segs)
        lo = (ctypes.c_int64 * self.nseg)(*(r[0] for r in self.ranges))
        hi = (ctypes.c_int64 * self.nseg)(*(r[1] for r in self.ranges))
        f, n = L.lib().spair_grad_norm_items, ctypes.c_int64(grads.numel())
        self.n_items = int(f(lo, hi, self.nseg, n, None))
        if self.n_items < 0:
            raise L.SpairHipError("spair_grad_norm_items refused the parameter layout (code %d)" % self.n_items)
        items = (ctypes.c_int64 * (3 * self.n_items))()
        f(lo, hi, self.nseg, n, items)
        dev = grads.device
        self.items = torch.tensor(list(items), dtype=torch.int64).to(dev)
        self.partial = torch.zeros(self.n_items, dtype=torch.float64, device=dev)
        self.seg_sumsq = torch.zeros(self.nseg, dtype=torch.float64, device=dev)
        self.out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.clip = torch.zeros(2, dtype=torch.int32, device=dev)
        self.grads_ptr = grads.data_ptr()
        self._bucket_index = None

    def run(self, max_norm, norm_eps=0.0):
        """Enqueue the norm of the buffer as it is now on the caller's stream (max_norm <= 0: measure only, scale = 1)."""
        L.check(L.lib().spair_grad_norm(ctypes.c_void_p(self.grads_ptr), L.ptr(self.items), self.n_items, self.nseg, L.ptr(self.partial),
                                        L.ptr(self.seg_sumsq), L.ptr(self.out), float(max_norm), float(norm_eps), L.ptr(self.clip),
                                        L.stream()), "spair_grad_norm")

    def bucket_index(self, model):
        """int64 [nseg] on the device: the spair_grad_buckets range (ddp.BUCKET_NAMES order) each parameter lies in, 3 for one in none."""
        if self._bucket_index is None:
            d = model._dims(1)
            lo, hi = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
            L.check(L.lib().spair_grad_buckets(ctypes.byref(d), lo, hi), "spair_grad_buckets")
            idx = [next((b for b in range(3) if lo[b] <= a and e <= hi[b]), 3) for a, e in self.ranges]
            self._bucket_index = torch.tensor(idx, dtype=torch.int64).to(self.out.device)
        return self._bucket_index


def _grad_norm_state(model):
    """The model's own _GradNorm (clip_grad_norm_ / grad_norms), rebuilt when its flat gradient buffer is."""
    grads = model.flat_gradients()
    gn = getattr(model, "_grad_norm_tables", None)
    if gn is None or gn.grads_ptr != grads.data_ptr():
        gn = _GradNorm(model)
        model._grad_norm_tables = gn
    return gn


class GradNorms:
    """What ``grad_norms`` returns, all on the device: ``total`` (0-dim fp32, the global L2 norm of the flat gradient buffer),
    ``per_parameter`` fp32 [n_params] and ``names`` (the parameters in flat-buffer order), ``buckets`` fp32 [3]: the norm over the
    parameters of each all-reduce bucket, in ``ddp.BUCKET_NAMES`` order."""
    __slots__ = ("total", "per_parameter", "names", "buckets")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __repr__(self):
        return "GradNorms(total=(), per_parameter=%s, names=[%d], buckets=%s)" % (tuple(self.per_parameter.shape), len(self.names),
                                                                                 tuple(self.buckets.shape))

    def as_dict(self):
        """{parameter name: norm} as Python floats.  SYNCHRONISES."""
        return dict(zip(self.names, self.per_parameter.tolist()))


def grad_norms(model):
    """Where the gradient mass is: the L2 norm of ``model.flat_gradients()`` as it is now, in total, per parameter and per all-reduce
    bucket (a ``GradNorms``), from one pass of spair_grad_norm in float64.  Measures only: the gradients are untouched; no
    synchronisation."""
    gn = _grad_norm_state(model)
    gn.run(0.0)
    buckets = torch.zeros(4, dtype=torch.float64, device=gn.out.device).index_add_(0, gn.bucket_index(model), gn.seg_sumsq)[:3]
    return GradNorms(total=gn.out[0].clone(), per_parameter=gn.seg_sumsq.sqrt().float(), names=list(gn.names),
                     buckets=buckets.sqrt().float())


def clip_grad_norm_(model, max_norm, norm_eps=1e-6):
    """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) for the stock torch.optim.Adam loop (train.py:64-67), on the flat
    gradient buffer: scales every gradient by min(1, max_norm / (norm + norm_eps)) in place and returns the norm from before the
    scaling as a 0-dim device tensor.  Two kernels and one multiply by the device scalar: no synchronisation.  Unlike torch, which
    turns every gradient into NaN when the norm is not finite, this leaves the buffer as it is (scale 1) and returns the non-finite
    norm -- FusedAdam's element guard then deals with the elements.  ``max_norm``: a positive finite Python float (it is passed to
    the kernel by value; a device tensor would have to be synchronised on)."""
    max_norm, norm_eps = check_max_grad_norm(max_norm, "max_norm"), _check_norm_eps(norm_eps)
    gn = _grad_norm_state(model)
    model._bind_grads()
    gn.run(max_norm, norm_eps)
    model.flat_gradients().mul_(gn.out[1])
    return gn.out[0].clone()


class FusedAdam:
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, norm_eps=1e-6):
        self.model, self.lr, self.betas, self.eps = model, lr, betas, eps
        self.max_grad_norm = None if max_grad_norm is None else check_max_grad_norm(max_grad_norm)
        self.norm_eps = _check_norm_eps(norm_eps)
        self.step_count = 0
        self._state_for = None
        self._counters = None       # device ints: [whole steps left out (non-finite loss), 1 if any element was ever left out (non-finite gradient)]
        self._gn = None             # with max_grad_norm: the _GradNorm of the model's flat gradient buffer
        self._clipped_once = False

    def _state(self):
        flat = self.model.flat_parameters()
        if self._state_for != flat.data_ptr():
            # (re)flattened parameters (first use, model.to(), load_state_dict(assign=True)): the moments follow the buffer -- copied when
            # the layout is unchanged, so that step_count and the bias correction stay consistent with them
            old_m, old_v = getattr(self, "exp_avg", None), getattr(self, "exp_avg_sq", None)
            self.exp_avg = torch.zeros_like(flat)
            self.exp_avg_sq = torch.zeros_like(flat)
            if old_m is not None and old_m.numel() == flat.numel():
                self.exp_avg.copy_(old_m.to(flat.device))
                self.exp_avg_sq.copy_(old_v.to(flat.device))
            elif old_m is not None:
                self.step_count = 0
            self._state_for = flat.data_ptr()
        if self._counters is None or self._counters.device != flat.device:
            self._counters = torch.zeros(2, dtype=torch.int32, device=flat.device)
        if self.max_grad_norm is not None and (self._gn is None or self._gn.grads_ptr != self.model.flat_gradients().data_ptr()):
            # the gradient buffer is rebuilt with the parameter buffer: new tables, the counters carried over
            old, self._gn = self._gn, _GradNorm(self.model)
            if old is not None:
                self._gn.clip.copy_(old.clip)
        return flat

    def zero_grad(self, set_to_none=False):
        self.model.flat_gradients().zero_()

    def step(self):
        flat = self._state()
        self.model._bind_grads()
        self.step_count += 1
        status = getattr(self.model, "_status_dev", None)
        skip = ctypes.c_void_p(status.data_ptr() + 4) if status is not None else ctypes.c_void_p(0)       # this optimizer step's bits
        if self.max_grad_norm is not None:
            return self._step_clipped(flat, skip)
        L.check(L.lib().spair_adam_guarded(L.ptr(flat), L.ptr(self.model.flat_gradients()), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                                           ctypes.c_int64(flat.numel()), ctypes.c_float(self.lr), ctypes.c_float(self.betas[0]),
                                           ctypes.c_float(self.betas[1]), ctypes.c_float(self.eps), int(self.step_count), skip,
                                           L.ptr(self._counters), L.stream()),
                "spair_adam_guarded")
        self._clear_step_word(status)

    @staticmethod
    def _clear_step_word(status):
        """The word belongs to the optimizer step that has just read it: the next step starts from a clean one (a fill of one int on the
        caller's stream, behind the Adam kernel; the sticky word and the host word keep the failure loud)."""
        if status is not None:
            status[1].zero_()

    def _step_clipped(self, flat, skip):
        self._gn.run(self.max_grad_norm, self.norm_eps)
        L.check(L.lib().spair_adam_clipped(L.ptr(flat), L.ptr(self.model.flat_gradients()), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                                           ctypes.c_int64(flat.numel()), ctypes.c_float(self.lr), ctypes.c_float(self.betas[0]),
                                           ctypes.c_float(self.betas[1]), ctypes.c_float(self.eps), int(self.step_count), skip,
                                           L.ptr(self._counters), L.ptr(self._gn.out), L.stream()),
                "spair_adam_clipped")
        self._clear_step_word(getattr(self.model, "_status_dev", None))
        self._clipped_once = True

    @property
    def grad_norm(self):
        """0-dim fp32 device tensor: the global gradient norm of the last ``step()``, before clipping (a view: the next step overwrites
        it; no synchronisation).  None without ``max_grad_norm`` or before the first step."""
        return self._gn.out[0] if self._clipped_once and self._gn is not None else None

    @property
    def clip_scale(self):
        """0-dim fp32 device tensor: the factor the last ``step()`` applied to its gradients (1 = not clipped), as ``grad_norm``."""
        return self._gn.out[1] if self._clipped_once and self._gn is not None else None

    def clip_stats(self):
        """dict(steps_clipped, steps_nonfinite_norm, last_norm, last_scale).  SYNCHRONISES.  A step with a non-finite norm was left out
        whole (it is not among ``skipped()``'s, which counts the steps whose loss was non-finite)."""
        if self._gn is None or not self._clipped_once:
            return dict(steps_clipped=0, steps_nonfinite_norm=0, last_norm=None, last_scale=None)
        c, o = self._gn.clip.tolist(), self._gn.out.tolist()
        return dict(steps_clipped=int(c[0]), steps_nonfinite_norm=int(c[1]), last_norm=float(o[0]), last_scale=float(o[1]))

    def skipped(self):
        """(steps left out because their loss was non-finite, whether any single element was ever left out for a non-finite gradient).
        SYNCHRONISES.  A left-out step still advanced ``step_count`` (the bias correction runs one step ahead per skip: 1e-3 relative
        on the update after a thousand steps)."""
        self._state()
        c = self._counters.tolist()
        return int(c[0]), bool(c[1])

    def state_dict(self):
        self._state()
        return dict(step=self.step_count, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, lr=self.lr, betas=self.betas, eps=self.eps,
                    max_grad_norm=self.max_grad_norm, norm_eps=self.norm_eps)

    def load_state_dict(self, sd):
        self._state()
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.lr = float(sd.get("lr", self.lr))
        self.betas = tuple(sd.get("betas", self.betas))
        self.eps = float(sd.get("eps", self.eps))
        mgn = sd.get("max_grad_norm", self.max_grad_norm)          # a checkpoint from before clipping has neither key
        self.max_grad_norm = None if mgn is None else check_max_grad_norm(mgn)
        self.norm_eps = _check_norm_eps(sd.get("norm_eps", self.norm_eps))
