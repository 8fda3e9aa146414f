"""Data-parallel SPAIR over the GPUs of one node: one process per GPU, replicated 1.46 M-parameter
model, a SUM all-reduce (RCCL over xGMI; gloo in the CPU tests / one-GPU rehearsals) of the flat fp32
gradient buffer, issued in THREE BUCKETS in the order the hand-written backward completes them and
overlapped with the backward kernels that are still running.

Loss scaling: the reference's loss is  sum_batch BCE + mean_batch KL
(models.py:547,553,558).  For S ranks to equal one process on the global batch, each rank
back-propagates  BCE_sum_local + KL_sum_local / (B_local * S)  and the gradients are SUMMED --
plain DDP averaging would silently divide the reconstruction gradient by S.  The model does this
when ``world_size`` is set; ``global_loss`` rebuilds the reported ELBO the same way.

Overlap: ``spair_backward`` (include/spair_hip.h, ``SpairStepIO.ev_*``) records one event per gradient range as soon as
that range is final -- decoder first (its weight gradients run on the engine's helper stream under
the per-cell backward chain), then the box / encoder / z / obj nets, last the backbone with the edge
element.  ``allreduce_gradients(model)`` makes a communication stream wait on each event and starts
that range's all-reduce there, so the decoder's 1.7 MB travel while the chain and the backbone
backward still compute; Adam (on the caller's stream) waits on the last collective.  The reference
has no counterpart (train.py:27-30 is single-device).

A failed step (optim.py): ``FusedAdam.step()`` leaves out a step whose loss was flagged non-finite or timed out, and it reads a word in
this rank's own memory.  ``allreduce_gradients(model)`` therefore exchanges that word too -- two ints, a MAX all-reduce beside the first
gradient bucket (spair_status_exchange) -- so that every rank takes the SAME decision: a step any rank flagged is left out on all of
them, parameters, moments and ``skipped()[0]`` stay equal across replicas, and every rank is loud afterwards (``check_step_status()``
and the next ``forward()`` raise everywhere, a rank flagged only through another one says so: bit 4), so no rank walks on into a
collective the flagged rank never reaches.  The flat-tensor form knows no model: there the caller owns that exchange.

Gradient clipping (``FusedAdam(max_grad_norm=...)``, ``optim.clip_grad_norm_``) belongs after ``allreduce_gradients``:
``FusedAdam.step()`` is already ordered behind the collectives on the caller's stream, and the norm is then that of
the summed global gradient, the same on every rank.
"""
import ctypes

import torch
import torch.distributed as dist

from . import _lib as L

BUCKET_NAMES = ("decoder", "cell_nets", "backbone+edge")


class GradBuckets:
    """The three readiness events + flat-buffer ranges of a model (created by ``attach``)."""

    def __init__(self, model, timing=False):
        lib = L.lib()
        d = model._dims(1)
        lo, hi = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
        L.check(lib.spair_grad_buckets(ctypes.byref(d), lo, hi), "spair_grad_buckets")
        self.ranges = [(int(lo[i]), int(hi[i])) for i in range(3)]
        dev = model.device
        with torch.cuda.device(dev):
            self.events = [torch.cuda.Event(enable_timing=bool(timing)) for _ in range(3)]      # timing: the overlap-window measurement only
            for e in self.events:
                e.record()                 # materialises the hipEvent_t behind the torch object
            self.comm = torch.cuda.Stream(device=dev)
            # timing: per bucket, when its all-reduce could start (its range was final) and when it had completed, on the communication stream
            self.t_start = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timing else None
            self.t_done = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timing else None
        self.timing = bool(timing)
        self.pending = False

    def handles(self):
        return [ctypes.c_void_p(e.cuda_event) for e in self.events]


def attach(model, world_size=None, overlap=True, timing=False):
    """Marks ``model`` as one of ``world_size`` replicas (sharded-loss scaling) and, with ``overlap``,
    arms the bucket events its backward records.  ``overlap=False`` (bench.py: SPAIR_DDP_OVERLAP=0) keeps the
    plain path: one all-reduce of the whole flat gradient on the caller's stream after the backward."""
    model.world_size = int(world_size if world_size is not None else dist.get_world_size())
    model._grad_buckets = GradBuckets(model, timing) if (overlap and model.device.type == "cuda" and model.world_size > 1) else None
    return model


def broadcast_parameters(flat_params, src=0):
    dist.broadcast(flat_params, src)


def _exchange_status(model, phase):
    """spair_status_exchange on the current stream: phase 0 packs the model's step word into its two exchange ints, phase 1 merges the
    all-reduced ints back into the step word, the sticky word and the host word.  No allocation after the first call."""
    status = getattr(model, "_status_dev", None)
    if status is None:
        return None
    x = getattr(model, "_status_xchg", None)
    if x is None or x.device != status.device:
        x = model._status_xchg = torch.zeros(2, dtype=torch.int32, device=status.device)
    host = ctypes.cast(model._status_host, ctypes.c_void_p) if model._status_host is not None else ctypes.c_void_p(0)
    L.check(L.lib().spair_status_exchange(L.ptr(status), L.ptr(x), host, int(phase), L.stream()), "spair_status_exchange")
    return x


def allreduce_gradients(target):
    """SUM (not mean) over ranks, in place.  ``target`` is a model prepared by ``attach`` (bucketed, overlapped
    with the tail of its backward) or a flat gradient tensor (one bucket, on the current stream).

    With a model, the word ``FusedAdam.step()`` reads as its skip flag is exchanged as well (MAX over ranks, one collective of two
    ints): after this call every rank leaves the step out if any rank flagged it.  With a flat tensor nothing is known of a model:
    the caller owns that exchange (or every rank may take its own decision and the replicas diverge)."""
    if isinstance(target, torch.Tensor):
        dist.all_reduce(target, op=dist.ReduceOp.SUM)
        return
    model = target
    flat = model.flat_gradients()
    gb = getattr(model, "_grad_buckets", None)
    if gb is None or not gb.pending:
        xchg = _exchange_status(model, 0)
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        if xchg is not None:
            dist.all_reduce(xchg, op=dist.ReduceOp.MAX)
            _exchange_status(model, 1)
        return
    gb.pending = False
    works = []
    xchg = None
    with torch.cuda.stream(gb.comm):
        for i, (ev, (lo, hi)) in enumerate(zip(gb.events, gb.ranges)):
            gb.comm.wait_event(ev)                       # this range's gradients are final
            if gb.timing:
                gb.t_start[i].record(gb.comm)
            w = dist.all_reduce(flat[lo:hi], op=dist.ReduceOp.SUM, async_op=True)
            if gb.timing:
                w.wait()                                 # the communication stream waits for the collective: `t_done` is its completion
                gb.t_done[i].record(gb.comm)
            works.append(w)
            if i == 0:
                # the step word was final with the forward's loss kernel, long before the first range: its two ints travel behind the
                # first bucket (after that bucket's timing marks, which stay the gradient collective's own)
                xchg = _exchange_status(model, 0)
                if xchg is not None:
                    works.append(dist.all_reduce(xchg, op=dist.ReduceOp.MAX, async_op=True))
    for w in works:
        w.wait()                                         # the CALLER's stream (Adam) waits for the collectives
    torch.cuda.current_stream().wait_stream(gb.comm)
    if xchg is not None:
        _exchange_status(model, 1)                       # on the caller's stream, in front of Adam


def bucket_timings(model, backward_end=None):
    """After a synchronised step of a model attached with ``timing=True``: per gradient bucket, the bytes, the time from "range final" to
    "all-reduce complete" on the communication stream and (given the event recorded behind ``loss.backward()``) how long before the end of the
    backward the range was final -- whether the window hides the collective is then one comparison."""
    gb = getattr(model, "_grad_buckets", None)
    if gb is None or not gb.timing:
        return None
    out = []
    for i, (lo, hi) in enumerate(gb.ranges):
        rec = dict(bucket=BUCKET_NAMES[i], bytes=4 * (hi - lo), allreduce_ms=gb.t_start[i].elapsed_time(gb.t_done[i]))
        if backward_end is not None:
            rec["ready_before_backward_end_ms"] = gb.events[i].elapsed_time(backward_end)
            rec["done_after_backward_end_ms"] = backward_end.elapsed_time(gb.t_done[i])
        out.append(rec)
    return out


def global_loss(loss_terms):
    """loss_terms[0..8] of each rank (total, BCE_sum_local, KL_k_local/(B*S)) -> global ELBO terms."""
    t = loss_terms.clone()
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t
