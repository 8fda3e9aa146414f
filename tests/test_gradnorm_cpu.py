"""Gradient-norm clipping without a GPU: the work-item table of spair_grad_norm_items against its Python restatement, what the three entry
points refuse before any launch (the library loads without a device; no call here reaches a kernel launch, and no pointer is read), the
optimizer's argument check, and which entry points FusedAdam.step() issues with and without ``max_grad_norm``."""
import ctypes
import math

import pytest

from gradnorm_helpers import ERR_SHAPE, i64, items_lib, items_ref, layout


@pytest.fixture(scope="module")
def lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def test_chunk_is_a_multiple_of_1024(lib):
    ch = lib.spair_grad_chunk()
    assert ch >= 1024 and ch % 1024 == 0


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_items_of_one_segment(lib, start):
    ch = lib.spair_grad_chunk()
    for n in (1, ch - 1, ch, ch + 1, 2 * ch + 3):
        k, table = items_lib(lib, [start], [start + n], start + n + 3)
        ref = items_ref([start], [start + n], ch)
        assert k == len(ref) // 3 == -(-n // ch) and table == ref, (start, n)
        assert all(0 < table[3 * i + 2] - table[3 * i + 1] <= ch for i in range(k))


def test_items_of_segments_with_gaps(lib):
    ch = lib.spair_grad_chunk()
    segs, end = layout([1, 1, 7, ch + 1, 3, 2 * ch], [0, 1, 2, 3, 4, 5], start=1)
    lo, hi = [s[0] for s in segs], [s[1] for s in segs]
    k, table = items_lib(lib, lo, hi, end + 2)
    assert table == items_ref(lo, hi, ch) and k == 1 + 1 + 1 + 2 + 1 + 2
    # every element of every segment is in exactly one item, no element of a gap in any
    covered = sorted(e for i in range(k) for e in range(table[3 * i + 1], table[3 * i + 2]))
    assert covered == [e for a, b in segs for e in range(a, b)]
    assert [table[3 * i] for i in range(k)] == sorted(table[3 * i] for i in range(k))


def _items(lib, lo, hi, n, nseg=None):
    return lib.spair_grad_norm_items(i64(lo), i64(hi), len(lo) if nseg is None else nseg, n, None)


def test_items_refusals(lib):
    assert _items(lib, [0], [4], 0) == ERR_SHAPE                       # n <= 0
    assert _items(lib, [0], [4], -5) == ERR_SHAPE
    assert _items(lib, [0], [4], 8, nseg=0) == ERR_SHAPE               # nseg < 1
    assert _items(lib, [0] * 4097, [1] * 4097, 8) == ERR_SHAPE         # nseg above the cap, before the table is read
    assert _items(lib, [2], [2], 8) == ERR_SHAPE                       # empty
    assert _items(lib, [4], [2], 8) == ERR_SHAPE                       # descending
    assert _items(lib, [0, 3], [4, 6], 8) == ERR_SHAPE                 # overlapping
    assert _items(lib, [4, 0], [6, 2], 8) == ERR_SHAPE                 # not ascending
    assert _items(lib, [-1], [2], 8) == ERR_SHAPE                      # in front of the buffer
    assert _items(lib, [0, 6], [4, 9], 8) == ERR_SHAPE                 # past n
    assert lib.spair_grad_norm_items(None, i64([4]), 1, 8, None) == ERR_SHAPE
    assert lib.spair_grad_norm_items(i64([0]), None, 1, 8, None) == ERR_SHAPE
    assert _items(lib, [0, 4], [4, 8], 8) == 2                         # adjacent segments up to n are fine


def _grad_norm(lib, null=None, n_items=2, nseg=2, max_norm=1.0, norm_eps=1e-6):
    """Dummy non-null pointers (never read: every call is refused before a launch), ``null`` names the one passed as NULL."""
    dummy = ctypes.c_void_p(64)
    ptrs = {k: (None if k == null else dummy) for k in ("grads", "items", "partial", "seg_sumsq", "out", "clip")}
    return lib.spair_grad_norm(ptrs["grads"], ptrs["items"], n_items, nseg, ptrs["partial"], ptrs["seg_sumsq"], ptrs["out"],
                               max_norm, norm_eps, ptrs["clip"], None)


def test_grad_norm_refusals(lib):
    for null in ("grads", "items", "partial", "seg_sumsq", "out", "clip"):
        assert _grad_norm(lib, null=null) == ERR_SHAPE, null
    assert _grad_norm(lib, nseg=0) == ERR_SHAPE
    assert _grad_norm(lib, nseg=4097, n_items=5000) == ERR_SHAPE
    assert _grad_norm(lib, n_items=0) == ERR_SHAPE
    assert _grad_norm(lib, n_items=1, nseg=2) == ERR_SHAPE             # fewer items than (non-empty) segments
    assert _grad_norm(lib, n_items=2 ** 31) == ERR_SHAPE
    assert _grad_norm(lib, norm_eps=-1e-6) == ERR_SHAPE
    assert _grad_norm(lib, norm_eps=math.nan) == ERR_SHAPE
    assert _grad_norm(lib, max_norm=math.nan) == ERR_SHAPE


def _adam_clipped(lib, null=None, n=8, step=1):
    dummy = ctypes.c_void_p(64)
    ptrs = {k: (None if k == null else dummy) for k in ("params", "grads", "m", "v", "skip", "counters", "norm_out")}
    return lib.spair_adam_clipped(ptrs["params"], ptrs["grads"], ptrs["m"], ptrs["v"], n, 1e-3, 0.9, 0.999, 1e-8, step, ptrs["skip"],
                                  ptrs["counters"], ptrs["norm_out"], None)


def test_adam_clipped_refusals(lib):
    for null in ("params", "grads", "m", "v", "counters", "norm_out"):
        assert _adam_clipped(lib, null=null) == ERR_SHAPE, null
    assert _adam_clipped(lib, n=0) == ERR_SHAPE
    assert _adam_clipped(lib, n=-3) == ERR_SHAPE
    assert _adam_clipped(lib, step=0) == ERR_SHAPE


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1.0, math.nan, math.inf, -math.inf, True, "1.0"])
def test_max_grad_norm_must_be_positive_and_finite(bad):
    from spair_pytorch_amd.optim import FusedAdam, check_max_grad_norm, clip_grad_norm_
    with pytest.raises(ValueError):
        FusedAdam(object(), max_grad_norm=bad)             # refused before the model is looked at
    with pytest.raises(ValueError):
        check_max_grad_norm(bad)
    with pytest.raises(ValueError):
        clip_grad_norm_(object(), bad)


def test_max_grad_norm_accepted_values():
    from spair_pytorch_amd.optim import FusedAdam
    assert FusedAdam(object()).max_grad_norm is None
    assert FusedAdam(object(), max_grad_norm=5).max_grad_norm == 5.0
    assert FusedAdam(object(), max_grad_norm=1e30, norm_eps=0.0).norm_eps == 0.0
    with pytest.raises(ValueError):
        FusedAdam(object(), max_grad_norm=1.0, norm_eps=-1e-6)


class _FlatModel:
    """What FusedAdam reads of a model: the two flat buffers (host tensors here: nothing is launched), the parameter slices."""

    def __init__(self, sizes):
        import torch
        self._slices, at = {}, 0
        for i, n in enumerate(sizes):
            self._slices["p%d" % i] = (at, n, (n,))
            at += n + (i % 3)                                  # gaps, as a padded layout has
        self._p, self._g = torch.zeros(at), torch.zeros(at)

    def flat_parameters(self):
        return self._p

    def flat_gradients(self):
        return self._g

    def _bind_grads(self):
        pass


class _Recorder:
    """The library with its three step entry points replaced by recorders (the host-only ones stay the real ones)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in ("spair_adam_guarded", "spair_grad_norm", "spair_adam_clipped", "spair_adam"):
            return lambda *a: self.calls.append((name, a)) or 0
        return getattr(self._lib, name)


def test_step_issues_the_guarded_call_alone_without_max_grad_norm(lib, monkeypatch):
    """Contract (a): FusedAdam(model, lr) launches exactly what it launched before -- one spair_adam_guarded; with max_grad_norm,
    spair_grad_norm on the model's segment table and then spair_adam_clipped reading that call's ``out``."""
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd.optim import FusedAdam
    rec = _Recorder(lib)
    monkeypatch.setattr(L, "lib", lambda: rec)
    monkeypatch.setattr(L, "stream", lambda: ctypes.c_void_p(0))
    ch = lib.spair_grad_chunk()
    model = _FlatModel([5, ch + 1, 1, 2 * ch])
    plain = FusedAdam(model, lr=1e-3)
    plain.step()
    plain.step()
    assert [c[0] for c in rec.calls] == ["spair_adam_guarded"] * 2
    assert plain.grad_norm is None and plain.clip_scale is None and plain._gn is None
    assert plain.clip_stats() == dict(steps_clipped=0, steps_nonfinite_norm=0, last_norm=None, last_scale=None)
    assert plain.state_dict()["max_grad_norm"] is None
    del rec.calls[:]
    clipped = FusedAdam(model, lr=1e-3, max_grad_norm=2.5, norm_eps=1e-5)
    assert clipped.grad_norm is None
    clipped.step()
    clipped.step()
    assert [c[0] for c in rec.calls] == ["spair_grad_norm", "spair_adam_clipped"] * 2
    norm_args, adam_args = rec.calls[2][1], rec.calls[3][1]
    gn = clipped._gn
    assert gn.names == ["p0", "p1", "p2", "p3"] and gn.n_items == 1 + 2 + 1 + 2 and norm_args[2] == gn.n_items and norm_args[3] == 4
    assert gn.items.tolist() == items_ref([r[0] for r in gn.ranges], [r[1] for r in gn.ranges], ch)
    assert norm_args[7] == 2.5 and norm_args[8] == 1e-5
    assert norm_args[6].value == gn.out.data_ptr() == adam_args[12].value           # the scale travels through device memory
    assert adam_args[9] == 2                                                         # Adam's step count
    sd = clipped.state_dict()
    assert sd["max_grad_norm"] == 2.5 and sd["norm_eps"] == 1e-5
    # a state dict from before clipping existed keeps the constructor's values; one with the keys overrides them
    old = {k: v for k, v in sd.items() if k not in ("max_grad_norm", "norm_eps")}
    clipped.load_state_dict(old)
    assert clipped.max_grad_norm == 2.5 and clipped.norm_eps == 1e-5
    plain.load_state_dict(old)
    assert plain.max_grad_norm is None
    plain.load_state_dict(sd)
    assert plain.max_grad_norm == 2.5 and plain.norm_eps == 1e-5
