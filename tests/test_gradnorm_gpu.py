"""Gradient-norm clipping on the MI355X (include/spair_hip.h, "gradient norm and clipping"; csrc/gradnorm.hip).  First straight through the
C ABI on torch tensors -- the float64 norm at every head / tail / chunk edge, run-to-run identity, the non-finite rule, the clipped Adam
against the guarded one (scale 1: to the bit) and against CPU torch clip_grad_norm_ + torch.optim.Adam -- then on a model: grad_norms,
FusedAdam(max_grad_norm=...), clip_grad_norm_, the checkpoint and a captured step.  References are numpy / CPU torch in float64."""
import os

import numpy as np
import pytest
import torch

from gradnorm_helpers import NORM_RTOL, GradNormCall, adam, layout, norm64

pytestmark = pytest.mark.gpu


def _chunk():
    from spair_pytorch_amd import _lib as L
    return L.lib().spair_grad_chunk()


def _nan_buffer(total, segs, rng, scales=None):
    """A host fp32 buffer of NaN with standard-normal values (times scales[s]) inside the segments."""
    host = np.full(total, np.nan, dtype=np.float32)
    for s, (lo, hi) in enumerate(segs):
        host[lo:hi] = (rng.standard_normal(hi - lo) * (1.0 if scales is None else scales[s])).astype(np.float32)
    return host


def _assert_norms(call, host, segs):
    """Contract (c), total and per segment, against float64 numpy on the same fp32 values."""
    out, seg = call.out.cpu().numpy(), call.seg_sumsq.cpu().numpy()
    ref_seg = [norm64(host[lo:hi]) for lo, hi in segs]
    ref = float(np.sqrt(sum(r * r for r in ref_seg)))
    assert np.isfinite(out[0]) and abs(float(out[0]) - ref) <= NORM_RTOL * ref, (float(out[0]), ref)
    for s, r in enumerate(ref_seg):
        assert abs(float(np.sqrt(seg[s])) - r) <= NORM_RTOL * r, (s, float(np.sqrt(seg[s])), r)
    assert out[1] == 1.0                                                      # measured only


# ---- the norm, through the C ABI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_single_segment_edges(start):
    """Every head (0..3 elements in front of the first 16-byte boundary), tail and chunk edge; the surroundings are NaN, so an element
    read from outside [lo, hi) shows as a non-finite norm."""
    ch = _chunk()
    rng = np.random.default_rng(10 + start)
    for n in (1, 3, 4, 5, 255, 256, 257, ch - 1, ch, ch + 1, 2 * ch + 3):
        segs = [(start, start + n)]
        host = _nan_buffer(start + n + 3, segs, rng)
        call = GradNormCall(torch.from_numpy(host).cuda(), segs)()
        _assert_norms(call, host, segs)
        assert call.clip.tolist() == [0, 0], n


@pytest.mark.parametrize("values", ["normal", "1e30", "1e-30", "mixed"])
def test_segments_with_nan_gaps_and_extreme_magnitudes(values):
    """Six segments with gaps of 0..5 NaN elements; elements around 1, around 1e30 (an fp32 square is inf), around 1e-30 (an fp32 square
    is 0) and magnitudes 1e-20 .. 1e15 by segment: the same 1e-6 bound, total and per segment."""
    ch = _chunk()
    segs, end = layout([1, 1, 7, ch + 1, 3, 2 * ch], [0, 1, 2, 3, 4, 5])
    scales = dict(normal=[1.0] * 6, **{"1e30": [1e30] * 6, "1e-30": [1e-30] * 6}, mixed=[1e-20, 1e-13, 1e-6, 1.0, 1e8, 1e15])[values]
    host = _nan_buffer(end + 2, segs, np.random.default_rng(3), scales)
    call = GradNormCall(torch.from_numpy(host).cuda(), segs)()
    _assert_norms(call, host, segs)
    assert call.clip.tolist() == [0, 0]


def test_two_calls_are_bit_identical():
    """Contract (d): out, seg_sumsq, the item partials and, through the clipped Adam, the parameters."""
    ch = _chunk()
    segs, end = layout([5, 2 * ch + 3, ch, 300], [1, 0, 2, 3])
    host = _nan_buffer(end, segs, np.random.default_rng(4))
    buf = torch.from_numpy(np.nan_to_num(host, nan=0.0)).cuda()              # the gaps are zeros here: Adam runs over the whole buffer
    ref = norm64(buf.cpu().numpy())
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        p = (torch.randn(end) * 0.1).cuda()
        m, v, counters = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(2, dtype=torch.int32, device="cuda")
        call = GradNormCall(buf, segs)(max_norm=0.1 * ref)
        adam(p, buf, m, v, 1, counters=counters, norm_out=call.out)
        runs.append((call.out.clone(), call.seg_sumsq.clone(), call.partial.clone(), p, m, v))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][0][1]) < 1.0


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["first", "last", "chunk"])
def test_one_non_finite_element(bad, where):
    """Contract (e): the norm is non-finite, the scale exactly 1, clip[1] counts the call, and spair_adam_clipped leaves parameters and
    moments untouched to the bit without touching its counters.  The other segment's sum stays finite."""
    ch = _chunk()
    segs, end = layout([2 * ch + 3, 5], [1, 2])
    host = _nan_buffer(end + 1, segs, np.random.default_rng(6))
    lo, hi = segs[0]
    host[dict(first=lo, last=hi - 1, chunk=lo + ch)[where]] = bad
    buf = torch.from_numpy(host).cuda()
    call = GradNormCall(buf, segs)(max_norm=1.0)
    out, seg = call.out.cpu().numpy(), call.seg_sumsq.cpu().numpy()
    assert not np.isfinite(out[0]) and out[1] == 1.0
    assert not np.isfinite(seg[0]) and np.isfinite(seg[1])
    assert call.clip.tolist() == [0, 1]
    call(max_norm=1.0)
    assert call.clip.tolist() == [0, 2]
    torch.manual_seed(7)
    n = end + 1
    p, m, v = torch.randn(n).cuda(), torch.randn(n).cuda(), torch.rand(n).cuda()
    g = torch.randn(n).cuda()                                                # finite gradients: only the norm says "leave it out"
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    adam(p, g, m, v, 3, counters=counters, norm_out=call.out)
    assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and counters.tolist() == [0, 0]


# ---- the clipped Adam, through the C ABI ----------------------------------------------------------------------------------------------
def _adam_state(n, seed):
    torch.manual_seed(seed)
    p, g = (torch.randn(n) * 0.1).cuda(), torch.randn(n).cuda()
    m, v = (torch.randn(n) * 0.1).cuda(), (torch.rand(n) * 0.1).cuda()
    return p, g, m, v


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("n", [1000, "2*CH+3"])
def test_scale_one_equals_the_guarded_step_to_the_bit(n, step):
    """Contract (b): max_norm above the norm gives scale == 1.0f exactly, and then parameters and both moments are bit-identical to
    spair_adam_guarded's; with a skip word of 1 nothing moves and counters[0] goes up."""
    n = 2 * _chunk() + 3 if n == "2*CH+3" else n
    p, g, m, v = _adam_state(n, 8)
    call = GradNormCall(g, [(0, n)])(max_norm=1e30)
    assert call.out[1].item() == 1.0 and call.clip.tolist() == [0, 0]
    skip = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = []
    for norm_out in (None, call.out):
        q, mq, vq, counters = p.clone(), m.clone(), v.clone(), torch.zeros(2, dtype=torch.int32, device="cuda")
        adam(q, g, mq, vq, step, skip=skip, counters=counters, norm_out=norm_out)
        res.append((q, mq, vq, counters))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0], p) and res[1][3].tolist() == [0, 0]
    skip.fill_(1)
    q, mq, vq, counters = p.clone(), m.clone(), v.clone(), torch.zeros(2, dtype=torch.int32, device="cuda")
    adam(q, g, mq, vq, step, skip=skip, counters=counters, norm_out=call.out)
    assert torch.equal(q, p) and torch.equal(mq, m) and torch.equal(vq, v) and counters.tolist() == [1, 0]


@pytest.fixture(scope="module")
def torch_adam_states():
    """n = 1000 parameters ~ N(0, 0.1) taken through 0, 1 and 999 steps of CPU torch.optim.Adam(lr=1e-3) on N(0, 1) gradients: the
    shared states {steps done: (params, exp_avg, exp_avg_sq)} the clipped step starts from, and the gradient of that step."""
    gen = torch.Generator().manual_seed(11)
    p = torch.nn.Parameter(torch.randn(1000, generator=gen) * 0.1)
    opt = torch.optim.Adam([p], lr=1e-3)
    states = {0: (p.detach().clone(), torch.zeros(1000), torch.zeros(1000))}
    for done in range(1, 1000):
        p.grad = torch.randn(1000, generator=gen)
        opt.step()
        if done in (1, 999):
            st = opt.state[p]
            states[done] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return states, torch.randn(1000, generator=gen)


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_clipped_step_against_torch_clip_and_adam(torch_adam_states, step):
    """max_norm = 0.1 x the norm: one step from the shared state against CPU clip_grad_norm_ + torch.optim.Adam.step() on the same
    tensors, to the project's 2e-7 for fused-vs-torch Adam on identical gradients (the clip moves g by a couple of fp32 ulps, the update
    by about lr * 1e-6: far below the spacing of the parameters)."""
    states, g = torch_adam_states
    p0, m0, v0 = states[step - 1]
    ref_norm = norm64(g.numpy())
    max_norm = 0.1 * ref_norm
    # CPU torch
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=1e-3)
    if step > 1:
        opt.state[pt] = dict(step=torch.tensor(float(step - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    pt.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([pt], max_norm)
    opt.step()
    # the kernels
    p, m, v, gd = p0.cuda(), m0.cuda(), v0.cuda(), g.cuda()
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = GradNormCall(gd, [(0, 1000)])(max_norm=max_norm, norm_eps=1e-6)
    adam(p, gd, m, v, step, lr=1e-3, counters=counters, norm_out=call.out)
    out = call.out.cpu().numpy()
    want = min(1.0, max_norm / (ref_norm + 1e-6))
    assert abs(float(out[0]) - ref_norm) <= NORM_RTOL * ref_norm
    assert abs(float(out[1]) - want) <= 1e-6 * want and call.clip.tolist() == [1, 0]
    diff = (p.cpu() - pt.detach()).abs().max().item()
    print("step %d: max |dp| vs torch %.3e, scale %.9g (want %.9g)" % (step, diff, float(out[1]), want))
    assert diff <= 2e-7
    assert torch.equal(gd.cpu(), g) and counters.tolist() == [0, 0]          # the gradients are read, never written


# ---- on a model ---------------------------------------------------------------------------------------------------------------------
class _Trained:
    """The 48x48 bf16 model after one forward and backward on a 4-image batch; ``reset`` puts parameters and gradients back."""

    def __init__(self):
        from spair_pytorch_amd import config as cfg, models
        from spair_pytorch_amd.data import scattered_digits
        cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
        torch.manual_seed(3)
        self.model = models.SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
        x = torch.from_numpy(scattered_digits(7, 4, 48, 3, obj_px=(10, 20))[0]).cuda()
        torch.manual_seed(100)
        self.model.flat_gradients().zero_()
        self.model(x, 2000)[0].backward()
        torch.cuda.synchronize()
        self.params, self.grads = self.model.flat_parameters().clone(), self.model.flat_gradients().clone()
        self.host = self.grads.cpu().numpy()
        self.total = norm64(self.host)
        assert np.isfinite(self.total) and self.total > 1.0                  # (the tests' norm_eps = 1e-6 is below 1e-6 of it)

    def reset(self):
        self.model.flat_parameters().copy_(self.params)
        self.model.flat_gradients().copy_(self.grads)
        self.model._bind_grads()
        return self.model


@pytest.fixture(scope="module")
def trained():
    return _Trained()


def test_grad_norms_of_a_model(trained):
    from spair_pytorch_amd import _lib as L, ddp
    from spair_pytorch_amd.optim import grad_norms
    import ctypes
    m = trained.reset()
    r = grad_norms(m)
    order = sorted(m._slices, key=lambda k: m._slices[k][0])
    assert r.names == order and set(order) == set(dict(m.named_parameters()))
    assert r.total.dim() == 0 and r.total.dtype == torch.float32 and tuple(r.per_parameter.shape) == (len(order),)
    assert abs(r.total.item() - trained.total) <= NORM_RTOL * trained.total and trained.total > 0
    per = r.per_parameter.cpu().numpy()
    for i, key in enumerate(order):
        off, cnt, _ = m._slices[key]
        ref = norm64(trained.host[off:off + cnt])
        assert abs(float(per[i]) - ref) <= NORM_RTOL * ref, key
        if key.startswith("attn."):
            assert per[i] == 0.0                                             # the reference's dead attention block
    assert any(k.startswith("attn.") for k in order) and (per > 0).sum() > len(order) // 2
    lo, hi = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    L.check(L.lib().spair_grad_buckets(ctypes.byref(m._dims(1)), lo, hi), "spair_grad_buckets")
    assert tuple(r.buckets.shape) == (len(ddp.BUCKET_NAMES),) == (3,)
    for b in range(3):
        ref = norm64(trained.host[lo[b]:hi[b]])
        assert ref > 0 and abs(r.buckets[b].item() - ref) <= NORM_RTOL * ref, ddp.BUCKET_NAMES[b]
    d = r.as_dict()
    assert list(d) == order and d[order[0]] == float(per[0])
    assert torch.equal(m.flat_gradients(), trained.grads)                    # measured only
    assert torch.equal(grad_norms(m).per_parameter, r.per_parameter)


def test_fused_adam_with_a_huge_max_grad_norm_equals_the_plain_one(trained):
    from spair_pytorch_amd.optim import FusedAdam
    after = []
    for kw in (dict(), dict(max_grad_norm=1e30)):
        m = trained.reset()
        opt = FusedAdam(m, lr=1e-3, **kw)
        opt.step()
        after.append(m.flat_parameters().clone())
        assert opt.skipped() == (0, False)
    assert torch.equal(after[0], after[1]) and not torch.equal(after[0], trained.params)
    assert opt.clip_stats() == dict(steps_clipped=0, steps_nonfinite_norm=0, last_norm=opt.grad_norm.item(), last_scale=1.0)


def test_fused_adam_clipped_against_torch(trained):
    from spair_pytorch_amd.optim import FusedAdam, grad_norms
    m = trained.reset()
    total = grad_norms(m).total
    max_norm = 0.1 * trained.total
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=max_norm)
    assert opt.grad_norm is None and opt.clip_scale is None
    opt.step()
    assert torch.equal(m.flat_gradients(), trained.grads)                    # contract (f)
    assert torch.equal(opt.grad_norm, total) and opt.grad_norm.dim() == 0
    want = min(1.0, max_norm / (trained.total + 1e-6))
    assert abs(opt.clip_scale.item() - want) <= 1e-6 * want
    stats = opt.clip_stats()
    assert stats["steps_clipped"] == 1 and stats["steps_nonfinite_norm"] == 0 and stats["last_norm"] == total.item()
    assert opt.skipped() == (0, False)
    pt = torch.nn.Parameter(trained.params.cpu().clone())
    pt.grad = trained.grads.cpu().clone()
    torch.nn.utils.clip_grad_norm_([pt], max_norm)
    torch.optim.Adam([pt], lr=1e-3).step()
    diff = (m.flat_parameters().cpu() - pt.detach()).abs().max().item()
    print("model: max |dp| vs torch %.3e" % diff)
    assert diff <= 2e-7


def test_clip_grad_norm_on_a_model(trained):
    from spair_pytorch_amd.optim import clip_grad_norm_, grad_norms
    m = trained.reset()
    total = grad_norms(m).total
    got = clip_grad_norm_(m, 0.1 * trained.total)
    assert got.dim() == 0 and got.is_cuda and torch.equal(got, total)
    new = norm64(m.flat_gradients().cpu().numpy())
    print("clipped buffer: norm %.9g, wanted %.9g (relative %.2e)" % (new, 0.1 * trained.total, abs(new / (0.1 * trained.total) - 1)))
    assert abs(new - 0.1 * trained.total) <= 1e-5 * 0.1 * trained.total      # one fp32 rounding per element, eps and the fp32 scale
    off, cnt, _ = max(m._slices.values(), key=lambda v: v[1])                # the largest parameter
    # a non-finite norm: torch would turn every gradient into NaN; here the buffer stays as it is
    m = trained.reset()
    m.flat_gradients()[off + cnt // 2] = float("nan")
    before = m.flat_gradients().clone()
    got = clip_grad_norm_(m, 0.1 * trained.total)
    assert not torch.isfinite(got).item()
    assert torch.equal(m.flat_gradients().view(torch.int32), before.view(torch.int32))


def test_checkpoint_carries_max_grad_norm(trained, tmp_path):
    from spair_pytorch_amd import checkpoint as ck
    from spair_pytorch_amd.optim import FusedAdam
    m = trained.reset()
    o1 = FusedAdam(m, lr=1e-3, max_grad_norm=0.5 * trained.total, norm_eps=1e-5)
    path = os.path.join(tmp_path, "ck.pt")
    ck.save_checkpoint(path, m, o1, iteration=7)
    o2 = FusedAdam(m, lr=1e-3)
    assert ck.load_checkpoint(path, m, o2) == 7
    assert o2.max_grad_norm == 0.5 * trained.total and o2.norm_eps == 1e-5
    old = {k: v for k, v in o1.state_dict().items() if k not in ("max_grad_norm", "norm_eps")}     # a file from before clipping
    o3 = FusedAdam(m, lr=1e-3, max_grad_norm=9.0)
    o3.load_state_dict(old)
    assert o3.max_grad_norm == 9.0 and o3.norm_eps == 1e-6
    o4 = FusedAdam(m, lr=1e-3)
    o4.load_state_dict(old)
    assert o4.max_grad_norm is None
    trained.reset()
    o2.step()                                                                # the loaded optimizer clips: its tables are built on first use
    assert o2.clip_stats()["steps_clipped"] == 1


def test_clipped_step_in_a_captured_graph_reads_the_scale_on_the_device(trained):
    """torch.cuda.graph around opt.step() alone (a linear graph: two norm kernels, then Adam).  The scale is a device scalar, not frozen
    at capture: after doubling the gradient buffer in place a replay reports twice the norm and half the scale."""
    from spair_pytorch_amd.optim import FusedAdam
    m = trained.reset()
    max_norm = 0.1 * trained.total
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=max_norm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                                           # warm-up outside the capture (optimizer state, tables)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    g.replay()
    torch.cuda.synchronize()
    n1, s1 = opt.grad_norm.item(), opt.clip_scale.item()
    assert abs(n1 - trained.total) <= NORM_RTOL * trained.total
    m.flat_gradients().mul_(2.0)
    g.replay()
    torch.cuda.synchronize()
    n2, s2 = opt.grad_norm.item(), opt.clip_scale.item()
    assert abs(n2 - 2 * n1) <= 1e-6 * 2 * n1 and abs(s2 - 0.5 * s1) <= 1e-6 * s1
    assert opt.clip_stats()["steps_clipped"] == 3 and torch.isfinite(m.flat_parameters()).all()
