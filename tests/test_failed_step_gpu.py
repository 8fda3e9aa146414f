"""The failed-step guard's contract (optim.py, ddp.py; SpairStep.status in include/spair_hip.h), beyond the single plain step of
test_status_gpu.py:
  A. ``FusedAdam.step()`` leaves the step out whole if ANY grad-enabled forward since the previous ``step()`` flagged its loss (gradient
     accumulation), and counts it once;
  B. no ``no_grad`` forward, ``parse``, ``evaluate``, ``compose`` or ``generate`` changes the word ``step()`` reads;
  C. after ``ddp.allreduce_gradients(model)`` every rank takes the same decision and every rank is loud (tests/ddp_status_worker.py);
  D. the step stays capturable (a captured step skips and recovers by itself);
  E. ``copy.deepcopy`` / ``torch.save`` of a model work and give an independent model.
Everything runs the ``c1_b8_step1001`` fixture: a 8-image batch, a handful of steps per test.  The band-split time-out bit (1) is never
provoked on the device: it is simulated by writing the word."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import load_case
import golden_inputs as gi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "c1_b8_step1001"
NOISE = ("eps_box", "eps_attr", "eps_depth", "u_pres")
NAN, INF = float("nan"), float("inf")


def _build(dtype):
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.models import SPAIR
    z, case = load_case(CASE)
    cfg.set_grid(case["I"], case["strides"])
    m = SPAIR([1, case["I"], case["I"]], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gi.make_weights(case["wseed"], case["wscale"]).items()})
    x = torch.from_numpy(z["x"]).cuda()
    noise = {k: torch.from_numpy(z[k]).cuda() for k in NOISE}
    return m, x, noise


_CACHE = {}


def _fresh(dtype, max_grad_norm=None):
    """One model per dtype for the whole module (built once), put back before each use: the fixture's weights after ONE finite Adam step
    (so the moments are not zero), those moments, clean status words.  Returns (model, a new FusedAdam on that state, x, noise, state)."""
    from spair_pytorch_amd.optim import FusedAdam
    if dtype not in _CACHE:
        m, x, noise = _build(dtype)
        opt = FusedAdam(m, lr=1e-3)
        _train_step(m, opt, x, noise, 1001)
        assert m.step_status() == 0 and opt.skipped() == (0, False)
        _CACHE[dtype] = (m, x, noise, dict(p=m.flat_parameters().clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone()))
    m, x, noise, st = _CACHE[dtype]
    m.raise_on_nonfinite = True
    with torch.no_grad():
        m.flat_parameters().copy_(st["p"])
    m.clear_step_status()
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=max_grad_norm)
    opt.load_state_dict(dict(step=1, exp_avg=st["m"], exp_avg_sq=st["v"]))
    return m, opt, x, {k: v.clone() for k, v in noise.items()}, st


def _train_step(m, opt, x, noise, gs, between=None):
    opt.zero_grad()
    loss = m(x, gs, noise=noise)[0]
    loss.backward()
    if between is not None:
        between()
    opt.step()
    return loss


def _state(m, opt):
    return m.flat_parameters().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()


def _same(a, b):
    """Bit-equal, a NaN the test itself planted in a parameter counting as equal to itself."""
    return all(torch.equal(torch.nan_to_num(s, nan=7.0, posinf=8.0, neginf=9.0), torch.nan_to_num(t, nan=7.0, posinf=8.0, neginf=9.0))
               for s, t in zip(a, b))


def _step_word(m):
    return int(m._status_dev[1].item())


# ---- 1. every loss term flags ------------------------------------------------------------------------------------------------------------
# The routes into loss_out[1..8], read off csrc/cell_math.h, csrc/cells.hip and csrc/loss.hip.  (kind, name, index, term, alone):
#   * KL cy / cx / height / width: the box head's MEAN enters its KL unclamped (box_forward: mu = lat[k]) while the sampled latent goes
#     through clamp10 (fminf(fmaxf(x, -10), 10): NaN -> -10) before anything else reads it -- the box, the glimpse and everything behind
#     them stay finite, so the term is non-finite ALONE.  The log-std half is clamped first: it cannot make a term non-finite.
#   * KL depth: the same, through the z network's mean (depth_forward).
#   * KL attr: the encoder's mean is the attribute latent itself (attr_forward: attr = mean + sd * eps), which the decoder, the z network,
#     the presence network and the later cells' context read: it cannot be made non-finite alone by construction (the log-std half is
#     clamped: no route).  The test holds that its term flags and says what else is certain.
#   * presence KL: the presence logit is clamped and the count prior is a host scalar, so only the uniform noise reaches it: z_pres is then
#     NaN, and z_pres weights every Gaussian KL (k_gauss_kl): the seven KL terms go together.
#   * BCE: the decoder's output bias reaches the sprites only, and those the renderer only: NaN there is BCE alone.  +-inf is a saturated
#     sigmoid (a sprite pixel of exactly 0 or 1): see test_decoder_bias_inf_saturates.
BOX, ZNET, ENC, DEC = "box_network.output_layers.0.bias", "z_network.output_layers.0.bias", "object_encoder.out.bias", "object_decoder.out.bias"
ROUTES = {
    "bce": ("param", DEC, 5, 1, True),
    "kl_cy": ("param", BOX, 0, 2, True),
    "kl_cx": ("param", BOX, 1, 3, True),
    "kl_height": ("param", BOX, 2, 4, True),
    "kl_width": ("param", BOX, 3, 5, True),
    "kl_attr": ("param", ENC, 3, 6, False),
    "kl_depth": ("param", ZNET, 0, 7, True),
    "kl_pres": ("noise", "u_pres", (1, 0, 2, 3), 8, False),
}
_CASES = [(r, v) for r in ROUTES for v in (NAN, INF, -INF) if not (r == "bce" and v != NAN)]


def _poison(m, noise, x, kind, name, index, value):
    if kind == "param":
        with torch.no_grad():
            dict(m.named_parameters())[name][index] = value
    elif kind == "noise":
        noise[name][index] = value
    else:
        x = x.clone()
        x[index] = value
    return x


def _assert_failed_step(m, opt, x, noise, before):
    """One whole step on poisoned inputs: flagged on the device (bit 2, in the step word before ``step()`` reads it and in the sticky word),
    in the host word, and left out whole.  Returns the loss terms."""
    seen = {}
    loss = _train_step(m, opt, x, noise, 1002, between=lambda: seen.update(word=m._status_dev.clone()))
    terms = m.loss_terms().clone()
    print(terms.cpu().numpy(), seen["word"].tolist(), opt.skipped())
    assert not np.isfinite(loss.item())
    assert int(seen["word"][1]) & 2 and int(seen["word"][0]) & 2
    assert m.step_status() & 2 and m._status_host[0] & 2
    assert opt.skipped()[0] == 1
    assert _same(_state(m, opt)[1:], before[1:])
    return terms


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("route,value", _CASES, ids=["%s[%s]" % c for c in _CASES])
def test_each_loss_term_flags(route, value, dtype):
    kind, name, index, term, alone = ROUTES[route]
    m, opt, x, noise, st = _fresh(dtype)
    x = _poison(m, noise, x, kind, name, index, value)
    before = _state(m, opt)                                    # with the poison in place
    terms = _assert_failed_step(m, opt, x, noise, before).cpu().numpy()
    assert _same(_state(m, opt)[:1], before[:1])
    assert not np.isfinite(terms[term]) and not np.isfinite(terms[0])
    others = [k for k in range(1, 9) if k != term]
    if alone:
        assert np.isfinite(terms[others]).all(), terms
    elif route == "kl_attr":
        # not alone: the attribute latent feeds every later network.  How far it gets depends on the value and the kernels on the way (a
        # ReLU written as fmaxf(x, 0) turns NaN into 0, +-inf goes through), so only what does not is held: the presence logit is
        # clamped (clamp10(NaN) = -10), the presence KL stays finite
        assert np.isfinite(terms[8]), terms
    else:
        assert not np.isfinite(terms[2:9]).any(), terms                                 # z_pres weights every Gaussian KL (k_gauss_kl)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_nan_pixel_flags(dtype):
    """A NaN pixel is the BCE's target and the backbone's input: every term goes."""
    m, opt, x, noise, st = _fresh(dtype)
    x = _poison(m, noise, x, "x", None, (2, 0, 17, 9), NAN)
    before = _state(m, opt)
    terms = _assert_failed_step(m, opt, x, noise, before).cpu().numpy()
    assert _same(_state(m, opt), before)
    assert not np.isfinite(terms[1]) and not np.isfinite(terms[0]), terms


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("value", [INF, -INF])
def test_decoder_bias_inf_saturates(value, dtype):
    """The BCE route with +-inf: an infinite decoder output bias is a saturated sigmoid, a sprite pixel (or its alpha) of exactly 1 or 0 --
    a finite image and, with the reference's clamp of the BCE's logs at -100, a finite loss.  Nothing is flagged; what the guard has
    to hold is the other half: the bias's own gradient and moments stay finite, and the infinite parameter stays what it was."""
    m, opt, x, noise, st = _fresh(dtype)
    _poison(m, noise, x, "param", DEC, 5, value)
    loss = _train_step(m, opt, x, noise, 1002)
    print(value, dtype, m.loss_terms().cpu().numpy(), m.step_status(), opt.skipped())
    assert np.isfinite(m.loss_terms().cpu().numpy()).all() and np.isfinite(loss.item())
    assert m.step_status() == 0 and m._status_host[0] == 0 and opt.skipped()[0] == 0
    assert torch.isfinite(opt.exp_avg).all() and torch.isfinite(opt.exp_avg_sq).all()
    assert int((~torch.isfinite(m.flat_parameters())).sum()) == 1


# ---- 2. no_grad calls between backward and step (contract B) -------------------------------------------------------------------------
def _flagging_noise(noise):
    bad = {k: v.clone() for k, v in noise.items()}
    bad["u_pres"][1, 0, 2, 3] = NAN
    return bad


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
@pytest.mark.parametrize("refuse", [True, False])
def test_no_grad_calls_between_backward_and_step_leave_the_step_word(refuse, max_grad_norm):
    """A flagged training forward and its backward, then every other kind of forward, then ``step()``.  With ``raise_on_nonfinite`` (the
    default) ``forward``, ``parse`` and ``evaluate`` refuse to run once the host word is set -- asserted as the refusal -- while ``compose``
    and ``generate`` (no loss, no status) run; with it off all five run, finite.  Either way the step is left out and counted once."""
    from spair_pytorch_amd._lib import SpairHipError
    m, opt, x, noise, st = _fresh("bf16", max_grad_norm)
    before = _state(m, opt)
    m.raise_on_nonfinite = refuse
    opt.zero_grad()
    loss = m(x, 1002, noise=_flagging_noise(noise))[0]
    loss.backward()
    torch.cuda.synchronize()
    assert _step_word(m) == 2 and m._status_host[0] == 2
    with torch.no_grad():
        calls = dict(forward=lambda: m(x, 1002, noise=noise)[0], parse=lambda: m.parse(x, 1002).loss_terms[0],
                     evaluate=lambda: m.evaluate(x, 1002, noise=noise).loss.sum())
        for name, call in calls.items():
            if refuse:
                with pytest.raises(SpairHipError, match="non-finite"):
                    call()
            else:
                assert np.isfinite(call().item()), name
            assert _step_word(m) == 2, name
        g = m.generate(4, 1002, count=2, seed=1)
        assert _step_word(m) == 2
        assert torch.isfinite(m.compose(g).recon).all() and _step_word(m) == 2
    opt.step()
    assert opt.skipped()[0] == 1 and _same(_state(m, opt), before)
    assert m.step_status() == 2


# ---- 3. gradient accumulation (contract A) -----------------------------------------------------------------------------------------
def _micro(x, noise, lo, hi):
    return x[lo:hi].contiguous(), {k: v[lo:hi].contiguous() for k, v in noise.items()}


def _accumulated_step(m, opt, batches):
    opt.zero_grad()
    for xb, nb in batches:
        m(xb, 1002, noise=nb)[0].backward()
    opt.step()


@pytest.mark.parametrize("flagged", [0, 1])
def test_accumulation_one_flagged_micro_batch_leaves_the_step_out(flagged):
    m, opt, x, noise, st = _fresh("bf16")
    m.raise_on_nonfinite = False            # the second micro-batch's forward is not to depend on when the first one's host word lands
    before = _state(m, opt)
    batches = [_micro(x, noise, 0, 4), _micro(x, noise, 4, 8)]
    batches[flagged] = (batches[flagged][0], _flagging_noise(batches[flagged][1]))
    _accumulated_step(m, opt, batches)
    assert opt.skipped()[0] == 1 and _same(_state(m, opt), before)
    assert m.step_status() == 2 and m._status_host[0] == 2
    assert _step_word(m) == 0               # read and cleared by the step: the next one starts clean
    m.raise_on_nonfinite = True
    m.clear_step_status()
    _accumulated_step(m, opt, [_micro(x, noise, 0, 4), _micro(x, noise, 4, 8)])
    assert opt.skipped()[0] == 1 and not torch.equal(m.flat_parameters(), before[0])


def test_accumulation_of_finite_micro_batches_is_the_plain_step():
    """Two finite micro-batches: the step is applied, and it is to the bit the step a second model, newly built and brought to the same
    state, takes over the same two micro-batches: the word the forwards OR into and the fill that clears it change nothing else."""
    from spair_pytorch_amd.optim import FusedAdam
    m, opt, x, noise, st = _fresh("bf16")
    batches = [_micro(x, noise, 0, 4), _micro(x, noise, 4, 8)]
    _accumulated_step(m, opt, batches)
    assert opt.skipped() == (0, False) and m.step_status() == 0 and _step_word(m) == 0
    got = _state(m, opt)
    assert not torch.equal(got[0], st["p"]) and torch.isfinite(got[0]).all()
    m2, _, _ = _build("bf16")
    with torch.no_grad():
        m2.flat_parameters().copy_(st["p"])
    opt2 = FusedAdam(m2, lr=1e-3)
    opt2.load_state_dict(dict(step=1, exp_avg=st["m"], exp_avg_sq=st["v"]))
    _accumulated_step(m2, opt2, batches)
    assert torch.equal(m2.flat_gradients(), m.flat_gradients())
    assert _same(_state(m2, opt2), got)


# ---- 4. a flag with finite gradients -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_flag_with_finite_gradients_leaves_the_step_out(max_grad_norm):
    """The band-split time-out bit, simulated: the step's word set to 1 by hand behind a finite forward and backward.  Every gradient is
    finite, so only the whole-step skip stands between this step and the parameters."""
    m, opt, x, noise, st = _fresh("bf16", max_grad_norm)
    before = _state(m, opt)

    def flag():
        assert torch.isfinite(m.flat_gradients()).all()
        m._status_dev[1] = 1

    assert np.isfinite(_train_step(m, opt, x, noise, 1002, between=flag).item())
    assert opt.skipped() == (1, False) and _same(_state(m, opt), before)
    if max_grad_norm is not None:
        assert opt.clip_stats()["steps_nonfinite_norm"] == 0
    m.clear_step_status()
    assert np.isfinite(_train_step(m, opt, x, noise, 1003).item())
    assert opt.skipped() == (1, False) and m.step_status() == 0
    after = _state(m, opt)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1]) and not torch.equal(after[2], before[2])


# ---- 5. two ranks (contract C) -----------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# as tests/test_ddp_gpu.py selects them: gloo with both ranks on one GPU always, RCCL where there are two GPUs
_MODES = [("gloo", "1"), ("gloo", "0")] + ([("nccl", "1"), ("nccl", "0")] if torch.cuda.device_count() >= 2 else [])


@pytest.mark.parametrize("backend,overlap", _MODES)
@pytest.mark.parametrize("variant", ["hand", "natural"])
def test_two_ranks_take_the_same_skip_decision(tmp_path, variant, backend, overlap):
    """Step 1 finite on both ranks; in step 2 rank 1 ALONE is flagged while gradients that reach rank 0 stay finite (``hand``: its step
    word set to 1 behind the backward, every gradient finite; ``natural``: a NaN in rank 1's box-head mean bias for that forward only --
    the cy KL alone is NaN, the decoder bucket's gradients stay finite, which the worker asserts); step 3 finite after
    ``clear_step_status()``.  The worker catches SpairHipError and every rank reaches every collective and the final barrier whatever
    the outcome, so a rank-local decision shows as a failed assertion here, not as a hang."""
    prefix = str(tmp_path / "rank")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SPAIR_DIST_BACKEND=backend,
                   SPAIR_DDP_OVERLAP=overlap, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ddp_status_worker.py"), prefix, "bf16", variant], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(logs)
    r = [np.load("%s%d.npz" % (prefix, rank)) for rank in range(2)]
    keys = [k + s for s in "123" for k in "pmv"]
    for k in keys:                                              # parameters and both moments, after each step: the replicas are one model
        assert np.array_equal(r[0][k], r[1][k], equal_nan=True), k
    assert not np.array_equal(r[0]["p1"], r[0]["p0"])
    for k in "pmv":                                             # step 2 was left out whole, on both
        assert np.array_equal(r[0][k + "2"], r[0][k + "1"]) and np.array_equal(r[1][k + "2"], r[1][k + "1"]), k
        assert not np.array_equal(r[0][k + "3"], r[0][k + "2"]), k         # step 3 applied
    for rank in range(2):
        assert r[rank]["skipped"].tolist() == [0, 1, 1], rank
        assert bool(r[rank]["raised_check"]) and bool(r[rank]["raised_forward"]), rank
        assert int(r[rank]["status3"]) == 0
    assert "another rank" in str(r[0]["message"]) and "another rank" not in str(r[1]["message"])
    if variant == "natural":
        assert "non-finite" in str(r[0]["message"]) and "non-finite" in str(r[1]["message"])
    else:
        assert "timed out" in str(r[0]["message"]) and "timed out" in str(r[1]["message"])


# ---- 6. the captured step ----------------------------------------------------------------------------------------------------------
def test_captured_step_skips_and_recovers():
    """zero_grad + forward + backward + ``step()`` captured as test_whole_step_is_capturable_in_a_hip_graph captures them (warm-up on a side
    stream, spair_init ahead).  A replay with a NaN in the static input leaves the step out by itself -- the flag travels through device
    memory, and the step's fill that clears the word is a node of the graph -- and a replay after the input is restored and the status
    cleared applies it.  ``raise_on_nonfinite`` inside a capture: forward's look at the host word is host code, it ran once, at capture
    time, and a replay runs no host code -- a replay never raises.  The failure is loud where the host looks again:
    ``check_step_status()``, ``step_status()``, the host word, and the next EAGER forward."""
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd._lib import SpairHipError
    m, opt, x, noise, st = _fresh("bf16")
    L.check(L.lib().spair_init(), "spair_init")
    xs = x.clone()

    def step():
        opt.zero_grad()
        loss = m(xs, 1002, noise=noise)[0]
        loss.backward()
        opt.step()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = step()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and opt.skipped() == (0, False) and m.step_status() == 0
    before = _state(m, opt)
    xs[2, 0, 17, 9] = NAN
    g.replay()
    torch.cuda.synchronize()
    assert not np.isfinite(float(loss))
    assert opt.skipped()[0] == 1 and _same(_state(m, opt), before)
    assert m._status_host[0] & 2 and _step_word(m) == 0
    with pytest.raises(SpairHipError, match="non-finite"):
        m.check_step_status()
    with pytest.raises(SpairHipError, match="non-finite"):
        m(x, 1003, noise=noise)
    xs.copy_(x)
    m.clear_step_status()
    g.replay()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and opt.skipped()[0] == 1 and m.step_status() == 0
    after = _state(m, opt)
    assert torch.isfinite(after[0]).all() and not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])


# ---- 7. copies (contract E) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["deepcopy", "save"])
@pytest.mark.parametrize("when", ["before_forward", "after_forward"])
def test_copies_are_independent_models(tmp_path, when, how):
    import ctypes
    from spair_pytorch_amd._lib import SpairHipError
    from spair_pytorch_amd.optim import FusedAdam
    m, x, noise = _build("bf16")
    if when == "after_forward":
        _train_step(m, FusedAdam(m, lr=1e-3), x, noise, 1001)
    if how == "deepcopy":
        c = copy.deepcopy(m)
    else:
        path = str(tmp_path / "model.pt")
        torch.save(m, path)
        c = torch.load(path, weights_only=False)
    with torch.no_grad():
        want = m(x, 1002, noise=noise)
        got = c(x, 1002, noise=noise)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert torch.equal(c.flat_parameters(), m.flat_parameters())
    # its own buffers, status words and engines
    addr = lambda mod: ctypes.cast(mod._status_host, ctypes.c_void_p).value
    assert c.flat_parameters().data_ptr() != m.flat_parameters().data_ptr()
    assert c.flat_gradients().data_ptr() != m.flat_gradients().data_ptr()
    assert c._status_dev.data_ptr() != m._status_dev.data_ptr() and addr(c) != addr(m)
    assert c._engines is not m._engines
    assert c._engines[8]["workspace"].data_ptr() != m._engines[8]["workspace"].data_ptr()
    # a failed step on the copy: the copy is loud, the original is not, and trains on
    copt = FusedAdam(c, lr=1e-3)
    _train_step(c, copt, x, _flagging_noise(noise), 1002)
    assert copt.skipped()[0] == 1
    with pytest.raises(SpairHipError, match="non-finite"):
        c.check_step_status()
    with pytest.raises(SpairHipError, match="non-finite"):
        c(x, 1003, noise=noise)
    m.check_step_status()
    assert m._status_host[0] == 0
    p0 = m.flat_parameters().clone()
    opt = FusedAdam(m, lr=1e-3)
    assert np.isfinite(_train_step(m, opt, x, noise, 1002).item()) and opt.skipped() == (0, False)
    assert not torch.equal(m.flat_parameters(), p0) and torch.equal(c.flat_parameters(), p0)
