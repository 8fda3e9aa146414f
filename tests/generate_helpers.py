"""Shared by test_generate_cpu.py / test_generate_gpu.py: SPAIR.generate's definition restated in float64 on the CPU (numpy).

Presence (include/spair_hip.h, "scene generation"; reference models.py:184-257): cells in row-major order, cd the distribution of the
object count c = 0 .. HW, `seen` the objects so far, rem = HW - i:
    q_c = clamp(c - seen, 0, rem) / rem,  p_z(i) = sum_c cd_c q_c,  z_i = [u_i < p_z(i)],
    cd <- cd (z_i q + (1 - z_i)(1 - q)) / max(its sum, 1e-6),  seen += z_i,
started from normalise((1 - p) p^c) (the geometric prior) or from the one-hot distribution at n (``count``).  ``presence_float64`` runs it
in ABSOLUTE bins, as the reference does, free-running (it takes its own decisions from ``u``) or teacher-forced (it is given ``z`` and
returns the p_z of every cell on that history).

Gaussian maps: raw = m + s eps with the priors (cy, cx, height, width, attr, depth), then the forward's transforms with
oracle.spair_oracle.clamped_sigmoid; ``gauss_bounds`` is the fp32 bound of those formulas from their operand magnitudes."""
import numpy as np
import torch

from oracle import spair_oracle as orc

MARGIN = 5e-5            # the p_z bound tests/test_countkl_gpu.py holds k_count_kl to; a decision is checked where |u - p_z64| exceeds it
MARGIN_SHARE = 0.005     # at most this share of a case's cells may fall inside the margin (expected: 2 * MARGIN = 1e-4)


def geometric_start(prob, HW):
    """normalise((1 - p) p^c), c = 0 .. HW, float64 (p: the fp32 value the kernel is given, widened)."""
    p = float(np.float32(prob))
    cd = (1.0 - p) * p ** np.arange(HW + 1, dtype=np.float64)
    return cd / cd.sum()


def presence_float64(HW, B, prob=None, count=None, u=None, z=None):
    """(z [B,HW], p_z [B,HW], n [B]) in float64.  ``count`` (None, an int or [B] ints; clamped to [0, HW]): one-hot start, else the
    geometric start of ``prob``.  ``z`` given: teacher-forced (``u`` is not read); else free-running on ``u`` [B,HW]."""
    c = np.arange(HW + 1, dtype=np.float64)[None, :]
    if count is None:
        cd = np.repeat(geometric_start(prob, HW)[None, :], B, axis=0)
    else:
        n = np.clip(np.broadcast_to(np.asarray(count, np.int64), (B,)), 0, HW)
        cd = (c == n[:, None]).astype(np.float64)
    seen = np.zeros((B, 1))
    zs, pzs = np.zeros((B, HW)), np.zeros((B, HW))
    forced = None if z is None else np.asarray(z, np.float64).reshape(B, HW)
    uu = None if u is None else np.asarray(u, np.float64).reshape(B, HW)
    for i in range(HW):
        rem = float(HW - i)
        q = np.clip(c - seen, 0.0, rem) / rem
        pz = (cd * q).sum(axis=1, keepdims=True)
        zi = forced[:, i:i + 1] if forced is not None else (uu[:, i:i + 1] < pz).astype(np.float64)
        cd = cd * (zi * q + (1 - zi) * (1 - q))
        cd = cd / np.maximum(cd.sum(axis=1, keepdims=True), 1e-6)
        seen = seen + zi
        zs[:, i], pzs[:, i] = zi[:, 0], pz[:, 0]
    return zs, pzs, seen[:, 0].astype(np.int64)


def onehot_reference_literal(HW, n, u):
    """models.py:206-241 run literally in float64 from a one-hot count distribution (torch, one sample): the clamp on the support, the
    normaliser's 1e-6 clamp and torch.round, with the cell's own draw z = [u < p_z] in place of the posterior sample."""
    support = torch.arange(HW + 1, dtype=torch.float64)
    cd = (support == float(n)).double()[None, :]
    count = torch.zeros(1, 1, dtype=torch.float64)
    zs, pzs = [], []
    for i in range(HW):
        q = torch.clamp(support - count, min=0.0, max=float(HW - i)) / (HW - i)
        p_z = (cd * q).sum(1, keepdim=True)
        pr = (torch.tensor([[float(u[i])]], dtype=torch.float64) < p_z).double()
        s = torch.round(pr)
        cd1 = (s * q + (1 - s) * (1 - q)) * cd
        cd = cd1 / cd1.sum(1, keepdim=True).clamp(min=1e-6)
        count = count + s
        zs.append(float(s)), pzs.append(float(p_z))
    return np.array(zs), np.array(pzs)


def exact_count_fp32(HW, count, u):
    """The closed form the kernel runs for ``count``: need = n - seen, p_z = fl32(need / rem), z = [u < p_z], all fp32 -> (z, p_z, n)."""
    u = np.asarray(u, np.float32)
    B = u.shape[0]
    n = np.clip(np.broadcast_to(np.asarray(count, np.int64), (B,)), 0, HW)
    z, pz = np.zeros((B, HW), np.float32), np.zeros((B, HW), np.float32)
    for b in range(B):
        need = int(n[b])
        for i in range(HW):
            p = np.float32(need) / np.float32(HW - i)
            on = bool(u[b, i] < p)
            z[b, i], pz[b, i] = on, p
            need -= on
    return z, pz, z.sum(axis=1).astype(np.int64)


def dense_patterns(kind, B, HW, seed=11):
    """bool [B,HW], the pattern family of tests/test_countkl_gpu.py (test_count_kl_dense_presence): an otherwise full grid with ONE absent
    cell at a different position per sample, i.i.d. presence at 0.6 / 0.8 / 0.9 / 0.97, runs of 4-19 present cells behind 1-8 absent."""
    rng = np.random.default_rng(seed)
    on = np.ones((B, HW), bool)
    if kind == "one_off":
        for b in range(B):
            on[b, (b * HW) // B] = False
    elif kind == "iid":
        dens = (0.6, 0.8, 0.9, 0.97)
        for b in range(B):
            on[b] = rng.uniform(size=HW) < dens[b % 4]
    elif kind == "runs":
        for b in range(B):
            i = int(rng.integers(0, 6))
            on[b, :i] = False
            while i < HW:
                i += int(rng.integers(4, 20))
                gap = int(rng.integers(1, 9))
                on[b, i:i + gap] = False
                i += gap
    else:
        raise ValueError(kind)
    return on


ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))     # 1 - 2^-24, the largest u


def uniform_u(seed, B, HW):
    """u in [0, 1) as fp32 (a draw that rounds to 1.0 is moved to the largest float below it)."""
    u = np.random.default_rng(seed).uniform(size=(B, HW)).astype(np.float32)
    return np.minimum(u, ONE_BELOW)


def check_presence_rule(u, z, pz, n, pz64, tag=""):
    """The teacher-forced rule on a kernel result (numpy arrays; pz64 = presence_float64(..., z=z)[1]).  Returns (largest |p_z - p_z64|,
    share of cells inside the margin) after asserting the rule."""
    u, z, pz = np.asarray(u, np.float64), np.asarray(z, np.float64), np.asarray(pz, np.float64)
    assert np.isfinite(pz).all() and pz.min() >= 0 and pz.max() <= 1, (tag, pz.min(), pz.max())
    assert np.isin(z, (0.0, 1.0)).all(), tag
    err = np.abs(pz - pz64).max()
    decided = np.abs(u - pz64) > MARGIN
    share = 1.0 - decided.mean()
    print("%s: largest |p_z - p_z64| %.3g, share of cells inside the margin %.3g" % (tag, err, share))
    assert err <= MARGIN, (tag, err)
    assert np.array_equal(z[decided], (u < pz64)[decided].astype(np.float64)), tag
    assert share <= MARGIN_SHARE, (tag, share)
    assert np.array_equal(np.asarray(n, np.int64), z.sum(axis=1).astype(np.int64)), tag
    return err, share


# ---- the Gaussian maps ------------------------------------------------------------------------------------------------------------------
def gauss_float64(eps_box, eps_attr, eps_depth, priors, hyper):
    """eps maps (numpy, NCHW) -> (z_where [B,4,G,Gw], z_what, z_depth) in float64.  ``priors``: six (mean, std) in the order cy, cx,
    height, width, attr, depth (fp32 values, widened); ``hyper``: dict(min_yx, max_yx, min_hw, max_hw, anchor, cell_px, I, Iw)."""
    eb, ea, ed = (torch.from_numpy(np.asarray(v, np.float64)) for v in (eps_box, eps_attr, eps_depth))
    pm = [float(np.float32(m)) for m, _ in priors]
    ps = [float(np.float32(s)) for _, s in priors]
    h = {k: float(np.float32(v)) if isinstance(v, float) else v for k, v in hyper.items()}
    B, _, G, Gw = eb.shape
    raw = [pm[k] + ps[k] * eb[:, k] for k in range(4)]
    sig = [orc.clamped_sigmoid(r) for r in raw]
    cell_y = (h["max_yx"] - h["min_yx"]) * sig[0] + h["min_yx"]
    cell_x = (h["max_yx"] - h["min_yx"]) * sig[1] + h["min_yx"]
    height = (h["max_hw"] - h["min_hw"]) * sig[2] + h["min_hw"]
    width = (h["max_hw"] - h["min_hw"]) * sig[3] + h["min_hw"]
    hh = torch.arange(G, dtype=torch.float64)[None, :, None]
    ww = torch.arange(Gw, dtype=torch.float64)[None, None, :]
    xt = h["cell_px"] / h["Iw"] * (cell_x + ww)
    yt = h["cell_px"] / h["I"] * (cell_y + hh)
    xs = width * h["anchor"] / h["Iw"]
    ys = height * h["anchor"] / h["I"]
    z_where = torch.stack((xt, yt, xs, ys), 1)
    z_what = pm[4] + ps[4] * ea
    z_depth = 4 * orc.clamped_sigmoid(pm[5] + ps[5] * ed)
    return z_where.numpy(), z_what.numpy(), z_depth.numpy()


def gauss_bounds(eps_box, eps_attr, eps_depth, priors, hyper):
    """fp32 against float64 on the same eps, from the operand magnitudes (e = 2^-24, one rounding to nearest):
      raw = m + s eps: one product and one sum (or one fused step), |d raw| <= 2 e (|m| + |s eps|);
      sigmoid(clamp10(raw)) = 1 / (1 + exp(-raw)): the sigmoid is 1/4-Lipschitz, and on its own operand exp (<= 2 ulp), the sum and the
        division (<= 1 ulp each) move it by <= 8 e relative to a value <= 1: |d sig| <= |d raw| / 4 + 8 e;
      range * sig + min: |d| <= range |d sig| + 3 e (range + |min|)   (the range is itself one fp32 difference);
      xt = cell_px / Iw (cell_x + w): the factor is rounded once, one sum, one product: |d xt| <= factor |d cell_x| + 3 e |xt|;
      xs = width anchor / Iw: one product, one division: |d xs| <= anchor / Iw |d width| + 3 e |xs|;
      z_depth = 4 sig: exact scaling, 4 |d sig|;   z_what = raw.
    Returns (E_where [B,4,G,Gw], E_what, E_depth)."""
    e = 2.0 ** -24
    eb, ea, ed = (np.abs(np.asarray(v, np.float64)) for v in (eps_box, eps_attr, eps_depth))
    pm = [abs(float(m)) for m, _ in priors]
    ps = [abs(float(s)) for _, s in priors]
    h = hyper
    d_raw = [2 * e * (pm[k] + ps[k] * eb[:, k]) for k in range(4)]
    d_sig = [d / 4 + 8 * e for d in d_raw]
    ryx, rhw = h["max_yx"] - h["min_yx"], h["max_hw"] - h["min_hw"]
    d_yx = [ryx * d_sig[k] + 3 * e * (abs(ryx) + abs(h["min_yx"])) for k in (0, 1)]          # cell_y, cell_x
    d_hw = [rhw * d_sig[k] + 3 * e * (abs(rhw) + abs(h["min_hw"])) for k in (2, 3)]          # height, width
    G, Gw = eb.shape[2], eb.shape[3]
    fx, fy = h["cell_px"] / h["Iw"], h["cell_px"] / h["I"]
    xt_max = fx * (max(abs(h["max_yx"]), abs(h["min_yx"])) + Gw)
    yt_max = fy * (max(abs(h["max_yx"]), abs(h["min_yx"])) + G)
    xs_max, ys_max = h["max_hw"] * h["anchor"] / h["Iw"], h["max_hw"] * h["anchor"] / h["I"]
    E_where = np.stack((fx * d_yx[1] + 3 * e * xt_max, fy * d_yx[0] + 3 * e * yt_max,
                        h["anchor"] / h["Iw"] * d_hw[1] + 3 * e * xs_max, h["anchor"] / h["I"] * d_hw[0] + 3 * e * ys_max), 1)
    E_what = 2 * e * (pm[4] + ps[4] * ea)
    E_depth = 4 * ((2 * e * (pm[5] + ps[5] * ed[:, 0])) / 4 + 8 * e)[:, None]
    return E_where, E_what, E_depth


# ---- the sampler's unit-level cases (test_generate_gpu.py runs them; test_generate_cpu.py checks their margin share on the reference) ----
SAMPLER_HW = (1, 2, 63, 64, 65, 127, 128, 129, 1024)      # HW + 1 bins against multiples of 64, and the limit
SAMPLER_B = (1, 5, 8)                                     # an odd batch, and waves per workgroup +- 1: the tail workgroup
SAMPLER_P = (0.0123, 0.5, 0.999999)                       # late in the schedule, the middle, the step-0 value (the dense regime)


def sampler_seed(HW, B, p):
    return 1000 * HW + 10 * B + SAMPLER_P.index(p)
