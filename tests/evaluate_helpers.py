"""Shared by test_evaluate_cpu.py / test_evaluate_gpu.py: SPAIR.evaluate's definition restated in float64 (numpy), the fp32 bound of that
definition from its operands' magnitudes, the made-up operands of the unit-level cases and the fixtures the model is held to.

Definition (include/spair_hip.h, "evaluation"; reference models.py:169-262, 544-563), cells in row-major order k = h * Gw + w:
    kl_map[b, j, k], j = 0 .. 5 (cy, cx, height, width, attr, depth) = z 0.5 (vr + t1 - 1 - log vr), vr = (sd / s)^2, t1 = ((mu - m) / s)^2,
        attr summed over its A elements;
    kl_map[b, 6, k] = z (log(z + 1e-9) - log(p_z + 1e-9)) + (1 - z)(log(1 - z + 1e-9) - log(1 - p_z + 1e-9)) on the GIVEN p_z;
    bce_map[b, y, x] = sum_c -(x max(log r, -100) + (1 - x) max(log(1 - r), -100));
    terms[b] = (bce_b + beta sum_j kl_b,j, bce_b, kl_b,0 .. kl_b,6), the maps summed per sample."""
import os

import numpy as np
import torch

import golden_inputs as gi
import parse_helpers as ph
from oracle import spair_oracle as orc

NAMES = ("cy_logit", "cx_logit", "height_logit", "width_logit", "attr", "depth_logit")
# every z_pres of these lies more than MARGIN from 0.5 (test_evaluate_cpu.py): the count prior's hard decision cannot flip under the fp32
# step's latent bound of 1e-4
FIXTURES = ("c1_b8_step7001", "c2_b2_step1001", "ref_default_b2_step1001", "rect_h48w80_b4_step1001", "rgb_c1_b4_step1001",
            "lb2_c1_b4_step1001", "c4_b1_step1001")
MARGIN = 2e-4
E32 = 2.0 ** -24         # one rounding to nearest in fp32
BCE_TOL, KL_TOL = 2e-5, 1e-4      # the project's loss / KL bounds
MAP_CAP = 2e-3           # the project's per-tensor gradient bound: the cap of the map comparison against the oracle


def config_priors():
    from spair_pytorch_amd import config as cfg
    return [(float(np.float32(cfg.PRIORS[n][0])), float(np.float32(cfg.PRIORS[n][1]))) for n in NAMES]


def _pieces(z, pz, mu, sd, priors, recon, x):
    """The addends of the definition in float64: gauss [6] of [B,HW,cols], pres [B,HW], px [B,C,npix] and the magnitudes their fp32 bounds
    are made of."""
    z, pz = np.asarray(z, np.float64), np.asarray(pz, np.float64)
    gauss, mag = [], []
    for j in range(6):
        m, s = priors[j]
        u, v = np.asarray(mu[j], np.float64), np.asarray(sd[j], np.float64)
        vr, t1 = (v / s) ** 2, ((u - m) / s) ** 2
        lv = np.log(vr)
        gauss.append(z[..., None] * 0.5 * (vr + t1 - 1 - lv))
        mag.append(z[..., None] * (vr + t1 + 1 + np.abs(lv)))
    la, lb, lc, ld = np.log(z + 1e-9), np.log(pz + 1e-9), np.log(1 - z + 1e-9), np.log(1 - pz + 1e-9)
    p1, p2 = z * (la - lb), (1 - z) * (lc - ld)
    pres = p1 + p2
    pres_mag = (z * (4 + 5 * (np.abs(la) + np.abs(lb))) + (1 - z) * (4 + 5 * (np.abs(lc) + np.abs(ld))) + 3 * (np.abs(p1) + np.abs(p2)))
    r, xv = np.asarray(recon, np.float64), np.asarray(x, np.float64)
    B, C = r.shape[:2]
    r, xv = r.reshape(B, C, -1), xv.reshape(B, C, -1)
    with np.errstate(divide="ignore"):
        l1, l2 = np.maximum(np.log(r), -100.0), np.maximum(np.log(1 - r), -100.0)
    px = -(xv * l1 + (1 - xv) * l2)
    px_mag = xv * 5 * np.abs(l1) + (1 - xv) * (1 + 6 * np.abs(l2)) + np.abs(px)
    return gauss, mag, pres, pres_mag, px, px_mag


def terms_float64(z, pz, mu, sd, priors, beta, recon, x):
    """z, pz [B,HW]; mu, sd: six arrays [B,HW,cols] (cols = A for attr, else 1) in the order of NAMES; priors: six (mean, std); recon, x
    [B,C,I,Iw].  Returns (terms [B,9], kl_map [B,7,HW], bce_map [B,I,Iw]) in float64."""
    gauss, _, pres, _, px, _ = _pieces(z, pz, mu, sd, priors, recon, x)
    B, _, I, Iw = np.asarray(x).shape
    kl_map = np.stack([g.sum(axis=-1) for g in gauss] + [pres], axis=1)
    bce_map = px.sum(axis=1).reshape(B, I, Iw)
    kl = kl_map.sum(axis=2)
    bce = bce_map.reshape(B, -1).sum(axis=1)
    terms = np.concatenate(((bce + beta * kl.sum(axis=1))[:, None], bce[:, None], kl), axis=1)
    return terms, kl_map, bce_map


def fp32_bounds(z, pz, mu, sd, priors, beta, recon, x, slices):
    """How far an fp32 evaluation of the definition on the same stored operands may lie from terms_float64, from the operands' magnitudes
    (e = 2^-24; logf within 4 e of its result's magnitude, every other operation correctly rounded; a fused multiply-add only removes a
    rounding).
      Gaussian element: vr = (sd / s)^2 carries three roundings (3 e vr), t1 = ((mu - m) / s)^2 five (5 e t1), log vr the error of its
        operand (3 e) and its own (4 e |log vr|), the three-term sum 3 e (vr + t1 + 1 + |log vr|), the product with z one more: with
        M = z (vr + t1 + 1 + |log vr|) all of it is below 4 e M + e |value| (the factor 0.5 is exact).
      attr: the A elements through the wave's reduction tree: + 8 e sum |value|.
      presence: each log(a + 1e-9) has an operand within 2 e (relative), i.e. 2 e + 4 e |log| absolute; the two differences, the products
        with z and 1 - z (itself one rounding) and the sum one rounding each:
        e (z (4 + 5 (|la| + |lb|)) + (1 - z)(4 + 5 (|lc| + |ld|))) + 3 e (|z (la - lb)| + |(1 - z)(lc - ld)|).
      pixel and channel: log r within 4 e |log r|; 1 - r one rounding, so log(1 - r) within e + 4 e |log(1 - r)|; 1 - x, the two products
        and the sum one rounding each: e (x 5 |l1| + (1 - x)(1 + 6 |l2|) + |value|) with the clamped logs (a clamped log is exact); the
        channel sum: + C e sum |value|.
      a per-sample sum over n addends in a chain / tree of depth d: the addends' own bounds + d e sum |addend|.  The depths follow the
        kernel's fixed order with `slices` workgroups per sample: a lane's own chain, the wave tree (8), the four waves (2), the second
        stage's chain over ceil(slices / 64) partials and its tree (8).
    Returns (E_terms [B,9], E_kl [B,7,HW], E_bce [B,I,Iw])."""
    gauss, mag, pres, pres_mag, px, px_mag = _pieces(z, pz, mu, sd, priors, recon, x)
    B, C, I, Iw = np.asarray(x).shape
    HW, npix, S = pres.shape[1], I * Iw, int(slices)
    E_el = [4 * E32 * m + E32 * np.abs(g) for g, m in zip(gauss, mag)]
    E_kl = np.stack([e.sum(axis=-1) + (8 * E32 * np.abs(g).sum(axis=-1) if g.shape[-1] > 1 else 0.0) for e, g in zip(E_el, gauss)]
                    + [E32 * pres_mag], axis=1)
    E_bce = (E32 * px_mag).sum(axis=1) + C * E32 * np.abs(px).sum(axis=1)
    kl_map = np.stack([g.sum(axis=-1) for g in gauss] + [pres], axis=1)
    tail = 8 + 2 + (S + 63) // 64 + 8
    d_cell = ((HW + S - 1) // S + 3) // 4 + tail
    d_pix = 4 * (((npix + S - 1) // S + 255) // 256 + 1) + tail
    E_t = np.zeros((B, 9))
    E_t[:, 2:] = E_kl.sum(axis=2) + d_cell * E32 * np.abs(kl_map).sum(axis=2)
    E_t[:, 1] = E_bce.sum(axis=1) + d_pix * E32 * np.abs(px).sum(axis=(1, 2))
    kl_abs = np.abs(kl_map).sum(axis=2)
    E_t[:, 0] = E_t[:, 1] + abs(beta) * (E_t[:, 2:].sum(axis=1) + 8 * E32 * kl_abs.sum(axis=1)) + E32 * (
        np.abs(px).sum(axis=(1, 2)) + abs(beta) * kl_abs.sum(axis=1))
    return E_t, E_kl, E_bce.reshape(B, I, Iw)


def check_outputs(got, ref, bounds, what=""):
    """got / ref / bounds: (terms, kl_map, bce_map) triples (a None map in ``got`` is skipped).  Asserts |got - ref| <= bound elementwise
    and returns the largest fraction of the bound per output."""
    fr = []
    for name, g, r, e in zip(("terms", "kl_map", "bce_map"), got, ref, bounds):
        if g is None:
            fr.append(0.0)
            continue
        g = np.asarray(g, np.float64).reshape(r.shape)
        assert np.isfinite(g).all(), (what, name)
        err = np.abs(g - r)
        f = float((err / (e + 1e-300)).max())
        fr.append(f)
    print("%s: largest fraction of the bound: terms %.3f, kl_map %.3f, bce_map %.3f" % (what, *fr))
    assert max(fr) <= 1.0, (what, fr)
    return fr


# ---- made-up operands of the unit-level cases ---------------------------------------------------------------------------------------------
SD_LO, SD_HI = (float(np.float32(2.0) / (np.float32(1.0) + np.exp(np.float32(v)))) for v in (10.0, -10.0))     # 2 sigmoid(-+10): the step's clamps

UNIT_CASES = [
    # seed B  HW    A   C  I    Iw   permute
    (1, 1, 1, 4, 1, 1, 1, False),
    (2, 3, 2, 16, 1, 7, 9, True),
    (3, 5, 63, 50, 3, 40, 64, True),
    (4, 3, 64, 59, 1, 48, 80, True),
    (5, 1, 65, 50, 1, 128, 128, False),
    (6, 5, 121, 16, 1, 7, 9, True),
    (7, 1, 1024, 59, 3, 40, 64, True),
    (8, 3, 1024, 4, 1, 128, 128, True),
    (9, 5, 64, 50, 1, 1, 1, True),
]


def make_unit_case(seed, B, HW, A, C, I, Iw, permute):
    """Operands in cell order (fp32 values): z, pz [B,HW] with entries exactly 0 and 1; mu, sd six [B,HW,cols], sd log-uniform over
    what 2 sigmoid(clamp10(.)) can give with entries AT both ends; recon, x [B,C,I,Iw] with exact 0 / 1 in every combination."""
    rng = np.random.default_rng(seed)

    def with_ends(shape, lo_hi=(0.0, 1.0)):
        v = rng.uniform(0.0, 1.0, shape)
        pick = rng.uniform(size=shape)
        v[pick < 0.1] = lo_hi[0]
        v[pick > 0.9] = lo_hi[1]
        return v.astype(np.float32)

    z, pz = with_ends((B, HW)), with_ends((B, HW))
    if HW >= 2:
        z[0, :2], pz[0, :2] = (0.0, 1.0), (1.0, 0.0)          # a present cell the prior rules out, and the reverse
    cols = (1, 1, 1, 1, A, 1)
    mu = [(rng.standard_normal((B, HW, c)) * 2 + (7 if j in (2, 3) else 0)).astype(np.float32) for j, c in enumerate(cols)]
    sd = []
    for c in cols:
        v = np.exp(rng.uniform(np.log(SD_LO), np.log(SD_HI), (B, HW, c)))
        pick = rng.uniform(size=v.shape)
        v[pick < 0.05], v[pick > 0.95] = SD_LO, SD_HI
        sd.append(np.clip(v, SD_LO, SD_HI).astype(np.float32))
    recon, x = with_ends((B, C, I, Iw)), with_ends((B, C, I, Iw))
    # (the last sample is the one a test takes an addend out of: where it has a single cell or pixel, that one is not an all-zero edge case)
    if HW == 1:
        z[-1, 0], pz[-1, 0] = 0.25, 0.75
    if I * Iw == 1:
        recon[-1], x[-1] = 0.3, 0.7
    rows = rng.permutation(HW).astype(np.int32) if permute else None
    return dict(z=z, pz=pz, mu=mu, sd=sd, recon=recon, x=x, rows=rows)


def store_rows(c, B, HW, A):
    """The operands as the step's workspace holds them (torch CPU tensors, NaN in every element the kernel must not read): rec [N, ld_rec]
    with z_pres in column REC - 1, stat [N,16] (mu_box 0..3, sd_box 4..7, mu_depth 8, sd_depth 9, p_z 10), Oe [N, ld_oe] with the
    attribute means in its first A columns, sd_attr [N, ld_rec]; row = rows[k] * B + b."""
    REC = 4 + A + 2
    ld_rec, ld_oe = (REC + 7) // 8 * 8, (2 * A + 7) // 8 * 8
    rows = c["rows"] if c["rows"] is not None else np.arange(HW, dtype=np.int32)
    r = torch.from_numpy((rows[None, :].astype(np.int64) * B + np.arange(B)[:, None]).reshape(-1))
    N = B * HW
    rec, stat = torch.full((N, ld_rec), float("nan")), torch.full((N, 16), float("nan"))
    Oe, sda = torch.full((N, ld_oe), float("nan")), torch.full((N, ld_rec), float("nan"))
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).reshape(N, -1)
    rec[r, REC - 1] = t(c["z"])[:, 0]
    stat[r, 10] = t(c["pz"])[:, 0]
    for j in range(4):
        stat[r, j], stat[r, 4 + j] = t(c["mu"][j])[:, 0], t(c["sd"][j])[:, 0]
    stat[r, 8], stat[r, 9] = t(c["mu"][5])[:, 0], t(c["sd"][5])[:, 0]
    Oe[r, :A], sda[r, :A] = t(c["mu"][4]), t(c["sd"][4])
    return dict(rec=rec, stat=stat, Oe=Oe, sd_attr=sda, REC=REC)


def run_rows(c, st, priors, beta, maps=True, out=None, accumulate=False, scale=1.0):
    """spair_sample_terms_rows on the stored rows ``st`` (store_rows, moved to the device by the caller)."""
    from spair_pytorch_amd import _lib as L
    stat, REC = st["stat"], st["REC"]
    A = c["mu"][4].shape[-1]
    rows = None if c["rows"] is None else torch.from_numpy(c["rows"]).cuda()
    return L.sample_terms(st["rec"][:, REC - 1:REC], stat[:, 10:11], stat[:, 0:4], stat[:, 4:8], st["Oe"][:, :A], st["sd_attr"][:, :A],
                          stat[:, 8:9], stat[:, 9:10], priors, beta, st["recon"], st["x"], rows=rows, maps=maps, out=out,
                          accumulate=accumulate, scale=scale)


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------------
def fixture_operands(name):
    """A fixture's stored maps as the definition's operands (cell order), widened to float64: dict(z, mu, sd, recon, x, step, B, HW, G, Gw)."""
    z = np.load(os.path.join(ph.GOLDEN, name + ".npz"))
    B, _, G, Gw = z["z_pres"].shape
    cells = lambda v: np.asarray(v, np.float64).transpose(0, 2, 3, 1).reshape(B, G * Gw, -1)
    return dict(z=cells(z["z_pres"])[..., 0], mu=[cells(z["mean_" + n]) for n in NAMES], sd=[cells(z["sigma_" + n]) for n in NAMES],
                recon=np.asarray(z["recon_x"], np.float64), x=np.asarray(z["x"], np.float64), step=int(z["global_step"]), B=B, HW=G * Gw,
                G=G, Gw=Gw, npz=z)


def count_prior_prob(step):
    return float(1 / ((-orc.exponential_decay(step, **orc.OracleConfig().count_prior)).exp() + 1))


def oracle_p_z(zp, step, G, Gw):
    """The count prior's p_z on a float64 z_pres [B,HW] (teacher-forced): the oracle's own recursion on a square grid; on a rectangular one,
    which the oracle's compute_kl cannot take, generate_helpers.presence_float64 -- the same recursion for any cell count, pinned to the
    oracle by test_generate_cpu.py."""
    B, HW = zp.shape
    if G == Gw:
        out = []
        orc.compute_kl({}, torch.from_numpy(zp).view(B, 1, G, G), step, orc.OracleConfig(image_shape=(1, 8 * G, 8 * G)), p_z_out=out)
        return out[0].double().numpy().reshape(B, HW)
    import generate_helpers as gh
    return gh.presence_float64(HW, B, prob=np.float64(count_prior_prob(step)), z=np.round(zp))[1]


_REF = {}


def fixture_reference(name):
    """(operands, p_z, (terms, kl_map, bce_map)) of a fixture in float64, computed once per process."""
    if name not in _REF:
        o = fixture_operands(name)
        pz = oracle_p_z(o["z"], o["step"], o["G"], o["Gw"])
        _REF[name] = (o, pz, terms_float64(o["z"], pz, o["mu"], o["sd"], config_priors(), 1.0, o["recon"], o["x"]))
    return _REF[name]
