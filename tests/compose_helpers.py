"""Shared by test_compose_cpu.py / test_compose_gpu.py and tests/golden/make_golden_compose.py: the fixture cases of SPAIR.compose, the
deterministic edit rule of the fixtures' latents, the float64 restatement of the layers on raw operands and its fp32 bounds.

Definition (include/spair_hip.h, "scene composition"): for sample b, pixel (y, x) and a requested cell k = h * Gw + w
    a_k = warp(alpha_k * pres_k),  m_k = warp(max(alpha_k * pres_k * depth_k, 0.01)),  D = sum over ALL cells of m + HW * 1e-9,
    layer_weight_k = a_k (m_k + 1e-9) / D,  layers_k[c] = layer_weight_k * warp(colour_k[c]);  a cell outside [0, HW): zeros."""
import os

import numpy as np

import golden_inputs as gi
import parse_helpers as ph

GOLDEN = ph.GOLDEN
TOL = 2e-4                  # the fp32 step's recon bound, and the parse weights' bound
K_LAYERS = 8
CASES = ph.PARSE_CASES      # the eight parse cases
# the unedited check runs on these base fixtures too (no compose_<case>.npz of their own)
EXTRA_BASE = ("lb3_c1_b3_step7001", "rect_lb2_h40w72_b2_step1001")
_RECT_EXTRA = {"rect_lb2_h40w72_b2_step1001": dict(C=1, H=40, W=72, strides=(2, 2, 2, 1, 1, 1), P=gi.OBJ_PX, lookback=2, wseed=34, wscale=1.0)}


def case_of(name):
    """parse_helpers.case_of, and the second rectangular base fixture."""
    return dict(_RECT_EXTRA[name]) if name in _RECT_EXTRA else ph.case_of(name)


def load_compose(name):
    return np.load(os.path.join(GOLDEN, "compose_" + name + ".npz"))


def cell_areas(owner, HW):
    """Pixels owned per cell on the rows the parse fixture keeps: owner [B,rows,Iw] -> [B,HW]."""
    return np.stack([np.bincount(o[o >= 0].astype(np.int64), minlength=HW) for o in owner])


def edit_latents(z_where, z_what, z_depth, z_pres, owner):
    """The fixtures' edit rule, per sample, from the base fixture's latents ([B,4,G,Gw], [B,A,G,Gw], [B,1,G,Gw] x 2) and the parse fixture's
    owner map.  With cells k = h * Gw + w ranked by owned area, largest first (ties: the lower index):
      * z_pres of the two largest-area cells becomes 0;
      * `present` = the cells with base z_pres > 0.5, in that ranking, without those two; where fewer than four are present, the remaining
        cells follow in descending base z_pres (ties: the lower index).  xt of present[0] moves by +0.1, xt of present[1] by -0.07, and
        z_what is swapped between present[2] and present[3];
      * among ALL cells with base z_pres > 0.5 the order of z_depth is negated: the cell holding the j-th smallest depth receives the j-th
        largest (ties: the lower index first).
    Returns (z_where, z_what, z_depth, z_pres) edited (fp32 copies) and cells int32 [B,8]: the six largest-area cells, present[0], -1."""
    zw, zt, zd, zp = (np.array(v, np.float32, copy=True) for v in (z_where, z_what, z_depth, z_pres))
    B, _, G, Gw = zw.shape
    HW = G * Gw
    area = cell_areas(owner, HW)
    cells = np.full((B, K_LAYERS), -1, np.int32)
    for b in range(B):
        rank = np.argsort(-area[b], kind="stable")
        top2 = rank[:2]
        pres0 = np.asarray(z_pres, np.float32)[b, 0].reshape(-1)
        here = pres0 > 0.5
        present = [int(k) for k in rank if here[k] and k not in top2]
        rest = [int(k) for k in np.argsort(-pres0, kind="stable") if k not in present and k not in top2]
        present = (present + rest)[:4]
        flat = lambda v, ch: v[b, ch].reshape(-1)      # (a view: the grid planes are contiguous)
        flat(zp, 0)[top2] = 0.0
        flat(zw, 0)[present[0]] += np.float32(0.1)
        flat(zw, 0)[present[1]] -= np.float32(0.07)
        for ch in range(zt.shape[1]):
            v = flat(zt, ch)
            v[present[2]], v[present[3]] = v[present[3]], v[present[2]]
        idx = np.nonzero(here)[0]
        d0 = np.asarray(z_depth, np.float32)[b, 0].reshape(-1)
        asc = idx[np.argsort(d0[idx], kind="stable")]
        flat(zd, 0)[asc] = d0[asc[::-1]]
        cells[b, :6] = rank[:6]
        cells[b, 6] = present[0]
    return zw, zt, zd, zp, cells


def to_cells(v):
    """[B,ch,G,Gw] -> [B,HW,ch] (cell order k = h * Gw + w), numpy."""
    v = np.asarray(v)
    return v.transpose(0, 2, 3, 1).reshape(v.shape[0], -1, v.shape[1])


def layers_float64(texels, nbox, pres, depth, cells, I, Iw, align_corners=False):
    """The definition in float64 on stored operands: texels [B,HW,P*P,CH] (alpha last), nbox [B,HW,4], pres / depth [B,HW], cells [B,K]
    -> (layers [B,K,C,I,Iw], layer_weight [B,K,I,Iw], recon_pre [B,C,I,Iw] = the sum over ALL cells, a, m, reach, D)."""
    texels = np.asarray(texels, np.float64)
    B, HW, PP, CH = texels.shape
    P = int(round(PP ** 0.5))
    C = CH - 1
    alpha = texels[..., C].reshape(B, HW, P, P)
    a, m, reach = ph.composite_parts(alpha, nbox, pres, depth, I, Iw, align_corners)
    D = m.sum(axis=1, keepdims=True) + HW * 1e-9
    w = a * (m + 1e-9) / D
    nb = np.asarray(nbox, np.float64).reshape(B * HW, 4)
    u = np.arange(P, dtype=np.float64)
    sx, sy = ph.src_coords(nb[:, 0], nb[:, 2], Iw, P, align_corners), ph.src_coords(nb[:, 1], nb[:, 3], I, P, align_corners)
    hx = np.maximum(0, 1 - np.abs(sx[:, :, None] - u))
    hy = np.maximum(0, 1 - np.abs(sy[:, :, None] - u))
    col = np.stack([np.einsum("niv,nvu,nju->nij", hy, texels[..., c].reshape(B * HW, P, P), hx).reshape(B, HW, I, Iw) for c in range(C)], 2)
    cells = np.asarray(cells, np.int64)
    K = cells.shape[1]
    ok = (cells >= 0) & (cells < HW)
    kk = np.where(ok, cells, 0)
    bi = np.arange(B)[:, None]
    lw = w[bi, kk] * ok[:, :, None, None]
    lay = lw[:, :, None] * col[bi, kk]
    return lay, lw, (w[:, :, None] * col).sum(axis=1), a, m, reach, D, col


def layer_bounds(a, m, reach, nbox, pres, P):
    """fp32 against float64 on the same stored operands, in the style of parse_helpers.fp32_bounds, with D taken from the renderer's own
    stored 1/D: E_w as there (the u / D part; the renderer's D is a sum of n fp32 terms in its own order, and 1/D one more rounding), and
    for a layer |d(w col)| <= E_w col + w E_col + 2^-23 w col, where the warped colour of texels in [0, 1] moves by at most dx + dy + 2^-22
    with the source coordinate (1-Lipschitz per axis), as a and m do.  For the sum of the layers of all cells against recon: both are
    fp32 evaluations of the same float64 sum, each term within E_layer of it, plus the n-term fp32 summation of the test's own sum and of
    the kernel's numerator (n 2^-24 times the sum of magnitudes each).  Returns (w, E_w, E_col), each [B,HW,I,Iw]; layer_error
    combines them."""
    B, HW = a.shape[:2]
    w, E_w, _ = ph.fp32_bounds(a, m, reach, nbox, pres, P)
    nb = np.asarray(nbox, np.float64).reshape(B, HW, 4)
    d_axis = lambda t, s: 2.0 ** -24 * P * (2.5 / s + np.abs(2 * t - 1) / s + 3)
    d = (d_axis(nb[..., 0], nb[..., 2]) + d_axis(nb[..., 1], nb[..., 3]))[:, :, None, None]
    E_col = (d + 2.0 ** -22) * reach
    E_w = E_w + 2.0 ** -22 * w         # 1/D stored by the renderer, then one product with it
    return w, E_w, E_col


def layer_error(w, E_w, E_col, col):
    """|fp32 layer - float64 layer| <= E_w (col + E_col) + w E_col + 2^-22 w col, [B,HW,C,I,Iw] (col: the float64 warped colours)."""
    return E_w[:, :, None] * (col + E_col[:, :, None]) + w[:, :, None] * E_col[:, :, None] + 2.0 ** -22 * w[:, :, None] * col
