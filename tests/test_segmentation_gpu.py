"""Instance masks of the device scene generator and the device segmentation metrics on the MI355X, against segmentation_helpers.py.

Masks: exact outside the pixels mask_rule leaves out (a decision a single fp32 rounding can flip), whose share is capped.  Metrics: the
contingency table and the matches are integers and must be equal; the scores are a double evaluation of integer sums rounded once to
fp32 (2^-24 relative on values in [-1, 1]: 6e-8), held to 1e-6 absolute.  The shapes are the smallest that reach every path: one pixel,
planes that are no multiple of 4 (the one-pixel-per-lane kernel), several slices per image, the largest table (NP = 1024, K = 32:
135,300 bytes of LDS)."""
import ctypes

import numpy as np
import pytest
import torch

import golden_inputs as gi
import segmentation_helpers as sh

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-6
SCORES = ("ari", "ari_fg", "msc", "sc", "fg_iou")


# ---- 1. instance masks -------------------------------------------------------------------------------------------------------------------
def device_scene(case, masks):
    """the entry points themselves, at any `first` (batch() only reaches multiples of the batch size)"""
    from spair_pytorch_amd import _lib as L
    B, I, K, seed, first, smin, smax = case
    img = torch.empty(B, 1, I, I, device="cuda")
    bbox = torch.empty(B, K, 4, device="cuda")
    cnt = torch.empty(B, dtype=torch.int64, device="cuda")
    scratch = torch.empty(B * K * 28, device="cuda")
    if not masks:
        L.check(L.lib().spair_scenes_generate(ctypes.c_uint64(seed), ctypes.c_longlong(first), B, I, K, smin, smax, L.ptr(img), L.ptr(bbox),
                                              L.ptr(cnt), L.ptr(scratch), L.stream()), "spair_scenes_generate")
        return img, bbox, cnt
    mask = torch.full((B, I, I), -5, dtype=torch.int32, device="cuda")
    L.check(L.lib().spair_scenes_generate_masks(seed, first, B, I, K, smin, smax, L.ptr(img), L.ptr(bbox), L.ptr(cnt), L.ptr(scratch),
                                                L.ptr(mask), L.stream()), "spair_scenes_generate_masks")
    return img, bbox, cnt, mask


@pytest.fixture(scope="module")
def planes():
    return {c: sh.scene_planes(c[3], c[4], c[0], c[1], c[2], c[5], c[6]) for c in sh.SCENE_CASES}


@pytest.mark.parametrize("case", sh.SCENE_CASES)
def test_masks_against_the_reference(planes, case):
    B, I, K, seed, first, smin, smax = case
    ri, rb, rc, pl = planes[case]
    ref_mask, left, stats = sh.mask_rule(pl)
    img, bbox, cnt, mask = device_scene(case, True)
    img0, bbox0, cnt0 = device_scene(case, False)
    assert torch.equal(img, img0) and torch.equal(bbox, bbox0) and torch.equal(cnt, cnt0)          # bit for bit
    again = device_scene(case, True)
    assert torch.equal(again[3], mask) and torch.equal(again[0], img)
    m, x, c, bb = mask.cpu().numpy(), img.cpu().numpy()[:, 0], cnt.cpu().numpy(), bbox.cpu().numpy()
    assert np.array_equal(c, rc) and np.array_equal(bb, rb)
    wrong = (m != ref_mask) & ~left
    print("case %s: %d differ outside the %d left out of %d pixels; %s" % (case, int(wrong.sum()), int(left.sum()), left.size, stats))
    assert left.mean() <= sh.LEFT_OUT_CAP
    assert not wrong.any()
    assert np.array_equal(m >= 0, x > 0) and m.min() >= -1 and (m < c[:, None, None]).all()
    b, y, xx = np.nonzero(m >= 0)                                                                 # inside the glyph's own box
    box = bb[b, m[b, y, xx]]
    assert ((xx >= box[:, 0]) & (xx < box[:, 0] + box[:, 2]) & (y >= box[:, 1]) & (y < box[:, 1] + box[:, 3])).all()


def test_batch_with_masks_and_rank_sharding():
    from spair_pytorch_amd.data import DeviceScatteredDigits
    a = DeviceScatteredDigits(4096, 8, 64, 7, seed=5)
    for i in (0, 3):
        plain, with_mask = a.batch(i, epoch=1), a.batch(i, epoch=1, masks=True)
        assert len(plain) == 3 and len(with_mask) == 4
        for p, q in zip(plain, with_mask):
            assert torch.equal(p, q)
        mask = with_mask[3]
        assert mask.dtype == torch.int32 and mask.shape == (8, 64, 64) and mask.is_cuda
        assert torch.equal(mask >= 0, with_mask[0][:, 0] > 0)
    assert len(next(iter(a))) == 3
    whole = torch.cat([a.batch(i, masks=True)[3] for i in range(4)])
    r0 = DeviceScatteredDigits(4096, 8, 64, 7, seed=5, rank=0, world=2)
    r1 = DeviceScatteredDigits(4096, 8, 64, 7, seed=5, rank=1, world=2)
    assert torch.equal(r0.batch(0, masks=True)[3], whole[0:8]) and torch.equal(r1.batch(0, masks=True)[3], whole[8:16])
    assert torch.equal(r0.batch(1, masks=True)[3], whole[16:24]) and torch.equal(r1.batch(1, masks=True)[3], whole[24:32])
    assert int(whole.max()) >= 1


# ---- 2. the metric kernels on made-up label maps ------------------------------------------------------------------------------------------
def run(pred, truth, NP, K):
    from spair_pytorch_amd import metric
    return metric.segmentation(torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(truth)).cuda(), NP, K)


def check(r, pred, truth, NP, K, what=""):
    """device result against segmentation_ref: integers equal, scores within SCORE_TOL (NaN where the reference has NaN)"""
    ref = sh.segmentation_ref(pred, truth, NP, K)
    B = pred.shape[0]
    cont = r.contingency.cpu().numpy()
    assert cont.shape == (B, NP + 1, K + 1) and cont.dtype == np.int32
    assert np.array_equal(cont, ref["contingency"]), what
    assert int(cont.sum()) == pred.size
    assert np.array_equal(r.match.cpu().numpy(), ref["match"]), what
    got = np.stack([getattr(r, k).cpu().numpy() for k in SCORES], axis=1).astype(np.float64)
    assert got.shape == (B, 5)
    assert np.array_equal(np.isnan(got), np.isnan(ref["scores"])), (what, got, ref["scores"])
    err = np.nanmax(np.abs(got - ref["scores"]), initial=0.0)
    err_iou = np.abs(r.match_iou.cpu().numpy().astype(np.float64) - ref["match_iou"]).max()
    print("%s: scores off by %.3g, match_iou by %.3g" % (what, err, err_iou))
    assert err <= SCORE_TOL and err_iou <= SCORE_TOL, what
    return ref


PLANES = [(1, 1), (1, 2), (7, 9), (16, 16), (33, 65), (128, 128)]
TABLES = [(1, 1), (2, 11), (36, 11), (36, 32), (1024, 1), (1024, 32)]


@pytest.mark.parametrize("hw", PLANES)
@pytest.mark.parametrize("table", TABLES)
def test_metrics_on_made_up_maps(hw, table):
    (H, W), (NP, K) = hw, table
    B = (1, 3, 5)[(PLANES.index(hw) + TABLES.index(table)) % 3]
    pred, truth = sh.blocky_maps(1000 * H + 10 * W + NP + K, B, H, W, NP, K)
    r = run(pred, truth, NP, K)
    check(r, pred, truth, NP, K, "B %d, %dx%d, NP %d, K %d" % (B, H, W, NP, K))


def test_every_batch_size_on_an_odd_plane():
    for B in (1, 3, 5):
        pred, truth = sh.blocky_maps(B, B, 33, 65, 36, 11, background=0.3)
        check(run(pred, truth, 36, 11), pred, truth, 36, 11, "B %d" % B)


def planted(H=16, W=16, NP=36, K=11):
    """B = 8 images at H x W: 0 identical partitions (relabelled), 1 background everywhere in pred, 2 in truth, 3 on both sides, 4 one
    predicted segment over the whole image, 5 only the highest labels, 6 two segments tying on an object, 7 90 % background"""
    pred, truth = sh.blocky_maps(77, 8, H, W, NP, K, background=0.4)
    pred[0] = np.where(truth[0] >= 0, K - 1 - truth[0], -1)
    pred[1] = -1
    truth[2] = -1
    pred[3] = -1
    truth[3] = -1
    pred[4] = 7
    pred[5] = np.where(pred[5] >= 0, NP - 1, -1)
    truth[5] = np.where(truth[5] >= 0, K - 1, -1)
    pred[6], truth[6] = -1, -1
    truth[6, 2, 0:4] = 3                                  # an object of 4 pixels, halved by segments 9 and 4: IoU 2/4 each -> 4
    pred[6, 2, 0:2], pred[6, 2, 2:4] = 9, 4
    truth[6, 5, 0:3] = 0                                  # an object of 3 pixels: segment 20 has 2 of its 5 in it (2/6), segment 30 its only one (1/3)
    pred[6, 5, 0:2], pred[6, 6, 0:3], pred[6, 5, 2] = 20, 20, 30
    rng = np.random.default_rng(5)
    keep = rng.uniform(size=(H, W)) < 0.1
    pred[7], truth[7] = np.where(keep, pred[7], -1), np.where(keep, truth[7], -1)
    return pred, truth


def test_planted_cases():
    NP, K = 36, 11
    pred, truth = planted()
    r = run(pred, truth, NP, K)
    ref = check(r, pred, truth, NP, K, "planted")
    s = {k: getattr(r, k).cpu().numpy() for k in SCORES}
    assert s["ari"][0] == 1 and s["ari_fg"][0] == 1 and s["msc"][0] == 1 and s["sc"][0] == 1 and s["fg_iou"][0] == 1
    assert s["fg_iou"][1] == 0 and s["msc"][1] == 0 and (r.match[1].cpu().numpy()[ref["contingency"][1].sum(axis=0)[1:] > 0] == -1).all()
    assert np.isnan(s["ari_fg"][2]) and np.isnan(s["msc"][2]) and np.isnan(s["sc"][2]) and s["fg_iou"][2] == 0
    assert s["ari"][3] == 1 and np.isnan(s["ari_fg"][3]) and s["fg_iou"][3] == 1
    assert (r.match[4].cpu().numpy()[ref["contingency"][4].sum(axis=0)[1:] > 0] == 7).all()
    assert r.contingency[5, NP, K].item() > 0
    m6 = r.match[6].cpu().numpy()
    assert m6[3] == 4 and m6[0] == 20 and r.match_iou[6, 3].item() == 0.5 and abs(r.match_iou[6, 0].item() - 1 / 3) < 1e-7
    assert r.contingency[7, 0, 0].item() >= 0.8 * 256
    mean = r.mean()
    for k in SCORES:
        v = s[k][~np.isnan(s[k])].astype(np.float64).mean()
        assert abs(mean[k].item() - v) <= 1e-6, k


def test_out_of_range_labels_are_background():
    NP, K = 36, 11
    pred, truth = sh.blocky_maps(8, 3, 33, 65, NP, K, background=0.3)
    rng = np.random.default_rng(9)
    bad_p, bad_t = rng.uniform(size=pred.shape) < 0.1, rng.uniform(size=truth.shape) < 0.1
    dirty_p, dirty_t = pred.copy(), truth.copy()
    dirty_p[bad_p] = rng.choice(np.array([NP, -7, 2 ** 31 - 1, -2 ** 31, NP + 1000], np.int64), size=int(bad_p.sum())).astype(np.int32)
    dirty_t[bad_t] = rng.choice(np.array([K, -7, 2 ** 31 - 1, -2, 1 << 20], np.int64), size=int(bad_t.sum())).astype(np.int32)
    clean_p, clean_t = np.where(bad_p, -1, pred).astype(np.int32), np.where(bad_t, -1, truth).astype(np.int32)
    a, b = run(dirty_p, dirty_t, NP, K), run(clean_p, clean_t, NP, K)
    for k in a.__slots__:
        assert torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)), k          # bit for bit, NaN included
    check(a, dirty_p, dirty_t, NP, K, "out-of-range labels")
    # wider integer types: a label int32 cannot hold is out of range, not wrapped into it
    wide = torch.from_numpy(dirty_p.astype(np.int64)).cuda()
    wide[0, 0, 0] = 2 ** 32 + 3
    dirty_p[0, 0, 0] = -1
    from spair_pytorch_amd import metric
    c = metric.segmentation(wide, torch.from_numpy(dirty_t.astype(np.int64)).cuda(), NP, K)
    check(c, dirty_p, dirty_t, NP, K, "int64 labels")


def test_several_slices_feed_one_table():
    """B = 1 at 256 x 256 with a 37 x 12 table: 64 workgroups add into the same 444 counters"""
    NP, K = 36, 11
    pred, truth = sh.blocky_maps(21, 1, 256, 256, NP, K, background=0.8, block=16)
    r = run(pred, truth, NP, K)
    ref = check(r, pred, truth, NP, K, "1 x 256 x 256")
    # the exact comparison cannot hide a dropped pixel: one relabelled pixel of the reference changes its table
    y, x = np.argwhere(truth[0] != 0)[0]
    moved = truth.copy()
    moved[0, y, x] = 0
    assert not np.array_equal(sh.segmentation_ref(pred, moved, NP, K)["contingency"], ref["contingency"])


def test_repeatable_and_optional_outputs():
    from spair_pytorch_amd import _lib as L
    from spair_pytorch_amd import metric
    NP, K, B, H, W = 36, 11, 3, 33, 65
    pred, truth = sh.blocky_maps(4, B, H, W, NP, K)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda()
    a, b = metric.segmentation(p, t, NP, K), metric.segmentation(p, t, NP, K)
    for k in a.__slots__:
        assert torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)), k
    # the defaults: max + 1 on either side
    d = metric.segmentation(p, t)
    assert d.contingency.shape == (B, int(pred.max()) + 2, int(truth.max()) + 2)
    assert torch.equal(d.ari.view(torch.int32), a.ari.view(torch.int32)) and torch.equal(d.sc.view(torch.int32), a.sc.view(torch.int32))
    # NULL match / match_iou
    cont = torch.full((B, NP + 1, K + 1), 7, dtype=torch.int32, device="cuda")
    scores = torch.empty(B, 5, device="cuda")
    L.check(L.lib().spair_segmentation(L.ptr(p), L.ptr(t), B, H * W, NP, K, L.ptr(cont), L.ptr(scores), None, None, L.stream()), "null outputs")
    assert torch.equal(cont, a.contingency)
    for i, k in enumerate(SCORES):
        assert torch.equal(scores[:, i].view(torch.int32), getattr(a, k).view(torch.int32)), k
    # planes of a multiple of 4 pixels that do not start 16-byte aligned take the one-pixel kernel: the same results
    H, W = 16, 24
    pred, truth = sh.blocky_maps(5, B, H, W, NP, K)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda()
    a = metric.segmentation(p, t, NP, K)
    flat_p, flat_t = (torch.empty(B * H * W + 1, dtype=torch.int32, device="cuda") for _ in range(2))
    flat_p[1:], flat_t[1:] = p.reshape(-1), t.reshape(-1)
    assert flat_p[1:].data_ptr() % 16 == 4
    L.check(L.lib().spair_segmentation(L.ptr(flat_p[1:]), L.ptr(flat_t[1:]), B, H * W, NP, K, L.ptr(cont), L.ptr(scores), None, None, L.stream()),
            "unaligned")
    assert torch.equal(cont, a.contingency)
    for i, k in enumerate(SCORES):
        assert torch.equal(scores[:, i].view(torch.int32), getattr(a, k).view(torch.int32)), k


def test_benchmark_batch_once():
    """B = 256 at 128 x 128 with 256 predicted labels (the grid of the benchmark's second configuration), 11 objects"""
    NP, K = 256, 11
    pred, truth = sh.blocky_maps(31, 256, 128, 128, NP, K, background=0.85, block=8)
    check(run(pred, truth, NP, K), pred, truth, NP, K, "256 x 128 x 128")


# ---- 3. end to end: a parse scored against the generator's masks ---------------------------------------------------------------------------
@pytest.fixture
def cfg():
    from spair_pytorch_amd import config as cfg
    old = (list(cfg.INPUT_IMAGE_SHAPE), [t["stride"] for t in cfg.DEFAULT_BACKBONE_TOPOLOGY])
    yield cfg
    cfg.INPUT_IMAGE_SHAPE[:] = old[0]
    for t, s in zip(cfg.DEFAULT_BACKBONE_TOPOLOGY, old[1]):
        t["stride"] = s


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_parse_scored_against_the_masks(dtype, cfg):
    from spair_pytorch_amd import metric, segmentation
    from spair_pytorch_amd.data import DeviceScatteredDigits
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
    torch.manual_seed(3)
    m = SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
    ds = DeviceScatteredDigits(64, 8, image_side=48, max_objects=5, seed=2, obj_px=(10, 20))
    x, bbox, cnt, mask = ds.batch(1, masks=True)
    parse = m.parse(x, 2000, threshold=0.02)
    assert parse.area.shape[1] == 36 and int((parse.owner >= 0).sum()) > 0
    status = m.step_status()
    torch.manual_seed(9)
    cpu_state, gpu_state = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    r = segmentation(parse, mask, n_truth=5)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), gpu_state)
    assert m.step_status() == status
    owner, truth = parse.owner.cpu().numpy(), mask.cpu().numpy()
    check(r, owner, truth, 36, 5, "%s parse" % dtype)
    bare = metric.segmentation(parse.owner, mask, 36, 5)
    for k in r.__slots__:
        assert torch.equal(getattr(r, k).view(torch.int32), getattr(bare, k).view(torch.int32)), k
    print({k: float(v) for k, v in r.mean().items()})


def test_rectangular_owner_map(cfg):
    from spair_pytorch_amd import segmentation
    from spair_pytorch_amd.models import SPAIR
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1), image_width=80)
    torch.manual_seed(4)
    m = SPAIR([1, 48, 80], None, torch.device("cuda"), compute_dtype="bf16").to("cuda")
    x = torch.from_numpy(gi.make_image(3, 4, 80, 3)[:, :, :48, :]).contiguous().cuda()
    parse = m.parse(x, 2000, threshold=0.02)
    assert parse.owner.shape == (4, 48, 80) and parse.area.shape[1] == 60
    truth = sh.blocky_maps(6, 4, 48, 80, 60, 7, background=0.6, block=8)[1]
    r = segmentation(parse, torch.from_numpy(truth).cuda(), n_truth=7)
    check(r, parse.owner.cpu().numpy(), truth, 60, 7, "48 x 80")
