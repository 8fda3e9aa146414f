"""The tiling of the patch-resident convolutions (cp_plan in conv_s2.hip, dg_tiling in conv_s2_dgrad.hip) against its Python transcription
f64_hold.patch_tiling, through spair_conv_s2k4_tiling -- the very code the launchers run, asked without a device -- and what the
patch-resident, stem and fused-decoder entry points refuse before any launch, with the exact code.

No GPU: the library loads without one; spair_conv_s2k4_tiling is host arithmetic, and every other call here returns from the checks at the
top of its entry point -- none reaches a kernel launch, and no pointer is read (the non-NULL ones point at a few bytes of host memory).

The decisions tests/test_patch_edges_gpu.py builds its cases on are asserted line by line (test_the_decisions_the_gpu_cases_rely_on):
the library agrees with every one of them.  One figure differs from the table this file was written from, by arithmetic and not by
the library: at Hout = 132 the last tile of an image has 16 rows (132^2 = 17424 = 68 * 256 + 16), not 17; the tile counts (69 per image) stand."""
import ctypes

import pytest

from f64_hold import CP_PPX, DG_PPX, patch_tiling, patch_windows

OK, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -4
BATCHES = (1, 2, 3, 24, 25, 28, 29, 98, 99, 300)


@pytest.fixture(scope="module")
def lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def tiling(lib, dgrad, B, H):
    """(rc, tiles, tpi); the outputs start as -1, which a refusal must leave."""
    t, p = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.spair_conv_s2k4_tiling(dgrad, B, H, ctypes.byref(t), ctypes.byref(p))
    return rc, t.value, p.value


@pytest.mark.parametrize("dgrad", [0, 1])
def test_library_tiling_equals_the_mirror(lib, dgrad):
    """Every H in 1 .. 140 (Hout of the forward, Ho of the data gradient) at ten batch sizes: return code, tile count and tiles per image."""
    seen = set()
    for H in range(1, 141):
        for B in BATCHES:
            want = patch_tiling(dgrad, B, H)
            got = tiling(lib, dgrad, B, H)
            assert got == ((ERR_UNSUPPORTED, -1, -1) if want is None else (OK,) + want), (dgrad, B, H, got, want)
            seen.add("refused" if want is None else "per-image" if want[1] else "whole-batch")
    assert seen == {"refused", "per-image", "whole-batch"}


def test_tiling_query_refuses_bad_arguments(lib):
    t = ctypes.c_int(-1)
    assert lib.spair_conv_s2k4_tiling(0, 1, 8, None, ctypes.byref(t)) == ERR_SHAPE
    assert lib.spair_conv_s2k4_tiling(1, 1, 8, ctypes.byref(t), None) == ERR_SHAPE
    for dgrad in (0, 1):
        assert tiling(lib, dgrad, 0, 8)[0] == ERR_UNSUPPORTED and tiling(lib, dgrad, 1, 0)[0] == ERR_UNSUPPORTED
        assert tiling(lib, dgrad, -1, 8)[0] == ERR_UNSUPPORTED


# (H, B): (tiles, tiles per image) or None = refused, and the largest window of the whole-batch / of the per-image tiling
FWD_DECISIONS = {
    (1, 98): ((1, 0), 392, 4),            # one tile over 98 images, its window exactly CP_PPX
    (1, 99): ((99, 1), 396, 4),           # one image more: per-image tiles of ONE row
    (3, 24): ((1, 0), 384, 16),           # 24 images in one tile
    (3, 25): ((25, 1), 400, 16),
    (132, 1): ((69, 0), 392, 392),        # the largest accepted side: exactly CP_PPX
    (132, 2): ((138, 69), 525, 392),      # per image 68 full tiles and one of 16 rows (132^2 = 68 * 256 + 16)
    (133, 1): (None, 393, 393),
    (133, 3): (None, 527, 393),
    (7, 40): ((8, 0), 349, 64),           # tiles spanning 5 - 6 images, partial last tile (1960 = 7 * 256 + 168)
    (66, 2): ((36, 18), 395, 328),
}
DGRAD_DECISIONS = {
    (1, 28): ((1, 0), 252, 9),
    (1, 29): ((29, 1), 261, 9),
    (123, 1): ((121, 0), 255, 255),
    (123, 2): ((242, 121), 380, 255),
    (124, 1): (None, 257, 257),
    (124, 3): (None, 382, 257),
    (7, 5): ((3, 0), 162, 81),            # 64 class pixels per image: 2 images per tile, the last tile half full
}


@pytest.mark.parametrize("dgrad,table", [(0, FWD_DECISIONS), (1, DGRAD_DECISIONS)])
def test_the_decisions_the_gpu_cases_rely_on(lib, dgrad, table):
    cap = DG_PPX if dgrad else CP_PPX
    for (H, B), (want, whole, per_image) in table.items():
        assert patch_windows(dgrad, B, H) == (whole, per_image), (H, B)
        assert patch_tiling(dgrad, B, H) == want, (H, B)
        rc, tiles, tpi = tiling(lib, dgrad, B, H)
        assert (rc, tiles, tpi) == ((ERR_UNSUPPORTED, -1, -1) if want is None else (OK,) + want), (H, B, rc, tiles, tpi)
        # the decision follows from the windows: whole-batch tiles iff they fit, else per-image tiles iff those fit
        assert (want is not None and want[1] == 0) == (whole <= cap) and (want is None) == (per_image > cap), (H, B)
    if dgrad == 0:
        assert 132 * 132 == 68 * 256 + 16
    # the persistent data gradient's cases at Ho = 7 (2 images per 128-pixel tile): B = 2 t gives t whole-batch tiles, whatever t
    if dgrad:
        for t in (5, 260, 513, 613):
            assert tiling(lib, 1, 2 * t, 7) == (OK, t, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals in front of the launch
# ---------------------------------------------------------------------------------------------------------------------------------------------
_HOST = (ctypes.c_char * 64)()          # a non-NULL pointer for the entry points that test theirs; never read


def _h():
    return ctypes.cast(_HOST, ctypes.c_void_p)


@pytest.mark.parametrize("Hin,Hout", [(16, 8), (19, 8), (17, 8), (18, 7), (4, 2)])
def test_conv_s2k4_fwd16_refuses_a_side_that_is_not_2_hout_plus_2(lib, Hin, Hout):
    assert Hin != 2 * Hout + 2
    assert lib.spair_conv_s2k4_fwd16(None, None, None, None, 2, Hin, Hout, None) == ERR_UNSUPPORTED
    assert lib.spair_conv_s2k4_fwd16_mask(None, None, None, None, _h(), 2, Hin, Hout, None) == ERR_UNSUPPORTED


def test_conv_s2k4_entry_points_refuse_a_null_mask_and_an_untileable_side(lib):
    assert lib.spair_conv_s2k4_fwd16_mask(None, None, None, None, None, 2, 18, 8, None) == ERR_SHAPE
    assert lib.spair_conv_s2k4_dgrad16_bits(None, None, None, None, None, None, None, 2, 8, None) == ERR_SHAPE
    assert lib.spair_conv_s2k4_fwd16(None, None, None, None, 1, 2 * 133 + 2, 133, None) == ERR_UNSUPPORTED
    assert lib.spair_conv_s2k4_fwd16(None, None, None, None, 0, 18, 8, None) == ERR_UNSUPPORTED
    assert lib.spair_conv_s2k4_dgrad16(None, None, None, None, None, None, None, 1, 124, None) == ERR_UNSUPPORTED
    assert lib.spair_conv_s2k4_dgrad16_bits(None, None, None, None, None, _h(), None, 1, 124, None) == ERR_UNSUPPORTED


def dec_fwd(lib, N=8, A=50, n_out=1568, ld_za=56, ld_s=None):
    f = ctypes.c_float
    return lib.spair_decoder_fwd16(None, ld_za, None, None, None, None, None, None, None, None, None, n_out if ld_s is None else ld_s,
                                   ctypes.c_longlong(N), A, n_out, f(1.0), f(1.0), f(0.0), None, None)


@pytest.mark.parametrize("kw", [dict(n_out=32), dict(n_out=2080), dict(n_out=1352), dict(A=65, ld_za=72), dict(ld_za=60), dict(ld_za=50),
                                dict(ld_s=1572), dict(n_out=64, ld_s=68)])
def test_decoder_fwd16_refusals(lib, kw):
    """n_out below 64, above 2048 and no multiple of 32 (1352 = 2 x 26 x 26 is one of 8 only: the backward takes it, the forward does
    not); A above 64; leading dimensions that are no multiple of 8."""
    assert dec_fwd(lib, **kw) == ERR_UNSUPPORTED


def dec_bwd(lib, N=8, A=50, n_out=1568, ld_s=None, ld2=None, ld_dza=56):
    return lib.spair_decoder_bwd16(None, n_out if ld_s is None else ld_s, None, n_out if ld2 is None else ld2, None, None, None, None, None,
                                   None, None, ld_dza, ctypes.c_longlong(N), A, n_out, None)


@pytest.mark.parametrize("kw", [dict(A=0), dict(A=65, ld_dza=72), dict(n_out=60, ld_s=64, ld2=64), dict(ld2=1572), dict(n_out=72, ld2=76),
                                dict(ld_s=1572), dict(n_out=56), dict(N=0)])
def test_decoder_bwd16_refusals(lib, kw):
    assert dec_bwd(lib, **kw) == ERR_UNSUPPORTED


@pytest.mark.parametrize("I,pre,post", [(29, 1, 1), (8, 0, 1), (611, 1, 1)])
def test_stem_conv_fwd_mask_refuses_an_odd_padded_side(lib, I, pre, post):
    """The mask is written by the matrix-core stem only, which takes an even padded side (the odd one runs on the FMA kernel, without a
    mask).  The shape itself is a valid one: the same call with the padded side one larger is refused for no such reason -- it cannot be
    shown here, where only refused calls may run."""
    Hin = I + pre + post
    assert Hin % 2 == 1
    Hout = (Hin - 4) // 2 + 1
    assert lib.spair_stem_conv_fwd_mask(_h(), _h(), _h(), _h(), _h(), 2, I, pre, Hin, Hout, None) == ERR_UNSUPPORTED
    assert lib.spair_stem_conv_fwd_mask(_h(), _h(), _h(), _h(), None, 2, I, pre, Hin, Hout, None) == ERR_SHAPE
    assert lib.spair_stem_conv_fwd_mask(_h(), _h(), _h(), _h(), _h(), 2, I, pre, Hin, Hout + 1, None) == ERR_SHAPE
