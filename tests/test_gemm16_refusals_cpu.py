"""What the bf16 matrix entry points refuse before any launch, with the exact code (no GPU: the library loads without one, and every call
here returns from the checks at the top of spair_gemm_nt16_impl, spair_gemm_tn16_impl, spair_pw_stack_fwd16 / _bwd16 and
spair_stem_wgrad16_impl -- none reaches a kernel launch, and no pointer is read)."""
import ctypes

import pytest

OK, ERR_SHAPE, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -4, -5


@pytest.fixture(scope="module")
def lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def _i(*a):
    return (ctypes.c_int * len(a))(*a)


def _nulls(n):
    return (ctypes.c_void_p * n)()


def nt16(lib, M=8, N=8, K=8, lda=8, ldb=8, ldc=8):
    return lib.spair_gemm_nt16(None, lda, None, ldb, None, ldc, M, N, K, None, None, 0, 0, 0, 1, None, None, None)


@pytest.mark.parametrize("kw", [dict(K=12, lda=16, ldb=16), dict(lda=12), dict(ldb=12), dict(K=1028, lda=1032, ldb=1032)])
def test_nt16_refuses_misaligned_k_and_leading_dimensions(lib, kw):
    assert nt16(lib, **kw) == ERR_ALIGN


@pytest.mark.parametrize("kw", [dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(N=-8), dict(K=-8)])
def test_nt16_refuses_non_positive_extents(lib, kw):
    assert nt16(lib, **kw) == ERR_SHAPE


def tn16(lib, M=8, N=8, R=8, lda=8, ldb=8, b_bf16=1):
    return lib.spair_gemm_tn16(None, lda, None, ldb, b_bf16, None, 8, M, N, R, None, 0, 0, None, None, ctypes.c_longlong(0), None)


@pytest.mark.parametrize("kw", [dict(lda=12), dict(lda=100, M=100), dict(ldb=12), dict(ldb=100, N=100), dict(b_bf16=0, ldb=6)])
def test_tn16_refuses_misaligned_leading_dimensions(lib, kw):
    """lda % 8; a bf16 B with ldb % 8 (an fp32 B: ldb % 4)."""
    assert tn16(lib, **kw) == ERR_ALIGN


@pytest.mark.parametrize("kw", [dict(M=0), dict(N=0), dict(R=0)])
def test_tn16_refuses_non_positive_extents(lib, kw):
    assert tn16(lib, **kw) == ERR_SHAPE


def pw_fwd(lib, L, couts, ldws, M=8):
    n = max(len(couts), 1)
    return lib.spair_conv1x1_stack_fwd16(None, _nulls(n), _i(*ldws), _i(*couts), _nulls(n), _nulls(n), None, 128, M, L, None)


def pw_bwd(lib, L, couts, ldws, kd=128, ldd=128, M=8):
    n = max(len(couts), 1)
    return lib.spair_conv1x1_stack_bwd16(None, ldd, kd, _nulls(n), _i(*ldws), _i(*couts), _nulls(n), _nulls(n), M, L, None)


def test_pointwise_stack_refuses_bad_shapes(lib):
    five = ([128] * 5, [128] * 5)
    assert pw_fwd(lib, 0, [128], [128]) == ERR_SHAPE
    assert pw_fwd(lib, 5, *five) == ERR_SHAPE
    assert pw_fwd(lib, 1, [128], [128], M=0) == ERR_SHAPE
    assert pw_bwd(lib, 0, [128], [128]) == ERR_SHAPE
    assert pw_bwd(lib, 5, *five) == ERR_SHAPE
    assert pw_bwd(lib, 1, [128], [128], kd=136, ldd=136) == ERR_SHAPE
    assert pw_bwd(lib, 1, [100], [104], kd=100, ldd=100) == ERR_SHAPE          # ldd % 8
    assert pw_bwd(lib, 1, [128], [128], M=0) == ERR_SHAPE


def test_pointwise_stack_refuses_unsupported_layers(lib):
    assert pw_fwd(lib, 1, [136], [136]) == ERR_UNSUPPORTED                     # cout > 128
    assert pw_fwd(lib, 2, [100, 128], [128, 128]) == ERR_UNSUPPORTED           # an inner cout != 128
    assert pw_fwd(lib, 3, [128, 120, 100], [128, 128, 128]) == ERR_UNSUPPORTED
    assert pw_fwd(lib, 1, [100], [120]) == ERR_UNSUPPORTED                     # forward: ldw < 128
    assert pw_fwd(lib, 1, [100], [132]) == ERR_UNSUPPORTED                     # ldw % 8
    assert pw_bwd(lib, 1, [136], [136]) == ERR_UNSUPPORTED                     # cout > 128
    assert pw_bwd(lib, 2, [100, 120], [104, 120]) == ERR_UNSUPPORTED           # backward order: only the top layer (l = 0) may be narrow
    assert pw_bwd(lib, 1, [100], [100]) == ERR_UNSUPPORTED                     # ldw % 8


def test_stem_wgrad_refuses_a_null_scratch(lib):
    rc = lib.spair_stem_wgrad16(None, None, None, None, None, ctypes.c_longlong(512 * 128 * 32), 1, 10, 2, 4, None)
    assert rc == ERR_UNSUPPORTED
