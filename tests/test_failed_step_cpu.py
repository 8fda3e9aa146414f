"""The host half of the failed-step guard (tests/test_failed_step_gpu.py has the device half): what spair_status_exchange refuses before it
launches anything, the status texts, and copies of a model that has not touched a device yet.  CPU only."""
import copy
import ctypes
import pickle

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from spair_pytorch_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.lib()


def test_status_exchange_refusals(lib):
    """NULL status or exchange ints, or a phase other than 0 / 1: SPAIR_ERR_SHAPE, nothing enqueued (no GPU here to enqueue on)."""
    fake = ctypes.c_void_p(1 << 30)
    for args in ((None, fake, fake, 0), (fake, None, fake, 1), (fake, fake, fake, 2), (fake, fake, None, -1)):
        assert lib.spair_status_exchange(*args, None) == -1


def test_status_text_names_every_bit():
    from spair_pytorch_amd.models import SPAIR
    assert SPAIR._status_text(0) == "ok"
    assert "non-finite" in SPAIR._status_text(2) and "another rank" not in SPAIR._status_text(2)
    assert "timed out" in SPAIR._status_text(1) and "non-finite" not in SPAIR._status_text(1)
    both = SPAIR._status_text(4 | 2)
    assert "non-finite" in both and "another rank" in both


def _model():
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.models import SPAIR
    cfg.set_grid(48, (2, 2, 2, 1, 1, 1))
    return SPAIR([1, 48, 48], None, torch.device("cuda"), compute_dtype="bf16")


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_copy_of_a_model_without_device_state(how):
    from spair_pytorch_amd.models import _NullWriter
    m = _model()
    c = copy.deepcopy(m) if how == "deepcopy" else pickle.loads(pickle.dumps(m))
    assert isinstance(c.writer, _NullWriter) and c.writer.add_scalar("a", 1, 2) is None      # not the None a probed __deepcopy__ would leave
    assert c._flat is None and c._status_host is None and c._status_dev is None and c._engines == {} and c._grad_buckets is None
    a, b = dict(m.named_parameters()), dict(c.named_parameters())
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].data_ptr() != b[k].data_ptr()
    assert c.compute_dtype == m.compute_dtype and c.image_shape == m.image_shape and c.raise_on_nonfinite is True


def test_null_writer_has_no_dunder_hooks():
    from spair_pytorch_amd.models import _NullWriter
    w = _NullWriter()
    assert w.add_scalar("x", 1.0, 0) is None and w.anything() is None
    with pytest.raises(AttributeError):
        w.__deepcopy__
    assert isinstance(copy.deepcopy(w), _NullWriter)
