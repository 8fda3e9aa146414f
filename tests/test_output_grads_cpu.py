"""The differentiable-outputs switch of SPAIR on the host side (no GPU): constructor argument, attribute, default, and the entry points
and SpairStepIO fields of the C ABI it runs on (include/spair_hip.h).  The gradients themselves are checked in test_output_grads_gpu.py."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fresh_cfg():
    from spair_pytorch_amd import config as cfg
    cfg.set_grid(128, (3, 2, 2, 1, 1, 1))
    cfg.INPUT_IMAGE_SHAPE[0] = 1
    cfg.N_LOOKBACK = 1


def test_switch_is_a_constructor_argument_and_defaults_off():
    _fresh_cfg()
    from spair_pytorch_amd.models import SPAIR
    m = SPAIR([1, 128, 128], None, torch.device("cpu"), differentiable_outputs=True)
    assert m.differentiable_outputs is True
    assert SPAIR([1, 128, 128], None, torch.device("cpu")).differentiable_outputs is False
    assert SPAIR([1, 128, 128], None, torch.device("cpu"), differentiable_outputs=0).differentiable_outputs is False


def test_switch_leaves_parameters_and_state_dict_alone():
    _fresh_cfg()
    from spair_pytorch_amd.models import SPAIR
    torch.manual_seed(3)
    a = SPAIR([1, 128, 128], None, torch.device("cpu"))
    torch.manual_seed(3)
    b = SPAIR([1, 128, 128], None, torch.device("cpu"), differentiable_outputs=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_output_gradient_io_fields_are_declared_and_exported():
    """spair_forward / spair_backward take the output gradients' buffers in SpairStepIO; the suffixed entry points that took them are gone."""
    from spair_pytorch_amd import _build, _lib
    hdr = open(os.path.join(ROOT, "include", "spair_hip.h")).read()
    io = re.search(r"typedef struct SpairStepIO \{(.*?)\} SpairStepIO;", hdr, re.S).group(1)
    for name in ("spair_forward", "spair_backward"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for field in ("inv_den", "grad_recon", "grad_z_where", "grad_z_pres", "aux_scratch"):
        assert re.search(r"\b%s;" % field, io), field
    _build.build(verbose=False)
    lib = _lib.lib()
    assert hasattr(lib, "spair_forward") and hasattr(lib, "spair_backward")
    for gone in ("spair_forward" + "_out", "spair_backward" + "_out", "spair_backward" + "_ev"):    # (spelled in parts: nothing else names them)
        assert not re.search(r"\b%s\b" % gone, hdr) and not hasattr(lib, gone), gone
