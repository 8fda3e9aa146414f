"""The ctypes mirrors of the C ABI's structs (_lib.SpairDims, SpairStep, SpairStepIO) against include/spair_hip.h.  A host program compiled
against the header with the compiler _build.py uses prints each struct's sizeof and every field's offsetof and size; the mirrors must have
the header's fields in the header's order, at the same offsets, with the same sizes.  And the one check of the step's entry points that needs
no GPU: both refuse a NULL among the inputs they both read before anything is enqueued.  CPU only."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spair_hip.h")
STRUCTS = ("SpairDims", "SpairStep", "SpairStepIO")


def header_fields(name):
    """The field names of `typedef struct name {...} name;` in the header, in declaration order."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")
        names += [re.sub(r"\[.*\]", "", v).strip(" *") for v in [first.split()[-1]] + more]
    return names


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{struct: sizeof, "struct.field": (offsetof, sizeof)} as the compiler lays out the header."""
    from spair_pytorch_amd import _build
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "spair_hip.h"', "int main(void) {"]
    for s in STRUCTS:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f in header_fields(s):
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f))
    lines += ["    return 0;", "}"]
    d = tmp_path_factory.mktemp("abi_layout")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_build.HIPCC, "-x", "c++", "-I" + _build.INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True,
                   text=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    layout = {}
    for line in out.splitlines():
        key, *vals = line.split()
        layout[key] = tuple(int(v) for v in vals) if len(vals) > 1 else int(vals[0])
    return layout


@pytest.mark.parametrize("name", STRUCTS)
def test_mirror_matches_the_header(name, c_layout):
    from spair_pytorch_amd import _lib
    mirror = getattr(_lib, name)
    fields = header_fields(name)
    assert [f for f, _ in mirror._fields_] == fields
    assert ctypes.sizeof(mirror) == c_layout[name]
    for f in fields:
        assert (getattr(mirror, f).offset, getattr(mirror, f).size) == c_layout["%s.%s" % (name, f)], f


def test_header_fields_of_the_step_io():
    """What the parser above reads from the header for SpairStepIO (so a parser that read nothing could not pass the test above)."""
    assert header_fields("SpairStepIO") == [
        "params", "x", "eps_box", "eps_attr", "eps_depth", "u_pres", "workspace", "loss_out", "recon", "z_where", "z_pres", "inv_den",
        "grad_loss", "grads", "ev_decoder", "ev_cells", "ev_backbone", "grad_recon", "grad_z_where", "grad_z_pres", "aux_scratch", "grad_x",
        "x_scratch", "bce_target"]


def test_models_exports_the_mirrors():
    from spair_pytorch_amd import _lib, models
    assert models.SpairDims is _lib.SpairDims and models.SpairStep is _lib.SpairStep
    assert callable(models.make_dims)


SHARED = ("params", "x", "eps_box", "eps_attr", "eps_depth", "u_pres", "workspace")


@pytest.mark.parametrize("missing", SHARED)
@pytest.mark.parametrize("direction", ("spair_forward", "spair_backward"))
def test_step_refuses_a_missing_shared_input(direction, missing):
    """make_ctx checks what both directions read, so the backward too returns SPAIR_ERR_SHAPE for a NULL noise map instead of launching kernels
    that read it.  Every other field is a fake address: nothing is dereferenced or enqueued before the check (no GPU here to enqueue on)."""
    from spair_pytorch_amd import _build, _lib as L
    from spair_pytorch_amd import config as cfg
    from spair_pytorch_amd.models import make_dims, step_scalars
    _build.build(verbose=False)
    d = make_dims(2, [1, 48, 48], [dict(t) for t in cfg.DEFAULT_BACKBONE_TOPOLOGY], "bf16")
    fake = 1 << 30
    io = L.SpairStepIO(**{f: fake for f in SHARED + ("loss_out", "recon", "z_where", "z_pres", "grad_loss", "grads")})
    setattr(io, missing, None)
    rc = getattr(L.lib(), direction)(ctypes.byref(d), ctypes.byref(step_scalars(0, 2)), ctypes.byref(io), None)
    assert rc == -1          # SPAIR_ERR_SHAPE
