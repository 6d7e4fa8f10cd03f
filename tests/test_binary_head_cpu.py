"""CPU: the surface of the binary-only detector forward (ocrvi_det_forward_binary) -- the C ABI symbols, the Python signatures and the
ISA of the kernels its epilogue is compiled into.  No GPU: nothing is launched."""
import inspect
import os
import re
import shutil
import sys

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "tools"))

NEW = ("ocrvi_det_binary_workspace_bytes", "ocrvi_det_forward_binary")


def test_new_symbols_are_declared_listed_and_exported():
    from ocr_vi_invoice_amd import _lib
    header = open(os.path.join(REPO, "include", "ocrvi.h")).read()
    declared = set(re.findall(r"\b(ocrvi_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/ocrvi.h"
        assert name in _lib.EXPORTS, f"{name} is not listed in _lib.EXPORTS"
        assert hasattr(lib, name), f"libocrvi.so does not export {name}"
    # the header points callers that read `binary` alone at the new entry and cites what it replaces
    assert "pipeline2.py:318" in header and re.search(r"head\.py:34.*head\.py:38|head\.py:34,\s*38", header, re.S)
    assert lib.ocrvi_abi_version() == _lib.ABI_VERSION >= 3


def test_python_surface_has_the_binary_head_option_off_by_default():
    from ocr_vi_invoice_amd import DBNetPP, Engine, pipeline
    assert callable(getattr(DBNetPP, "forward_binary", None))
    assert list(inspect.signature(DBNetPP.forward_binary).parameters) == ["self", "x"]
    for fn in (Engine.__init__, pipeline.detect_and_recognize, pipeline.detect_and_recognize_pages):
        p = inspect.signature(fn).parameters.get("binary_head")
        assert p is not None, f"{fn.__qualname__} has no binary_head parameter"
        assert p.default is False, (fn.__qualname__, p.default)
    # forward() keeps its signature: the new forward is additive
    assert list(inspect.signature(DBNetPP.forward).parameters) == ["self", "x", "binary_only"]


def test_no_new_environment_switch_selects_the_forward():
    """The choice between the two forwards is an API argument: det_model.hip reads no environment variable."""
    src = open(os.path.join(REPO, "ocr_vi_invoice_amd", "csrc", "det_model.hip")).read()
    assert "ocrvi_det_forward_binary" in src and "getenv" not in src


@pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")
@pytest.mark.parametrize("src", ["conv_f32.hip", "conv_bf16.hip", "conv_f16.hip", "conv_f16x2.hip"])
def test_db_bin_epilogue_is_compiled_in_and_spills_nothing(src):
    """ST_DB_BIN lives in the epilogue of every conv_gemm build whose waves own 64 columns: those builds still use no scratch, and the
    store mode exists in the sources they are compiled from."""
    import check_ring_isa
    csrc = os.path.join(REPO, "ocr_vi_invoice_amd", "csrc")
    assert "ST_DB_BIN" in open(os.path.join(csrc, "conv_gemm.h")).read()
    assert "db_sigmoid" in open(os.path.join(csrc, "conv_gemm.h")).read() and "db_sigmoid" in open(os.path.join(csrc, "kernels.hip")).read()
    rep = check_ring_isa.check_scratch(src)
    assert rep, src
    bad = {n: v for n, v in rep.items() if v[0] != 0}
    assert not bad, f"kernels with scratch instructions: {bad}"
