"""The f16x2 grouped 3x3 kernel (csrc/gconv_x2.hip) holds the next tile's halo patch (36 registers), the tile's fp32 residual and three
MFMA blocks' accumulators per wave, and needs two workgroups per CU (two waves per SIMD: at most 256 VGPRs) to hide its loads.  The
generated ISA of both builds (f16x2 output, fp32 output with the residual) is checked for that, and for the MFMAs of a tile:
three blocks per wave x nine taps x two 16-channel N-blocks x three products.  Cross-compiles for gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not available")
def test_gconv_x2_has_no_scratch_fits_two_workgroups_per_cu_and_162_mfmas_per_tile(tmp_path):
    import check_ring_isa
    out = str(tmp_path / "gconv_x2.s")
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                    os.path.join(ROOT, "ocr_vi_invoice_amd", "csrc", "gconv_x2.hip"), "-o", out], check=True, capture_output=True)
    text = open(out).read()
    bodies = check_ring_isa.kernel_bodies(text, "_ZN5ocrvi15gconv_x2_kernel")
    assert len(bodies) == 2, sorted(bodies)
    for name, body in bodies.items():
        meta = re.search(r"\.name:\s+" + re.escape(name) + r"\n(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S)
        assert meta, name
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta.group(1)).group(1))
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta.group(1)).group(1))
        scratch = [t for t, _ in body if t.startswith("scratch_")]
        assert not scratch and private == 0 and int(meta.group(2)) == 0, (name, len(scratch), private, meta.group(2))
        assert 0 < vgprs <= 256, (name, vgprs)
        mfma = sum(1 for t, _ in body if t.startswith("v_mfma_f32_16x16x32"))
        assert mfma == 3 * 9 * 2 * 3, (name, mfma)
