"""The direct 3x3 convolution (csrc/conv3_halo.h) requests every MFMA operand fragment one stage ahead of its use: a row's pixel fragment
under the row before, a unit's weights and first pixel row under the last row of the unit before, across the unit's barrier.  Both waves of
a SIMD pass that barrier together, so an LDS round trip that the compiler leaves exposed there stalls the matrix pipe outright.  The
generated ISA of every build is checked for it.  Cross-compiles for gfx950; no GPU needed.

What this cannot see: a wait placed one instruction behind its read is exactly as exposed as one directly behind it, and a counted wait
can be too strict as well.  The per-shape times in profiles/r10_conv3_halo.md are the proof; this only guards against the known regression
(hipcc sinking a fragment read to its first use, or issuing it ahead of a full wait for an older one)."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))


@pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_conv3_halo_unit_loop_has_no_exposed_lds_wait_and_no_spill():
    import check_ring_isa
    rep = check_ring_isa.check_halo()
    assert len(rep) >= 4, sorted(rep)      # f16x2: {128, 64} columns x {ReLU, none}
    for name, r in rep.items():
        assert r["mfma"] > 0 and r["ds_read"] > 0 and r["barriers"] >= 10, (name, r)
        assert r["scratch"] == 0, f"{name}: {r['scratch']} scratch instructions (register spills)"
        assert r["exposed_waits"] == 0, f"{name}: {r['exposed_waits']} `s_waitcnt lgkmcnt(0)` directly behind a ds_read in the unit loop"
