"""The token-stationary f16x2 Linear (csrc/lin_x2.hip) counts the vmcnt of its weight ring and of its two stores per unit by hand and reads
its weight fragments two K-steps ahead of the MFMAs that use them.  The generated ISA of both builds (K = 256, K = 384) is checked for
what that rests on.  Cross-compiles for gfx950; no GPU needed."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))


@pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_lin_x2_has_no_spill_no_exposed_lds_wait_and_no_uncounted_vmcnt_wait():
    import check_ring_isa
    rep = check_ring_isa.check_lin_x2()
    assert len(rep) == 2, sorted(rep)
    for name, r in rep.items():
        K = 256 if "ILi256E" in name else 384
        assert r["scratch"] == 0, f"{name}: {r['scratch']} scratch instructions (register spills)"
        assert 0 < r["vgprs"] <= 256, (name, r["vgprs"])
        # a unit: K / 32 K-steps x two 16-column blocks x three products; its two stores; one counted wait (+ barrier)
        assert r["mfma"] == K // 32 * 6, (name, r["mfma"])
        assert r["stores"] == 2 and r["counted_waits"] == 1, (name, r["stores"], r["counted_waits"])
        assert r["exposed_waits"] == 0, f"{name}: {r['exposed_waits']} `s_waitcnt lgkmcnt(0)` directly behind a ds_read in the unit loop"
        assert not r["compiler_vmcnt_waits"], (name, r["compiler_vmcnt_waits"])
