"""The fused layer1 chain (csrc/bneck_tail.h) counts the vmcnt of its weight ring, its identity loads and its stores by hand, and keeps
conv3_halo's fragment look-ahead in phase A.  The generated ISA of both builds (with the next conv1 / y only) is checked for what that
rests on.  Cross-compiles for gfx950; no GPU needed."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))


@pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_bneck_tail_has_no_spill_no_exposed_lds_wait_and_the_mfma_counts_of_the_design():
    import check_ring_isa
    rep = check_ring_isa.check_bneck_tail()
    assert len(rep) == 2, sorted(rep)
    for name, r in rep.items():
        with_c = "ILb1E" in name
        assert r["scratch"] == 0, f"{name}: {r['scratch']} scratch instructions (register spills)"
        assert 0 < r["vgprs"] <= 256, (name, r["vgprs"])
        assert r["exposed_waits"] == 0, f"{name}: {r['exposed_waits']} `s_waitcnt lgkmcnt(0)` directly behind a ds_read in the phase-A unit loop"
        # phase A: nine unrolled taps x 2 rows x 4 blocks x 3 products, run for both channel blocks of a tile (9 * 2 * 24 per tile and wave);
        # the tail: eight groups of 24 (conv3) + 24 (next conv1) products
        assert r["mfma_a"] == 9 * 24, (name, r["mfma_a"])
        assert r["mfma_bc"] == (8 * 48 if with_c else 8 * 24), (name, r["mfma_bc"])
        assert r["asm_loads"] == 4 * 8, (name, r["asm_loads"])     # four per group: group 0's behind phase A, the others' a group ahead
        assert not r["touches"], (name, r["touches"][:4])
        assert not r["compiler_vmcnt_waits"], (name, r["compiler_vmcnt_waits"])
