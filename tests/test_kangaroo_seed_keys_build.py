"""CPU: the register budget of the per-key herd seeding kernel (csrc/kangaroo_seed_keys.hip), from the compiler's own remarks where it is built
(cross-compilation, no GPU): one kernel, at most 128 VGPRs at four waves per SIMD, no AGPRs, no spilled VGPR, no scratch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kangaroo_seed_keys_kernel_does_not_spill():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    rows = {r["kernel"]: r for r in spill_report.report(tus=["kangaroo_seed_keys"])}
    assert sorted(rows) == ["kangaroo_seed_keys_kernel(KeySeedArgs)"], sorted(rows)
    r = rows["kangaroo_seed_keys_kernel(KeySeedArgs)"]
    assert r["vgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0, r
    assert r["vgprs"] <= 128 and r["agprs"] == 0 and r["waves_per_simd"] >= 4, r
