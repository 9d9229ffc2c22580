"""CPU: the register budget of the two herd seeding kernels (csrc/kangaroo_seed.hip: one Q for the call, one Q per key of a list), from the compiler's own
remarks where they are built (cross-compilation, no GPU): exactly these two kernels, each at most 128 VGPRs at four waves per SIMD, no AGPRs, no spilled VGPR,
no scratch -- and no walk instantiation in this unit.  The list kernel spills no SGPR either (the single-Q kernel, which holds Q in SGPRs, spills some)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_Q, PER_KEY = "kangaroo_seed_kernel(SeedArgs)", "kangaroo_seed_keys_kernel(KeySeedArgs)"


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    rows = {r["kernel"]: r for r in spill_report.report(tus=["kangaroo_seed"])}
    assert sorted(rows) == sorted([ONE_Q, PER_KEY]), sorted(rows)
    return rows


def test_kangaroo_seed_kernel_does_not_spill(rows):
    r = rows[ONE_Q]
    assert r["vgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0, r
    assert r["vgprs"] <= 128 and r["agprs"] == 0 and r["waves_per_simd"] >= 4, r


def test_kangaroo_seed_keys_kernel_does_not_spill(rows):
    r = rows[PER_KEY]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0, r
    assert r["vgprs"] <= 128 and r["agprs"] == 0 and r["waves_per_simd"] >= 4, r
