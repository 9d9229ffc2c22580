"""CPU: the register budget of the kernels of the symmetric list herd, from the compiler's own remarks (cross-compilation, no GPU): the two
kangaroo_sym_keys_kernel entry points and the seeding kernel such a herd is seeded by -- at most 128 VGPRs, no AGPRs, no spilled register, no scratch, four
waves per SIMD, and no static LDS for the walk."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    return {r["kernel"]: r for r in spill_report.report(tus=["kangaroo", "kangaroo_seed"])}


def budget(r):
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0, r
    assert r["vgprs"] <= 128 and r["agprs"] == 0 and r["waves_per_simd"] >= 4, r


def test_symmetric_list_walk_meets_the_budget(rows):
    walk = sorted(k for k in rows if "kangaroo_sym_keys_kernel<" in k)
    assert walk == ["void kangaroo_sym_keys_kernel<false>(KangSymArgs)", "void kangaroo_sym_keys_kernel<true>(KangSymArgs)"], sorted(rows)
    for k in walk:
        budget(rows[k])
        assert rows[k]["lds_bytes_per_block"] == 0, rows[k]


def test_seeding_of_a_symmetric_list_herd_meets_the_budget(rows):
    budget(rows["kangaroo_seed_keys_kernel(KeySeedArgs)"])
    split = [k for k in rows if k.startswith("kangaroo_split_keys_kernel(")]
    assert len(split) == 1, sorted(rows)
    budget(rows[split[0]])
