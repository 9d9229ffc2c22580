"""CPU: the register budget of the symmetric kangaroo kernel, from the compiler's own remarks (cross-compilation, no GPU): both instantiations -- blocks of four
waves with one inversion per block, and one-wave blocks -- at four waves per SIMD, at most 128 VGPRs, no spilled VGPR, no scratch, no static LDS."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symmetric_kangaroo_kernel_does_not_spill():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    rows = {r["kernel"]: r for r in spill_report.report(tus=["kangaroo"])}
    walk = [r for k, r in rows.items() if "kangaroo_sym_kernel<" in k]
    assert sorted(r["kernel"] for r in walk) == ["void kangaroo_sym_kernel<false>(KangSymArgs)", "void kangaroo_sym_kernel<true>(KangSymArgs)"], sorted(rows)
    for r in walk:
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0, r
        assert r["vgprs"] <= 128 and r["agprs"] == 0 and r["waves_per_simd"] >= 4, r
        assert r["lds_bytes_per_block"] == 0, r                       # the jump table is read from device memory; the inversion regions are dynamic LDS
