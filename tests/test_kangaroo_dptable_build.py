"""CPU: the unit of the distinguished-point table in device memory (csrc/kangaroo_dptable.hip), from the compiler's own remarks where it is built
(cross-compilation, no GPU): exactly the insert, resolve, load and harvest kernels, no spilled register, no scratch, no AGPRs, no LDS, eight waves per SIMD;
the library exports the six calls, the header carries the section, and the growing tame table's unit still reports its two kernels as it did."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["kangaroo_dptable_insert_kernel(DptArgs)", "kangaroo_dptable_resolve_kernel(DptArgs)", "kangaroo_dptable_load_kernel(DptLoadArgs)",
           "kangaroo_dptable_harvest_kernel(DptHarvestArgs)"]
CALLS = {"bsgs_kangaroo_dptable_begin", "bsgs_kangaroo_run_dptable", "bsgs_kangaroo_dptable_insert", "bsgs_kangaroo_dptable_load", "bsgs_kangaroo_dptable_read",
         "bsgs_kangaroo_dptable_end"}


def report(tu):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    return {r["kernel"]: r for r in spill_report.report(tus=[tu])}


def test_the_unit_holds_its_four_kernels_within_budget():
    rows = report("kangaroo_dptable")
    assert sorted(rows) == sorted(KERNELS), sorted(rows)
    for r in rows.values():
        print(r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, r
        assert r["lds_bytes_per_block"] == 0 and r["waves_per_simd"] == 8, r


def test_the_growing_tame_table_unit_is_as_it_was():
    rows = report("kangaroo_tames_gen")
    assert sorted(rows) == sorted(["kangaroo_tames_gen_insert_kernel(TamesGenArgs)", "kangaroo_tames_gen_harvest_kernel(TamesGenHarvestArgs)"]), sorted(rows)


def test_the_library_exports_the_calls():
    import pybsgs
    out = subprocess.run(["nm", "-D", "--defined-only", pybsgs.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert CALLS <= exported, CALLS - exported
    assert CALLS <= set(pybsgs.NATIVE_SYMBOLS)
    for call in CALLS:
        assert hasattr(pybsgs.Device, call[len("bsgs_"):]), call


def test_the_header_carries_the_section():
    with open(os.path.join(ROOT, "include", "bsgs_hip.h")) as f:
        text = f.read()
    assert "Kangaroo, distinguished-point table in device memory" in text
    for call in CALLS:
        assert "int %s(bsgs_dev *dev" % call in text, call
