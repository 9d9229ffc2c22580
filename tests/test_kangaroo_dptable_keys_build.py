"""CPU: the unit of the distinguished-point table for a key list (csrc/kangaroo_dptable_keys.hip), from the compiler's own remarks where it is built
(cross-compilation, no GPU): exactly its one kernel, the keyed insert, with the register counts DESIGN.md 10 quotes beside the unkeyed insert's, no spilled
register, no scratch, no AGPRs, no LDS, eight waves per SIMD; the units it stands beside report what they did; the library exports the three calls and the
header carries the section."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["kangaroo_dptable_insert_keys_kernel(DptKeysArgs)"]
CALLS = {"bsgs_kangaroo_dptable_begin_keys", "bsgs_kangaroo_run_dptable_keys", "bsgs_kangaroo_dptable_insert_keys"}
UNKEYED = ["kangaroo_dptable_insert_kernel(DptArgs)", "kangaroo_dptable_resolve_kernel(DptArgs)", "kangaroo_dptable_load_kernel(DptLoadArgs)",
           "kangaroo_dptable_harvest_kernel(DptHarvestArgs)"]


def report(tu):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    return {r["kernel"]: r for r in spill_report.report(tus=[tu])}


def test_the_unit_holds_its_kernel_within_budget():
    rows = report("kangaroo_dptable_keys")
    assert sorted(rows) == sorted(KERNELS), sorted(rows)
    for r in rows.values():
        print(r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, r
        assert r["lds_bytes_per_block"] == 0 and r["waves_per_simd"] == 8, r
    # the herd is a kernel argument, wave-uniform: the keyed insert takes the unkeyed insert's 40 VGPRs and two SGPRs more than its 47
    r = rows[KERNELS[0]]
    assert (r["vgprs"], r["sgprs"]) == (40, 49), r


def test_the_units_beside_it_are_as_they_were():
    rows = report("kangaroo_dptable")
    assert sorted(rows) == sorted(UNKEYED), sorted(rows)
    assert (rows[UNKEYED[0]]["vgprs"], rows[UNKEYED[0]]["sgprs"]) == (40, 47), rows[UNKEYED[0]]
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
    assert pybsgs.KANGAROO_DPT_KEY_SHIFT == 8


def test_the_header_carries_the_section():
    with open(os.path.join(ROOT, "include", "bsgs_hip.h")) as f:
        text = f.read()
    assert "Kangaroo, distinguished-point table for a key list" in text
    assert "#define BSGS_KANGAROO_DPT_KEY_SHIFT 8" in text
    for call in CALLS:
        assert "int %s(bsgs_dev *dev" % call in text, call
