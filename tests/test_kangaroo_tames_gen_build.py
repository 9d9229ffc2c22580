"""CPU: the unit of the tame table grown on the device (csrc/kangaroo_tames_gen.hip), from the compiler's own remarks where it is built (cross-compilation,
no GPU): exactly the insert and the harvest kernel, no spilled register, no scratch, no AGPRs, no LDS, eight waves per SIMD; the library exports the five
calls, the header carries the section, and the search's unit still reports its two kernels as it did."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSERT = "kangaroo_tames_gen_insert_kernel(TamesGenArgs)"
HARVEST = "kangaroo_tames_gen_harvest_kernel(TamesGenHarvestArgs)"
CALLS = {"bsgs_kangaroo_tames_gen_begin", "bsgs_kangaroo_run_tames_gen", "bsgs_kangaroo_tames_gen_insert", "bsgs_kangaroo_tames_gen_read", "bsgs_kangaroo_tames_gen_end"}


def report(tu):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    return {r["kernel"]: r for r in spill_report.report(tus=[tu])}


def test_the_unit_holds_the_insert_and_the_harvest_within_budget():
    rows = report("kangaroo_tames_gen")
    assert sorted(rows) == sorted([INSERT, HARVEST]), sorted(rows)
    for r in rows.values():
        print(r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, r
        assert r["lds_bytes_per_block"] == 0 and r["waves_per_simd"] == 8, r


def test_the_search_unit_is_as_it_was():
    rows = report("kangaroo_tames")
    assert sorted(rows) == sorted(["kangaroo_tames_match_kernel(TamesArgs)", "kangaroo_tames_match_keys_kernel(TamesArgs)"]), sorted(rows)
    assert rows["kangaroo_tames_match_kernel(TamesArgs)"]["vgprs"] == 34


def test_the_library_exports_the_calls():
    import pybsgs
    out = subprocess.run(["nm", "-D", "--defined-only", pybsgs.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert CALLS <= exported, CALLS - exported
    assert CALLS <= set(pybsgs.NATIVE_SYMBOLS)


def test_the_header_carries_the_section():
    with open(os.path.join(ROOT, "include", "bsgs_hip.h")) as f:
        text = f.read()
    assert "Kangaroo, tame table grown on the device" in text
    for call in CALLS:
        assert "int %s(bsgs_dev *dev" % call in text, call
    for k, name in enumerate(["DEAD", "DUPLICATE", "TAG_ZERO", "FULL"]):
        assert "#define BSGS_KANGAROO_GEN_%s %du" % (name, k) in text
