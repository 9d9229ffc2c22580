"""CPU: the match kernel of the tame table for herds with a key word (csrc/kangaroo_tames.hip, which holds it beside the plain one), from the compiler's
own remarks where it is built (cross-compilation, no GPU): the unit holds exactly the two match kernels, the keyed one with its registers pinned, no spilled
register, no scratch, no LDS, eight waves per SIMD; the library exports the two calls; and the plain kernel still has the registers it had."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "kangaroo_tames_match_keys_kernel(TamesArgs)"
PLAIN = "kangaroo_tames_match_kernel(TamesArgs)"
CALLS = {"bsgs_kangaroo_tames_install_keys", "bsgs_kangaroo_run_tames_keys"}


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    return {r["kernel"]: r for r in spill_report.report(tus=["kangaroo_tames"])}


def test_match_keys_kernel_budget(rows):
    assert sorted(rows) == sorted([KERNEL, PLAIN]), sorted(rows)
    r = rows[KERNEL]
    print(r)
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, r
    assert r["lds_bytes_per_block"] == 0 and r["waves_per_simd"] == 8, r
    # the plain match holds 34 VGPRs; this one keeps the record's fourth vector whole and adds one address pair for the entry word
    assert r["vgprs"] <= 40, r


def test_the_plain_unit_is_as_it_was(rows):
    assert sorted(rows) == sorted([KERNEL, PLAIN]), sorted(rows)
    assert rows[PLAIN]["vgprs"] == 34


def test_the_library_exports_the_calls():
    import pybsgs
    out = subprocess.run(["nm", "-D", "--defined-only", pybsgs.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert CALLS <= exported and CALLS <= set(pybsgs.NATIVE_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "bsgs_hip.h")).read()
    assert "Kangaroo, tame table for the symmetric walk" in hdr and all(c + "(" in hdr for c in CALLS)
