"""CPU: the unit of the kangaroo verification (csrc/kangaroo_verify.hip), from the compiler's own remarks where it is built (cross-compilation, no GPU): exactly
the two entry kernels, no spilled VGPR, no scratch; the herd kernel asks for no LDS.  The test build's hook BSGS_TEST_CORRUPT_KANGAROO is in bsgs_mi355x_test
only, and the library exports the two calls."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["kangaroo_verify_kernel(VerifyArgs)", "kangaroo_verify_points_kernel(VerifyArgs)"]


def test_kangaroo_verify_kernels_do_not_spill():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    rows = {r["kernel"]: r for r in spill_report.report(tus=["kangaroo_verify"])}
    assert sorted(rows) == KERNELS, sorted(rows)
    for name in KERNELS:
        r = rows[name]
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, r
    assert rows[KERNELS[0]]["lds_bytes_per_block"] == 0


def test_the_hook_is_in_the_test_host_only():
    import pybsgs
    build = os.path.dirname(pybsgs.LIB_PATH)
    if not os.path.exists(os.path.join(build, "bsgs_mi355x")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    ship, test = open(os.path.join(build, "bsgs_mi355x"), "rb").read(), open(os.path.join(build, "bsgs_mi355x_test"), "rb").read()
    assert b"BSGS_TEST_CORRUPT_KANGAROO" not in ship and b"BSGS_TEST_CORRUPT_KANGAROO" in test
    out = subprocess.run(["nm", "-D", "--defined-only", pybsgs.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"bsgs_kangaroo_verify", "bsgs_kangaroo_verify_points"} <= exported
