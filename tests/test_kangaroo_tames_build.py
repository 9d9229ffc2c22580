"""CPU: the unit of the tame table (csrc/kangaroo_tames.hip), from the compiler's own remarks where it is built (cross-compilation, no GPU): exactly the
two match kernels (the plain one checked here, the keyed one in test_kangaroo_tames_sym_build.py), no spilled register, no scratch, no LDS, at least four
waves per SIMD; the library exports the three calls and the walk's unit still holds the kernels it held."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "kangaroo_tames_match_kernel(TamesArgs)"


def test_match_kernel_budget():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    rows = {r["kernel"]: r for r in spill_report.report(tus=["kangaroo_tames"])}
    assert sorted(rows) == sorted([KERNEL, "kangaroo_tames_match_keys_kernel(TamesArgs)"]), sorted(rows)
    r = rows[KERNEL]
    print(r)
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, r
    assert r["lds_bytes_per_block"] == 0 and r["waves_per_simd"] >= 4, r


def test_the_library_exports_the_calls():
    import pybsgs
    out = subprocess.run(["nm", "-D", "--defined-only", pybsgs.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"bsgs_kangaroo_tames_image", "bsgs_kangaroo_tames_install", "bsgs_kangaroo_run_tames"} <= exported
    assert {"bsgs_kangaroo_tames_image", "bsgs_kangaroo_tames_install", "bsgs_kangaroo_run_tames"} <= set(pybsgs.NATIVE_SYMBOLS)
