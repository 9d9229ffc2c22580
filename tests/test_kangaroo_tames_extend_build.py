"""CPU: the unit of the load and the sorted read of a growing tame table (csrc/kangaroo_tames_extend.hip), from the compiler's own remarks where it is built
(cross-compilation, no GPU): exactly its six kernels, each with the registers it was written to, no spilled register, no scratch, no AGPRs, eight waves per
SIMD, LDS only where the sort counts and ranks; the library exports the two calls and links nothing but the HIP runtime; the header carries their contract; and
the unit of the insert and the harvest still holds its two kernels alone."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"bsgs_kangaroo_tames_gen_load", "bsgs_kangaroo_tames_gen_read_sorted"}
# kernel -> (VGPRs, SGPRs, LDS bytes per block) as hipcc -O3 --offload-arch=gfx950 reports them
KERNELS = {
    "kangaroo_tames_load_kernel(TamesLoadArgs)": (18, 36, 0),
    "kangaroo_tames_sort_harvest_kernel(TamesSortHarvestArgs)": (26, 38, 0),
    "kangaroo_tames_sort_hist_kernel(TamesSortArgs)": (8, 22, 1024),
    "kangaroo_tames_sort_scan_kernel(TamesSortArgs)": (21, 36, 16),
    "kangaroo_tames_sort_scatter_kernel(TamesSortArgs)": (62, 38, 5136),
    "kangaroo_tames_sort_gather_kernel(TamesSortGatherArgs)": (12, 22, 0),
}


def report(tu):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    return {r["kernel"]: r for r in spill_report.report(tus=[tu])}


def test_the_unit_holds_its_six_kernels_within_budget():
    rows = report("kangaroo_tames_extend")
    assert sorted(rows) == sorted(KERNELS), sorted(rows)
    for name, (vgprs, sgprs, lds) in KERNELS.items():
        r = rows[name]
        print(r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, r
        assert (r["vgprs"], r["sgprs"], r["lds_bytes_per_block"], r["waves_per_simd"]) == (vgprs, sgprs, lds, 8), r


def test_the_unit_of_the_insert_is_as_it_was():
    rows = report("kangaroo_tames_gen")
    assert sorted(rows) == sorted(["kangaroo_tames_gen_insert_kernel(TamesGenArgs)", "kangaroo_tames_gen_harvest_kernel(TamesGenHarvestArgs)"]), sorted(rows)
    assert rows["kangaroo_tames_gen_insert_kernel(TamesGenArgs)"]["vgprs"] == 32 and rows["kangaroo_tames_gen_harvest_kernel(TamesGenHarvestArgs)"]["vgprs"] == 22


def test_the_library_exports_the_calls_and_links_the_hip_runtime_alone():
    import pybsgs
    out = subprocess.run(["nm", "-D", "--defined-only", pybsgs.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert CALLS <= exported, CALLS - exported
    assert CALLS <= set(pybsgs.NATIVE_SYMBOLS)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", subprocess.run(["readelf", "-d", pybsgs.LIB_PATH], capture_output=True, text=True).stdout)
    assert any(n.startswith("libamdhip64") for n in needed), needed
    assert not [n for n in needed if re.search(r"rocprim|hipcub|rocthrust|rocrand|rocblas", n)], needed
    gpu_libs = [n for n in needed if not re.match(r"lib(amdhip64|stdc\+\+|m|gcc_s|c|dl|pthread|rt)\.so", n) and not n.startswith("ld-linux")]
    assert gpu_libs == [], gpu_libs


def test_the_header_carries_the_contract():
    with open(os.path.join(ROOT, "include", "bsgs_hip.h")) as f:
        text = f.read()
    section = text[text.index("Kangaroo, tame table grown on the device"):]
    for call in CALLS:
        assert "int %s(bsgs_dev *dev" % call in section, call
    assert "#define BSGS_KANGAROO_TAMES_LOAD_CHUNK (1u << 20)" in section and "#define BSGS_KANGAROO_TAMES_SORT_TILE 2048u" in section
    assert "tests/kangaroo_tames_extend_model.py" in section and "*n_stored + *n_duplicate + *n_zero + *n_full = n" in section
    import kangaroo_tames_extend_model as XM
    assert XM.LOAD_CHUNK == 1 << 20 and XM.SORT_TILE == 2048


def test_the_source_uses_no_sort_library():
    with open(os.path.join(ROOT, "bsgs-cuda_amd", "csrc", "kangaroo_tames_extend.hip")) as f:
        src = f.read()
    assert not re.search(r"rocprim|hipcub|thrust|#include <hip/hip_cooperative", src)
    assert src.count("__global__") == len(KERNELS)
