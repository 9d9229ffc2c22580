"""CPU: the unit of the distinguished-point table divided over engines (csrc/kangaroo_dptable_shard.hip), from the compiler's own remarks where it is built
(cross-compilation, no GPU): exactly its two kernels, the insert that counts and the scatter, with the register counts DESIGN.md 10 quotes, no spilled
register, no scratch, no AGPRs, no LDS, eight waves per SIMD; the units it stands beside report exactly their kernels; the library exports the three calls,
pybsgs binds them and the header carries the section."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSERT, SCATTER = "kangaroo_dptable_shard_insert_kernel(DptShardArgs)", "kangaroo_dptable_shard_scatter_kernel(DptShardArgs)"
CALLS = {"bsgs_kangaroo_dptable_begin_shard", "bsgs_kangaroo_run_dptable_shard", "bsgs_kangaroo_dptable_insert_shard"}
UNKEYED = ["kangaroo_dptable_insert_kernel(DptArgs)", "kangaroo_dptable_resolve_kernel(DptArgs)", "kangaroo_dptable_load_kernel(DptLoadArgs)",
           "kangaroo_dptable_harvest_kernel(DptHarvestArgs)"]
KEYED = ["kangaroo_dptable_insert_keys_kernel(DptKeysArgs)"]


def report(tu):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_report
    return {r["kernel"]: r for r in spill_report.report(tus=[tu])}


def test_the_unit_holds_its_kernels_within_budget():
    rows = report("kangaroo_dptable_shard")
    assert sorted(rows) == sorted([INSERT, SCATTER]), sorted(rows)
    for r in rows.values():
        print(r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, r
        assert r["lds_bytes_per_block"] == 0 and r["waves_per_simd"] == 8, r
    # the unsharded insert takes 40 VGPRs and 47 SGPRs; the sixteen counts a wave keeps per destination, and the scatter's sixteen places, live in SGPRs
    assert (rows[INSERT]["vgprs"], rows[INSERT]["sgprs"]) == (44, 74), rows[INSERT]
    assert (rows[SCATTER]["vgprs"], rows[SCATTER]["sgprs"]) == (40, 64), rows[SCATTER]


def test_the_units_beside_it_keep_exactly_their_kernels():
    rows = report("kangaroo_dptable")
    assert sorted(rows) == sorted(UNKEYED), sorted(rows)
    assert (rows[UNKEYED[0]]["vgprs"], rows[UNKEYED[0]]["sgprs"]) == (40, 47), rows[UNKEYED[0]]
    rows = report("kangaroo_dptable_keys")
    assert sorted(rows) == sorted(KEYED), sorted(rows)
    assert (rows[KEYED[0]]["vgprs"], rows[KEYED[0]]["sgprs"]) == (40, 49), rows[KEYED[0]]


def test_the_library_exports_the_calls():
    import pybsgs
    out = subprocess.run(["nm", "-D", "--defined-only", pybsgs.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert CALLS <= exported, CALLS - exported
    assert CALLS <= set(pybsgs.NATIVE_SYMBOLS)
    for call in CALLS:
        assert hasattr(pybsgs.Device, call[len("bsgs_"):]), call
    assert pybsgs.KANGAROO_DPT_MAX_SHARDS == 16


def test_the_header_carries_the_section():
    with open(os.path.join(ROOT, "include", "bsgs_hip.h")) as f:
        text = f.read()
    assert "Kangaroo, distinguished-point table divided over engines" in text
    assert "#define BSGS_KANGAROO_DPT_MAX_SHARDS 16u" in text
    assert "shard(tag) = ((tag >> 48) * E) >> 16" in text
    for call in CALLS:
        assert "int %s(bsgs_dev *dev" % call in text, call
