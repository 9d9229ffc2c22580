"""Register budget of the two probe loops of the quad-chain tile kernels (cross-compiled for gfx950, no GPU).  BSGS_TILES_PER_BLOCK is a wave-uniform launch
argument of ONE instantiation, so the one-tile loop and the pair loop (tile_pair_walk) share the kernel's register allocation: neither may spill a VGPR, and the
scalars of the loops stay in SGPRs -- lane moves (v_readlane / v_writelane: an SGPR parked in a VGPR lane) inside a loop are counted per giant step by
tools/isa_budget.py.  The headline <2> pair loop has none; the budgets below are what the shared allocation gives today, so that a change that
moves more scalars into the loops fails here rather than in a benchmark."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel: (max lane moves per giant step in the one-tile loop, in the pair loop)
BUDGET = {"_Z18giant_pair2_kernelILi2ELb0ELb1EEv8TileArgs": (0.125, 0.0), "_Z18giant_pair2_kernelILi4ELb0ELb1EEv8TileArgs": (0.625, 0.125)}


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_both_probe_loops_keep_their_scalars(tmp_path, kernel):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    out = tmp_path / "isa.json"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "isa_budget.py"), str(out)], env=dict(os.environ, ISA_KERNEL=kernel),
                          stdout=subprocess.DEVNULL)
    r = json.loads(out.read_text())
    one, pair = r["probe_loop_per_giant_step"], r["pair_walk_loop_per_giant_step"]
    assert r["vgprs"] <= 128
    assert one["lane_moves"] <= BUDGET[kernel][0] + 1e-9, one
    assert pair["lane_moves"] <= BUDGET[kernel][1] + 1e-9, pair
    # the pair loop loads each giant once for both tiles: fewer vector-memory instructions per giant step than the one-tile loop
    assert pair["vmem"] < one["vmem"] and pair["smem"] > 0
