"""bench.py without and with --full: a plain run carries the headline and its set-up checks only; --full adds the legs after the timed region (idle power,
sustained region, other quirk mode, roofline denominators) -- and both time the same launches, so they find the same hits."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_other_legs(tmp_path):
    common = ["--w", "26", "--htsz", "25", "--tiles-per-launch", "48", "--steps", "2", "--warmup", "1", "--warmup-s", "0"]
    plain_hits, full_hits = str(tmp_path / "plain.json"), str(tmp_path / "full.json")
    a = _bench(common + ["--dump-hits", plain_hits, "--dump-outputs", str(tmp_path / "plain")])
    b = _bench(common + ["--full", "--sustain-s", "1", "--no-cpu-baseline", "--no-pmc", "--no-solve", "--dump-hits", full_hits, "--dump-outputs", str(tmp_path / "full")])
    for d in (a, b):
        assert d["metric"] == "giant-steps/s" and d["value"] > 1e9 and d["unit"] == "giant-steps/s" and d["higher_is_better"] is True
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"].startswith("u32x8")
        assert d["table_checksum_equal"] is True and d["replica_hits_equal"] is True
        assert d["verification"]["structural"]["census_total"] == 1 << 26 and d["verification"]["structural"]["sampled_kG_found"] == "1024/1024"
        assert d["roofline"]["kernel"].startswith("giant_pair2_kernel<") and 0 < d["roofline"]["frac"] < 1
        assert "cpu_baseline" not in d and "measured_solve" not in d and d["roofline"]["traffic_measured_this_run"] is None
    # plain: nothing after the timed region but the line
    assert a["full"] is False
    assert a["sustained"] is None and a["value_sustained"] is None and a["refquirks"] is None
    assert a["roofline"]["probe_phase"] is None and a["roofline"]["random_read_64B_peak_GBps"] is None and a["roofline"]["frac_of_random_read_peak"] is None
    assert a["alu"]["modmul_G_per_s"] is None and a["nJ_per_giant_step"] is None
    # --full: the legs are there, as before the option existed
    assert b["full"] is True
    assert b["sustained"]["launches_per_gpu"] >= 2 and b["value_sustained"] > 1e9
    assert b["refquirks"]["value"] > 1e9 and b["refquirks"]["mode_timed_here"] == "BSGS_FLAG_REFERENCE_QUIRKS"
    assert b["roofline"]["probe_phase"]["ms_phase3_probes"] > 0 and b["roofline"]["random_read_64B_peak_GBps"] > 0 and b["alu"]["modmul_G_per_s"] > 0
    # the same timed launches, the same hits
    with open(plain_hits) as f:
        ha = json.load(f)
    with open(full_hits) as f:
        hb = json.load(f)
    assert ha["per_rank_launches"] == hb["per_rank_launches"] == [[1, 2]]
    assert ha["hits"] == hb["hits"]
    import numpy as np
    assert np.array_equal(np.load(str(tmp_path / "plain" / "hits.npy")), np.load(str(tmp_path / "full" / "hits.npy")))
