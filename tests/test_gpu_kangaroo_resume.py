"""GPU: bsgs_mi355x -kangaroo with herds seeded on the GPU, the work file kangaroo.work, -ksteps and -wl (host_kangaroo_run.cpp, host_kangaroo_work.cpp), through the
command line.  One host process at a time, each under its own time limit."""
import math
import os
import re
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_workfile as WF
from pybsgs.ecpy import P as FIELD_P, add, mul, neg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


def run_host(args, cwd, timeout=240):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([EXE, "-kangaroo", "-dir", str(cwd)] + args, capture_output=True, text=True, timeout=timeout)


def job(key, lo, bits):
    return ["-pb", compressed(mul(key)), "-pk", "%x" % lo, "-pke", "%x" % (lo + (1 << bits) - 1), "-d", "0"]


def stopped_steps(out):
    m = re.search(r"Kangaroo: stopped after (\d+) steps \(-ksteps\)", out)
    assert m, out[-2000:]
    return int(m.group(1))


def check_states(states, Q):
    """every state lies on the curve and stands where its offset says: d G (tame) or Q + d G (wild) -- point and offset together, after any number of steps"""
    for x, y, d, fl in states:
        assert fl in (0, K.WILD)
        assert (y * y - x * x * x - 7) % FIELD_P == 0
        assert (x, y) == K.start(Q, K.signed128(d), bool(fl & K.WILD))


def test_gpu_and_host_seeding_give_the_same_herd(tmp_path):
    lo, bits = 0x5 << 70, 64
    key = lo + 0x0123456789ABCDEF
    Q = add(mul(key), neg(mul(lo)))
    files = {}
    for name, extra in (("gpu", []), ("host", ["-kcpuseed"])):
        d = tmp_path / name
        d.mkdir()
        r = run_host(job(key, lo, bits) + ["-kseed", "0x5EED", "-kn", "16384", "-dp", "32", "-ksteps", "1"] + extra, d)
        assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-1000:]
        assert ("[startup] herds (GPU)" in r.stdout) == (name == "gpu") and ("[startup] herds (host)" in r.stdout) == (name == "host")
        files[name] = WF.parse((d / "kangaroo.work").read_bytes())
        assert not (d / "kangaroo.temp").exists()
    g, h = files["gpu"], files["host"]
    assert g["engines"] == 1 and g["herd"] == 16384 and g["dp"] == 32 and g["seed"] == 0x5EED
    assert g["herd_bytes"] == h["herd_bytes"]
    assert (g["steps"], g["rng"], g["fingerprint"], g["table"], g["reseed"]) == (h["steps"], h["rng"], h["fingerprint"], 0, [[]])
    assert g["steps"] == stopped_steps(r.stdout) and g["steps"] % 16384 == 0 and g["steps"] > 0
    herd = g["herds"][0]
    assert sum(1 for s in herd if s[3] & K.WILD) == 8192 and all(s[3] == K.WILD for s in herd[8192:])
    check_states(herd[::256], Q)                                      # 64 of them


def test_resume_is_exact(tmp_path):
    lo, bits = 0x9 << 80, 72
    W = 1 << bits
    key = lo + 0x5DEECE66D12345678A % W
    Q = add(mul(key), neg(mul(lo)))
    kn, seed = 16384, 0xC0FFEE
    base = job(key, lo, bits) + ["-kn", str(kn), "-dp", "32"]
    ra = run_host(base + ["-kseed", hex(seed), "-ksteps", "1"], tmp_path)
    assert ra.returncode == 3, ra.stdout[-2000:] + ra.stderr[-1000:]
    work = tmp_path / "kangaroo.work"
    A = WF.parse(work.read_bytes())
    assert A["steps"] == stopped_steps(ra.stdout)
    # the plan and the seed come from the file: the resumed run names neither
    rb = run_host(job(key, lo, bits) + ["-wl", str(work), "-ksteps", str(A["steps"] + 1)], tmp_path)
    assert rb.returncode == 3, rb.stdout[-2000:] + rb.stderr[-1000:]
    B = WF.parse(work.read_bytes())
    assert "Resumed: %d steps, 0 DPs" % A["steps"] in rb.stdout
    assert B["steps"] == stopped_steps(rb.stdout) and B["steps"] > A["steps"] and (B["steps"] - A["steps"]) % kn == 0
    assert re.search(r"Job time [0-9.]+s, " + re.escape("%.3e kangaroo steps" % B["steps"]), rb.stdout), rb.stdout[-1500:]
    assert B["elapsed"] > A["elapsed"] > 0
    for k in ("engines", "herd", "dp", "per_thread", "seed", "fingerprint", "rng"):      # (-dp 32: nothing was re-seeded, the stream stands still)
        assert A[k] == B[k], k
    assert A["table"] == B["table"] == 0 and A["reseed"] == B["reseed"] == [[]]
    # the jump table again, from the seed and the printed plan, as the host derives it
    m = re.search(r"Kangaroo: 1 engine\(s\) x (\d+) kangaroos \((\d+) per thread\), -dp 32, (\d+) steps per launch, -kseed 0x([0-9a-f]+)", rb.stdout)
    assert m and int(m.group(1)) == kn and int(m.group(4), 16) == seed, rb.stdout[:1500]
    mean = max(1.0, min(2.0 ** 62, kn * math.sqrt(float(W)) / 4.0))
    scalars, jumps = K.jump_table(K.Stream(seed), mean)
    per_kangaroo = (B["steps"] - A["steps"]) // kn
    assert per_kangaroo % int(m.group(3)) == 0
    sample = list(range(5, kn, kn // 16))[:16]
    check_states([A["herds"][0][i] for i in sample], Q)
    walked, recs = K.walk([A["herds"][0][i] for i in sample], jumps, scalars, per_kangaroo, 32)
    assert not recs
    assert [B["herds"][0][i] for i in sample] == walked


def test_resume_finds_the_key(tmp_path):
    bits = 56
    lo = 0x3 << 100 | (0x5A << bits)
    key = lo + (1 << bits) // 3
    used = None
    for seed in (0x101, 0x202, 0x303):          # on the MI355X this test was written on, 0x101 stops at its budget before the key: it is the one used
        d = tmp_path / ("seed%x" % seed)
        d.mkdir()
        plan = run_host(job(key, lo, bits) + ["-kseed", hex(seed), "-ksteps", "1"], d)
        assert plan.returncode in (0, 3), plan.stdout[-2000:] + plan.stderr[-1000:]
        expected = 2.0 ** float(re.search(r"Expected steps: 2\^([0-9.]+)", plan.stdout).group(1))
        (d / "kangaroo.work").unlink(missing_ok=True)
        r1 = run_host(job(key, lo, bits) + ["-kseed", hex(seed), "-ksteps", str(int(expected / 3))], d)
        if r1.returncode == 0:
            continue                             # found before the budget: the next seed
        assert r1.returncode == 3, r1.stdout[-2000:] + r1.stderr[-1000:]
        used = seed
        break
    assert used is not None, "all three seeds found the key within a third of the expected steps"
    print("seed used: 0x%x" % used)
    work = d / "kangaroo.work"
    steps1 = stopped_steps(r1.stdout)
    in_table = int(re.search(r"\((\d+) in the table", r1.stdout).group(1))
    saved = WF.parse(work.read_bytes(), states=False)
    assert (saved["steps"], saved["table"]) == (steps1, in_table) and in_table > 0
    assert not os.path.exists(d / "win.txt") or os.path.getsize(d / "win.txt") == 0
    r2 = run_host(job(key, lo, bits) + ["-wl", str(work)], d)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-1000:]
    assert "Resumed: %d steps, %d DPs" % (steps1, in_table) in r2.stdout
    lines = (d / "win.txt").read_bytes().decode().split("\r\n")
    assert lines[0] == "KEY[1]: 0x%064x" % key and lines[1] == " " * 3 + "Pub: " + compressed(mul(key))
    assert not work.exists() and not (d / "kangaroo.temp").exists()
    total = float(re.search(r"Job time [0-9.]+s, ([0-9.e+]+) kangaroo steps", r2.stdout).group(1))
    assert total > steps1


def test_resume_with_other_settings_is_refused(tmp_path):
    lo, bits = 0x7 << 66, 60
    key = lo + 0xABCDEF0123456
    r = run_host(job(key, lo, bits) + ["-kseed", "9", "-kn", "16384", "-dp", "32", "-ksteps", "1"], tmp_path)
    assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-1000:]
    work = tmp_path / "kangaroo.work"
    before = work.read_bytes()
    good = job(key, lo, bits)
    other_pb = ["-pb", compressed(mul(key + 1))] + good[2:]
    other_pke = good[:4] + ["-pke", "%x" % (lo + (1 << bits))] + good[6:]
    two_engines = good[:6] + ["-d", "0,0"]
    for args in (other_pb, other_pke, two_engines, good + ["-dp", "31"], good + ["-kseed", "10"]):
        r = run_host(args + ["-wl", str(work)], tmp_path, timeout=60)
        assert r.returncode not in (0, 3) and "Recovery file was made with other settings" in r.stderr, (args, r.stdout[-800:], r.stderr[-400:])
        assert work.read_bytes() == before
