"""GPU: the signal stop of bsgs_mi355x -kangaroo (host_kangaroo_run.cpp): SIGTERM while the engines walk ends the run through the last save --
rc 3, `stopped after N steps (signal)`, a complete kangaroo.work and no kangaroo.temp -- in each mode: plain, -ksym, and -infile with three keys.  The range
is 100 bits wide, so no key is found.  No assertion touches a rate or a time."""
import os
import re
import select
import signal
import subprocess
import time

import pytest

from pybsgs.ecpy import mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
LO, W = 0x9 << 104, 1 << 100
KN = 16384
KEYS = [LO + 0x5DEECE66D12345678A0B1C2D3 % W, LO + W // 3, LO + W - 2]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def read_until(proc, needle, bound):
    """stdout up to and including the first chunk that holds `needle` (the status line ends in no newline: raw reads)"""
    got, deadline = b"", time.monotonic() + bound
    while needle not in got:
        left = deadline - time.monotonic()
        assert left > 0 and select.select([proc.stdout], [], [], left)[0], "no %r within %d s:\n%s" % (needle, bound, got.decode(errors="replace")[-2000:])
        chunk = os.read(proc.stdout.fileno(), 65536)
        assert chunk, "the host ended before %r:\n%s" % (needle, got.decode(errors="replace")[-2000:])
        got += chunk
    return got


def selftest_work(path):
    r = subprocess.run([EXE, "-selftest", "kangaroo-work", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(ln.split(" ", 1) for ln in r.stdout.split("\n") if " " in ln)


@pytest.mark.parametrize("mode", ["plain", "ksym", "infile"])
def test_sigterm_saves_and_exits_3(tmp_path, mode):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    if mode == "infile":
        (tmp_path / "keys.txt").write_text("\n".join(compressed(mul(k)) for k in KEYS) + "\n")
        job = ["-infile", str(tmp_path / "keys.txt")]
    else:
        job = ["-pb", compressed(mul(KEYS[0]))] + (["-ksym"] if mode == "ksym" else [])
    cmd = [EXE, "-kangaroo", "-dir", str(tmp_path), "-pk", "%x" % LO, "-pke", "%x" % (LO + W - 1), "-d", "0", "-kn", str(KN), "-kseed", "0x51671"] + job
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        # the first status line: flushed, and printed after the handlers are installed and the engines have started
        head = read_until(proc, b"steps/s", 60)
        proc.send_signal(signal.SIGTERM)
        rest, err = proc.communicate(timeout=60)
    finally:
        if proc.poll() is None:
            proc.kill()
            proc.communicate()
    out = (head + rest).decode()
    assert proc.returncode == 3, out[-2000:] + err.decode()[-1000:]
    m = re.search(r"Kangaroo: stopped after (\d+) steps \(signal\)", out)
    assert m, out[-2000:]
    steps = int(m.group(1))
    assert steps > 0 and steps % KN == 0
    assert not (tmp_path / "kangaroo.temp").exists()
    h = selftest_work(tmp_path / "kangaroo.work")
    assert (h["steps"], h["engines"], h["herd"]) == (str(steps), "1", str(KN)), h
    assert h.get("version") == {"plain": None, "ksym": "2", "infile": "3"}[mode], h
    if mode == "infile":
        assert h["keys"] == "3" and "3 of 3 keys open" in out, (h, out[-1500:])
