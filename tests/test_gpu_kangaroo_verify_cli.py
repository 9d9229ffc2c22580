"""GPU: bsgs_mi355x -kangaroo verifies what it loads and what it saves (host_kangaroo_run.cpp; DESIGN.md 10, "verification"): a work file with one flipped bit in
a herd state or in a table entry is refused by -wl before any step, in each of the three modes, and stays as it is; an untouched file resumes and says what
it checked; -noverify skips it all; the test build's BSGS_TEST_CORRUPT_KANGAROO makes a herd go wrong before a save, which then does not happen.  One host
process at a time, each under its own time limit."""
import os
import re
import struct
import subprocess

import pytest

from pybsgs.ecpy import mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "bsgs-cuda_amd", "build")
EXE, EXE_TEST = os.path.join(BUILD, "bsgs_mi355x"), os.path.join(BUILD, "bsgs_mi355x_test")
LO, BITS = 0x5 << 70, 60
KEYS = [LO + 0x0123456789ABCDE, LO + 0xFEDCBA987654321 % (1 << BITS), LO + 12345, LO + (1 << BITS) - 77]
KN = 16384
MODES = ["plain", "sym", "list"]


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


def run_host(args, cwd, exe=EXE, env=None, timeout=120):
    assert os.path.exists(exe), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([exe, "-kangaroo", "-dir", str(cwd), "-pk", "%x" % LO, "-pke", "%x" % (LO + (1 << BITS) - 1), "-d", "0"] + args, capture_output=True, text=True,
                          timeout=timeout, env=dict(os.environ, **(env or {})))


def mode_args(mode, cwd):
    if mode == "list":
        keys = os.path.join(str(cwd), "keys.txt")
        with open(keys, "w") as f:
            f.write("\n".join(compressed(mul(k)) for k in KEYS) + "\n")
        return ["-infile", keys]
    return ["-pb", compressed(mul(KEYS[0]))] + (["-ksym"] if mode == "sym" else [])


def sections(data):
    """(steps, table entries, offset of the table, offset of engine 0's herd) of a one-engine work file of any of the three versions"""
    assert data[:8] == b"KANGWORK"
    version, engines, herd = struct.unpack_from("<IIQ", data, 8)
    assert engines == 1 and herd == KN
    steps, table = struct.unpack_from("<Q", data, 48)[0], struct.unpack_from("<Q", data, 96)[0]
    pos = 168 if version == 2 else 144
    if version == 3:                                                 # the key list's state: a status byte per key and the key when solved, counters, links
        (n_keys,) = struct.unpack_from("<I", data, pos)
        pos += 4
        for _ in range(n_keys):
            pos += 1 + 32 * data[pos]
        pos += 24 + 24 * struct.unpack_from("<Q", data, pos + 16)[0]
    herd_at = pos + 32 * table
    (n_reseed,) = struct.unpack_from("<I", data, herd_at + 96 * KN)
    assert herd_at + 96 * KN + 4 + 4 * n_reseed == len(data)
    return steps, table, pos, herd_at


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """per mode, made once and never changed: (the arguments that name the job, the bytes of a work file after one launch at dp 4)"""
    made = {}

    def get(mode):
        if mode not in made:
            d = tmp_path_factory.mktemp("made_" + mode)
            args = mode_args(mode, d)
            r = run_host(args + ["-kseed", "0x5EED", "-kn", str(KN), "-dp", "4", "-ksteps", "1"], d)
            assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-1000:]
            assert "[verify] herd 0: %d kangaroos at their offsets" % KN in r.stdout          # the last save went through the check
            data = (d / "kangaroo.work").read_bytes()
            steps, table, _, _ = sections(data)
            assert table > 0 and steps > 0
            made[mode] = (args, data)
        return made[mode]
    return get


def resume(args, data, cwd, extra=(), change=None):
    """-wl on a copy of the file with `change` (offset, xor) applied -> (the finished process, the file's bytes before, the path)"""
    if change:
        data = data[:change[0]] + bytes([data[change[0]] ^ change[1]]) + data[change[0] + 1:]
    work = os.path.join(str(cwd), "saved.work")
    with open(work, "wb") as f:
        f.write(data)
    steps = sections(data)[0]
    r = run_host(args + ["-wl", work, "-ksteps", str(steps + 1)] + list(extra), cwd)
    return r, data, work


@pytest.mark.parametrize("mode", MODES)
def test_a_damaged_herd_state_is_refused(saved, tmp_path, mode):
    args, data = saved(mode)
    herd = sections(data)[3]
    r, before, work = resume(args, data, tmp_path, change=(herd + 96 * 777 + 64 + 5, 0x10))      # one bit of d of kangaroo 777
    assert r.returncode not in (0, 3), r.stdout[-1500:] + r.stderr[-800:]
    assert "Recovery file is damaged: kangaroo 777 of engine 0 does not stand at its offset" in r.stderr, r.stderr[-800:]
    assert open(work, "rb").read() == before and not os.path.exists(os.path.join(str(tmp_path), "kangaroo.work"))
    assert "Job time" not in r.stdout                                # the run ended before its first step


@pytest.mark.parametrize("mode", MODES)
def test_a_damaged_table_entry_is_refused(saved, tmp_path, mode):
    args, data = saved(mode)
    table = sections(data)[2]
    r, before, work = resume(args, data, tmp_path, change=(table + 32 * 3 + 8 + 2, 0x04))        # one bit of d of table entry 3
    assert r.returncode not in (0, 3), r.stdout[-1500:] + r.stderr[-800:]
    assert "Recovery file is damaged: table entry 3 does not match its offset" in r.stderr, r.stderr[-800:]
    assert "[verify] herd 0" in r.stdout                             # the herd was found in order first
    assert open(work, "rb").read() == before and not os.path.exists(os.path.join(str(tmp_path), "kangaroo.work"))


@pytest.mark.parametrize("mode", MODES)
def test_an_untouched_file_resumes_and_says_what_it_checked(saved, tmp_path, mode):
    args, data = saved(mode)
    steps, table, _, _ = sections(data)
    r, _, _ = resume(args, data, tmp_path)
    assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-1000:]
    assert re.search(r"\[verify\] herd 0: %d kangaroos at their offsets [0-9.]+s\n" % KN, r.stdout), r.stdout[-2000:]
    assert re.search(r"\[verify\] table: %d entries [0-9.]+s\n" % table, r.stdout), r.stdout[-2000:]
    assert r.stdout.count("[verify] herd 0") == 2                    # at -wl and before the last save
    after = (tmp_path / "kangaroo.work").read_bytes()
    assert sections(after)[0] > steps


def test_noverify_takes_the_damaged_file(saved, tmp_path):
    args, data = saved("plain")
    herd = sections(data)[3]
    r, _, _ = resume(args, data, tmp_path, extra=["-noverify"], change=(herd + 96 * 777 + 64 + 5, 0x10))
    assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-1000:]
    assert "[verify]" not in r.stdout and "damaged" not in r.stderr
    assert (tmp_path / "kangaroo.work").exists()


def test_a_herd_that_went_wrong_is_not_saved(tmp_path):
    """the test build flips bit 0 of the offset of kangaroo 4242 after the first launch: the save that -ksteps asks for does not happen; a file that was there stays"""
    args = mode_args("plain", tmp_path) + ["-kseed", "0x5EED", "-kn", str(KN), "-dp", "4", "-ksteps", "1"]
    hook = {"BSGS_TEST_CORRUPT_KANGAROO": "4242"}
    r = run_host(args, tmp_path, exe=EXE_TEST, env=hook)
    assert r.returncode not in (0, 3), r.stdout[-1500:] + r.stderr[-800:]
    assert "herd of engine 0 failed verification at kangaroo 4242: kangaroo.work left as it was" in r.stderr, r.stderr[-800:]
    assert not (tmp_path / "kangaroo.work").exists() and not (tmp_path / "kangaroo.temp").exists()
    (tmp_path / "kangaroo.work").write_bytes(b"an earlier file")
    r = run_host(args, tmp_path, exe=EXE_TEST, env=hook)
    assert r.returncode not in (0, 3) and "failed verification at kangaroo 4242" in r.stderr
    assert (tmp_path / "kangaroo.work").read_bytes() == b"an earlier file"


def test_the_shipped_host_has_no_such_hook(tmp_path):
    args = mode_args("plain", tmp_path) + ["-kseed", "0x5EED", "-kn", str(KN), "-dp", "4", "-ksteps", "1"]
    r = run_host(args, tmp_path, env={"BSGS_TEST_CORRUPT_KANGAROO": "4242"})
    assert r.returncode == 3, r.stdout[-1500:] + r.stderr[-800:]
    assert "TEST HOOK" not in r.stderr and (tmp_path / "kangaroo.work").exists()
