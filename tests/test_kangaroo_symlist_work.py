"""CPU: kangaroo.work version 4 (a list of keys searched with -kwalk sym) -- the table, the solved keys and the signed links through a file in the middle of
a scripted stream, the file read back by tests/kangaroo_symlist_workfile.py, the versions refused by each other's modes, damaged files and a fingerprint that
differs in one key."""
import os
import subprocess

import pytest

import kangaroo_symlist_workfile as WF
import test_kangaroo_symlist_model as T
from pybsgs.ecpy import mul

HOST = T.HOST
A, W, PUBS, KP, KPP = T.A, T.W, T.PUBS, T.KP, T.KPP
RANGE = ["%x" % A, "%x" % (A + W - 1)]
PUBLIST = ",".join(T.compressed(p) for p in PUBS)


def selftest(name, args, env=None):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(T.ROOT, "bsgs-cuda_amd"), "-s"])
    return subprocess.run([HOST, "-selftest", name] + args, capture_output=True, text=True, timeout=60, env=dict(os.environ, **(env or {})))


def recs(records):
    return ["%s,%x,%x,%d" % (t, x, d & T.K.M128, kid) for t, x, d, kid in records]


# links open at the split (2, 3, 4), keys solved at the split (4, 6), a cycle counted before it
@pytest.mark.parametrize("name, split", [("link_then_second", 2), ("link_minus_then_first", 3), ("chain", 4), ("false_link", 2), ("solved_acts_as_tame", 4),
                                         ("solved_acts_as_tame", 6), ("same_type", 8), ("same_key_plus", 1), ("tame_wild_minus", 0)])
def test_round_trip_mid_stream(name, split):
    r = T.streams()[name]
    out = selftest("kangaroo-symlist-roundtrip", RANGE + [PUBLIST, str(split)] + recs(r))
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:-1] == T.model_lines(PUBS, r)[0]


@pytest.fixture
def v4(tmp_path):
    """a version-4 file with one solved key, two open links (eps = +1 and -1) and three entries, one of a NEG kangaroo"""
    r = T.streams()["chain"][:4] + [T.tame(0x5000, 3), T.wild(3, 1, 0x5000 - KPP[3], 4), ("C", 5, 5, 9)]
    path = str(tmp_path / "kangaroo.work")
    out = selftest("kangaroo-symlist-roundtrip", RANGE + [PUBLIST, str(len(r))] + recs(r), {"BSGS_SELFTEST_WORK": path})
    assert out.returncode == 0, out.stderr
    return path


def test_file_contents_and_header(v4):
    w = WF.read(v4)
    assert w["keys"] == [None, None, None, A + KP[3]]
    assert w["links"] == [(0, 1, T.E0, 1, 1, T.E1), (2, -1, T.F2M, 1, 1, T.F1)] and (w["links_kept"], w["links_resolved"]) == (2, 0)
    assert sorted((e[3], e[4]) for e in w["entries"]) == [(0, False), (1, False), (3, True)] and w["engines"] == 0
    assert (w["jumps"], w["jumpscale"], w["cycles"], w["reseeds"]) == (1024, 1.0, 1, 3)
    out = selftest("kangaroo-work", [v4])
    assert out.returncode == 0 and out.stdout.split("\n")[:7] == ["version 4", "jumps 1024", "jumpscale 1", "cycles 1", "keys 4", "solved 1", "links 2"]
    out = selftest("kangaroo-work", [v4] + RANGE + [PUBLIST])
    assert out.returncode == 0 and "fingerprint-check ok" in out.stdout
    other = ",".join(T.compressed(p) for p in PUBS[:2] + [mul(A + 5)] + PUBS[3:])
    out = selftest("kangaroo-work", [v4] + RANGE + [other])
    assert out.returncode == 1 and "other settings" in out.stderr


def test_damaged_files_are_refused(v4, tmp_path):
    b = open(v4, "rb").read()
    link0 = 168 + 4 + 3 + 33 + 24                                  # header, L, three open keys, one solved key, the link counters
    cases = (("short", b[:-10]), ("long", b + b"\0"), ("cut_in_keys", b[:174]), ("status", b[:172] + b"\x02" + b[173:]), ("zero_word", b[:148] + b"\x01" + b[149:]),
             ("link_sign", b[:link0 + 8] + b"\x02\0\0\0" + b[link0 + 12:]), ("link_key", b[:link0] + b"\x09\0\0\0" + b[link0 + 4:]))
    for name, data in cases:
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        out = selftest("kangaroo-work", [p])
        assert out.returncode == 1, name
    assert b[link0:link0 + 16] == (0).to_bytes(4, "little") + (1).to_bytes(4, "little") + (1).to_bytes(4, "little") * 2      # the cases above hit what they name


def test_each_version_is_refused_by_the_other_modes(v4, tmp_path):
    keys = tmp_path / "keys.txt"
    keys.write_text("\n".join(T.compressed(p) for p in PUBS) + "\n")
    rng = ["-pk", RANGE[0], "-pke", RANGE[1], "-dir", str(tmp_path)]
    one = T.compressed(PUBS[0])
    # a version-4 file: one key plain and -ksym, the plain list search
    for extra, reads in ((["-pb", one], 1), (["-pb", one, "-ksym"], 2), (["-pb", one, "-kwalk", "sym"], 2), (["-infile", str(keys)], 3)):
        r = subprocess.run([HOST, "-kangaroo", "-wl", v4] + extra + rng, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and ("work file version 4, this host reads version %d" % reads) in r.stderr, r.stderr
    # versions 1, 2 and 3 at the symmetric list search
    t = T.tame(0x5000, 1)
    for st, ver, pubs in (("kangaroo-table-roundtrip", 1, one), ("kangaroo-sym-roundtrip", 2, one), ("kangaroo-multi-roundtrip", 3, PUBLIST)):
        p = str(tmp_path / ("v%d.work" % ver))
        out = selftest(st, RANGE + [pubs, "1"] + recs([t]), {"BSGS_SELFTEST_WORK": p})
        assert out.returncode == 0, out.stderr
        r = subprocess.run([HOST, "-kangaroo", "-infile", str(keys), "-kwalk", "sym", "-wl", p] + rng, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and ("work file version %d, this host reads version 4" % ver) in r.stderr, r.stderr
    # a version-4 file of another list, and one of other jump settings
    r = subprocess.run([HOST, "-kangaroo", "-infile", str(keys), "-kwalk", "sym", "-kjumps", "512", "-wl", v4] + rng, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "other settings" in r.stderr
    keys.write_text("\n".join(T.compressed(p) for p in PUBS[:3] + [mul(A + 9)]) + "\n")
    r = subprocess.run([HOST, "-kangaroo", "-infile", str(keys), "-kwalk", "sym", "-wl", v4] + rng, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "other settings" in r.stderr
