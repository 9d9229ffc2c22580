"""CPU: kangaroo.work version 3 (a list of keys) -- the table, the solved keys and the links through a file in the middle of a scripted stream, the file read
back by tests/kangaroo_multi_workfile.py, each of the three versions refused by the other modes, damaged files and a fingerprint that differs in one key."""
import os
import subprocess

import pytest

import kangaroo_multi_workfile as WF
import test_kangaroo_multi_model as T
from pybsgs.ecpy import mul

HOST = T.HOST
A, W, PUBS, KP = T.A, T.W, T.PUBS, T.KP
RANGE = ["%x" % A, "%x" % (A + W - 1)]
PUBLIST = ",".join(T.compressed(p) for p in PUBS)


def selftest(name, args, env=None):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(T.ROOT, "bsgs-cuda_amd"), "-s"])
    return subprocess.run([HOST, "-selftest", name] + args, capture_output=True, text=True, timeout=60, env=dict(os.environ, **(env or {})))


def recs(records):
    return ["%s,%x,%x,%d" % (t, x, d & T.K.M128, kid) for t, x, d, kid in records]


@pytest.mark.parametrize("name, split", [("link_then_second", 2), ("link_then_first", 3), ("chain", 4), ("false_link", 2), ("solved_acts_as_tame", 4),
                                         ("solved_acts_as_tame", 6), ("same_type", 3), ("tame_wild", 0)])
def test_round_trip_mid_stream(name, split):
    r = T.streams()[name]
    out = selftest("kangaroo-multi-roundtrip", RANGE + [PUBLIST, str(split)] + recs(r))
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:-1] == T.model_lines(PUBS, r)[0]


@pytest.fixture
def v3(tmp_path):
    """a version-3 file with one solved key, one open link and three entries"""
    r = T.streams()["chain"][:4] + [T.tame(0x5000, 3), T.wild(3, 0x5000 - KP[3], 4)]
    path = str(tmp_path / "kangaroo.work")
    out = selftest("kangaroo-multi-roundtrip", RANGE + [PUBLIST, str(len(r))] + recs(r), {"BSGS_SELFTEST_WORK": path})
    assert out.returncode == 0, out.stderr
    return path


def test_file_contents_and_header(v3):
    w = WF.read(v3)
    assert w["keys"] == [None, None, None, A + KP[3]]
    e0 = 0x777
    e1 = KP[0] + e0 - KP[1]
    f1 = -0x4321
    f2 = KP[1] + f1 - KP[2]
    assert w["links"] == [(0, 1, e1 - e0), (2, 1, f1 - f2)] and (w["links_kept"], w["links_resolved"]) == (2, 0)
    assert sorted(e[3] for e in w["entries"]) == [0, 1, 3] and w["engines"] == 0
    out = selftest("kangaroo-work", [v3])
    assert out.returncode == 0 and out.stdout.split("\n")[:4] == ["version 3", "keys 4", "solved 1", "links 2"]
    out = selftest("kangaroo-work", [v3] + RANGE + [PUBLIST])
    assert out.returncode == 0 and "fingerprint-check ok" in out.stdout
    other = ",".join(T.compressed(p) for p in PUBS[:2] + [mul(A + 5)] + PUBS[3:])
    out = selftest("kangaroo-work", [v3] + RANGE + [other])
    assert out.returncode == 1 and "other settings" in out.stderr


def test_damaged_files_are_refused(v3, tmp_path):
    b = open(v3, "rb").read()
    for name, data in (("short", b[:-10]), ("long", b + b"\0"), ("cut_in_keys", b[:150]), ("status", b[:148] + b"\x02" + b[149:])):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        out = selftest("kangaroo-work", [p])
        assert out.returncode == 1, name


def test_each_version_is_refused_by_the_other_modes(v3, tmp_path):
    keys = tmp_path / "keys.txt"
    keys.write_text("\n".join(T.compressed(p) for p in PUBS) + "\n")
    rng = ["-pk", RANGE[0], "-pke", RANGE[1], "-dir", str(tmp_path)]
    one = T.compressed(PUBS[0])
    for extra in ([], ["-ksym"]):
        r = subprocess.run([HOST, "-kangaroo", "-pb", one, "-wl", v3] + rng + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "work file version 3" in r.stderr, r.stderr
    t = T.tame(0x5000, 1)
    for st, ver in (("kangaroo-table-roundtrip", 1), ("kangaroo-sym-roundtrip", 2)):
        p = str(tmp_path / ("v%d.work" % ver))
        out = selftest(st, RANGE + [one, "1"] + recs([t]), {"BSGS_SELFTEST_WORK": p})
        assert out.returncode == 0, out.stderr
        r = subprocess.run([HOST, "-kangaroo", "-infile", str(keys), "-wl", p] + rng, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and ("work file version %d, this host reads version 3" % ver) in r.stderr, r.stderr
    # a version-3 file of another list
    keys.write_text("\n".join(T.compressed(p) for p in PUBS[:3] + [mul(A + 9)]) + "\n")
    r = subprocess.run([HOST, "-kangaroo", "-infile", str(keys), "-wl", v3] + rng, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "other settings" in r.stderr
