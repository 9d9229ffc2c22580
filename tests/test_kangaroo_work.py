"""CPU: the kangaroo work file (host_kangaroo_work.cpp; layout in DESIGN.md 10).  The host's table of distinguished points goes through a work file at every
split point of scripted record streams and still gives the model's verdicts for the undivided stream; the file's header and table section hold what the model
has at the split; files that are truncated, foreign or made with other settings are refused."""
import os
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_workfile as WF
from pybsgs.ecpy import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
TYPES = {"T": 0, "W": K.WILD, "D": K.DEAD}


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


def streams():
    """(name, a, W, pub, records): records as the host's selftests take them, (type letter, x, d, kangaroo)"""
    a, W = 0x2B << 44, 1 << 28
    kp = 0x9A7B3C1
    pub = mul(a + kp)
    d_w = -(W // 5)
    d_t = kp + d_w                                                   # tame at d_t G meets wild at Q + d_w G
    xt = mul(d_t)[0]
    filler = [("T", mul(1000 + i)[0], 1000 + i, 20 + i) for i in range(3)] + [("W", mul(2000 + i)[0], 2000 + i - kp, 30 + i) for i in range(3)]
    late = filler + [("T", xt, d_t, 1), ("D", mul(7)[0], 7, 21), ("W", xt, d_w, 2)]
    early = [("W", xt, d_w, 2)] + filler + [("T", xt, d_t, 1)]
    mixed = [("T", xt, d_t, 1), ("T", xt, d_t, 1), ("T", xt, d_t + 9, 3), ("W", xt, d_t + 1, 4), ("D", mul(11)[0], 3, 3), ("W", mul(5)[0], 5, 6),
             ("W", mul(5)[0], 5, 8), ("T", mul(5)[0], 5 + W, 9), ("W", mul(5)[0], 5, 6), ("D", mul(5)[0], 5, 6)]
    negd = [("W", mul(31)[0], -(W // 2), 40), ("W", mul(32)[0], -1, 41), ("T", mul(31)[0], kp - (W // 2), 42), ("T", mul(32)[0], W - 1, 43)]
    return [("late", a, W, pub, late), ("early", a, W, pub, early), ("mixed", a, W, pub, mixed), ("negative_offsets", a, W, pub, negd), ("empty", a, W, pub, [])]


def model(a, W, pub, records, upto=None):
    """the model's verdict lines for the stream, and its table after the first `upto` records (all of them: None)"""
    t = K.DPTable(a, W, pub)
    out, at_split = [], None
    for i, (typ, x, d, kid) in enumerate(records):
        if i == upto:
            at_split = (dict(t.map), t.false_matches, t.reseeds)
        v, key = t.add(x, d, kid, TYPES[typ])
        out.append("found %064x" % key if v == "found" else "reseed %d" % kid if v == "reseed" else v)
    if at_split is None:
        at_split = (dict(t.map), t.false_matches, t.reseeds)
    out.append("summary %d %d %d" % (len(t.map), t.false_matches, t.reseeds))
    return out, at_split


def host_args(a, W, pub, records):
    return ["%x" % a, "%x" % (a + W - 1), compressed(pub)], ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in records]


def roundtrip(a, W, pub, records, split, keep=None):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    head, recs = host_args(a, W, pub, records)
    env = dict(os.environ)
    env.pop("BSGS_SELFTEST_WORK", None)
    if keep:
        env["BSGS_SELFTEST_WORK"] = str(keep)
    return subprocess.run([HOST, "-selftest", "kangaroo-table-roundtrip"] + head + [str(split)] + recs, capture_output=True, text=True, timeout=60, env=env)


def work_header(path, extra=()):
    r = subprocess.run([HOST, "-selftest", "kangaroo-work", str(path)] + list(extra), capture_output=True, text=True, timeout=60)
    return r, dict(ln.split(" ", 1) for ln in r.stdout.split("\n") if " " in ln)


@pytest.mark.parametrize("name", [s[0] for s in streams()])
def test_table_round_trip_at_every_split(name):
    _, a, W, pub, recs = next(s for s in streams() if s[0] == name)
    want, _ = model(a, W, pub, recs)
    for split in range(len(recs) + 1):
        r = roundtrip(a, W, pub, recs, split)
        assert r.returncode == 0, (split, r.stderr)
        assert r.stdout.split("\n")[:-1] == want, split
    if name in ("late", "early"):
        assert any(ln.startswith("found ") for ln in want)
    assert roundtrip(a, W, pub, recs, len(recs) + 1).returncode != 0          # a split beyond the stream


@pytest.mark.parametrize("name", ["late", "mixed", "negative_offsets"])
def test_work_file_holds_the_model_state_at_the_split(tmp_path, name):
    _, a, W, pub, recs = next(s for s in streams() if s[0] == name)
    head, _ = host_args(a, W, pub, recs)
    for split in range(len(recs) + 1):
        path = tmp_path / ("split%d.work" % split)
        assert roundtrip(a, W, pub, recs, split, keep=path).returncode == 0
        _, (table, false_matches, reseeds) = model(a, W, pub, recs, upto=split)
        dps = sum(1 for r in recs[:split] if r[0] != "D")
        r, h = work_header(path, head)
        assert r.returncode == 0, r.stderr
        assert (h["steps"], h["dps"], h["table"], h["engines"], h["herd"], h["rng"]) == ("0", str(dps), str(len(table)), "0", "0", "0x0")
        assert "fingerprint-check ok" in r.stdout and len(h["fingerprint"]) == 40
        # the bytes themselves, read as DESIGN.md 10 lays them out
        w = WF.parse(path.read_bytes())
        assert (w["version"], w["engines"], w["herd"], w["steps"], w["dps"], w["table"], w["false_matches"], w["reseeds"]) == \
            (1, 0, 0, 0, dps, len(table), false_matches, reseeds)
        assert w["fingerprint"] == h["fingerprint"]
        assert sorted(w["entries"]) == sorted((k64, d, kid, 1 if wild else 0) for k64, (d, kid, wild) in table.items())


def test_damaged_and_foreign_files_are_refused(tmp_path):
    _, a, W, pub, recs = next(s for s in streams() if s[0] == "late")
    head, _ = host_args(a, W, pub, recs)
    good = tmp_path / "good.work"
    assert roundtrip(a, W, pub, recs, 7, keep=good).returncode == 0
    data = good.read_bytes()
    assert work_header(good, head)[0].returncode == 0
    cases = {"truncated_table": data[:-5], "truncated_header": data[:100], "empty": b"", "wrong_magic": b"KANGWORX" + data[8:], "trailing": data + b"\0",
             "wrong_version": data[:8] + b"\x02\0\0\0" + data[12:], "text": b"1\r\n02aa\r\n1f\r\nabcdef\r\n"}
    for what, blob in cases.items():
        p = tmp_path / (what + ".work")
        p.write_bytes(blob)
        r, _ = work_header(p)
        assert r.returncode != 0 and r.stderr.strip(), what
    # a changed fingerprint byte, and an unchanged file against another range or key: made with other settings
    flipped = tmp_path / "flipped.work"
    flipped.write_bytes(data[:110] + bytes([data[110] ^ 1]) + data[111:])
    r, _ = work_header(flipped, head)
    assert r.returncode != 0 and "other settings" in r.stderr
    for other in ([head[0], "%x" % (a + W), head[2]], [head[0], head[1], compressed(mul(12345))]):
        r, _ = work_header(good, other)
        assert r.returncode != 0 and "other settings" in r.stderr
    # the resume path refuses the same files before it looks for a device, and leaves them in place
    for p in (tmp_path / "wrong_magic.work", tmp_path / "truncated_table.work", flipped, tmp_path / "missing.work"):
        before = p.read_bytes() if p.exists() else None
        r = subprocess.run([HOST, "-kangaroo", "-dir", str(tmp_path), "-d", "0", "-pk", head[0], "-pke", head[1], "-pb", head[2], "-wl", str(p)], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode not in (0, 3) and r.stderr.strip(), p
        assert (p.read_bytes() if p.exists() else None) == before
        assert not (tmp_path / "kangaroo.work").exists()
