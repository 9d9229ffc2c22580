"""CPU: the version-2 kangaroo work file of -ksym (host_kangaroo_work.cpp).  The symmetric table goes through a version-2 file at every split of
scripted record streams and still gives the model's verdicts; the file holds the model's table at the split; each mode refuses the other's file."""
import os
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_sym_workfile as WF2
import kangaroo_workfile as WF1
from test_kangaroo_sym_model import TYPES, compressed, scripted_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")


def model(a, W, pub, records, upto=None):
    t = S.SymTable(a, W, pub)
    out, at_split = [], None
    for i, (typ, x, d, kid) in enumerate(records):
        if i == upto:
            at_split = (dict(t.map), t.false_matches, t.reseeds, t.cycles)
        v, key = t.add(x, d & K.M128, kid, TYPES[typ])
        out.append("found %064x" % key if v == "found" else "reseed %d" % kid if v == "reseed" else v)
    if at_split is None:
        at_split = (dict(t.map), t.false_matches, t.reseeds, t.cycles)
    out.append("summary %d %d %d %d" % (len(t.map), t.false_matches, t.reseeds, t.cycles))
    return out, at_split


def host_args(a, W, pub, records):
    return ["%x" % a, "%x" % (a + W - 1), compressed(pub)], ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in records]


def roundtrip(which, a, W, pub, records, split, keep=None):
    head, recs = host_args(a, W, pub, records)
    env = dict(os.environ)
    env.pop("BSGS_SELFTEST_WORK", None)
    if keep:
        env["BSGS_SELFTEST_WORK"] = str(keep)
    return subprocess.run([HOST, "-selftest", which] + head + [str(split)] + recs, capture_output=True, text=True, timeout=60, env=env)


def work_header(path, extra=()):
    r = subprocess.run([HOST, "-selftest", "kangaroo-work", str(path)] + list(extra), capture_output=True, text=True, timeout=60)
    return r, dict(ln.split(" ", 1) for ln in r.stdout.split("\n") if " " in ln)


@pytest.mark.parametrize("name", ["tame_neg", "wild_wild_rev", "other"])
def test_version2_round_trip_at_every_split(tmp_path, name):
    _, a, W, pub, recs = next(s for s in scripted_streams() if s[0] == name)
    head, _ = host_args(a, W, pub, recs)
    want, _ = model(a, W, pub, recs)
    for split in range(len(recs) + 1):
        path = tmp_path / ("split%d.work" % split)
        r = roundtrip("kangaroo-sym-roundtrip", a, W, pub, recs, split, keep=path)
        assert r.returncode == 0, (split, r.stderr)
        assert r.stdout.split("\n")[:-1] == want, split
        _, (table, false_matches, reseeds, cycles) = model(a, W, pub, recs, upto=split)
        w = WF2.parse(path.read_bytes())
        dps = sum(1 for r in recs[:split] if r[0] not in "DC")
        assert (w["version"], w["jumps"], w["jumpscale"], w["cycles"], w["dps"], w["table"], w["false_matches"], w["reseeds"]) == \
            (2, 1024, 1.0, cycles, dps, len(table), false_matches, reseeds)
        assert sorted(w["entries"]) == sorted((k64, d, kid, fl) for k64, (d, kid, fl) in table.items())
        r, h = work_header(path, head)
        assert r.returncode == 0 and "fingerprint-check ok" in r.stdout, r.stderr
        assert (h["version"], h["jumps"], h["jumpscale"], h["cycles"], h["table"], h["fingerprint"]) == ("2", "1024", "1", str(cycles), str(len(table)), w["fingerprint"])
    if name == "tame_neg":
        assert WF2.parse((tmp_path / "split1.work").read_bytes())["entries"][0][3] == 3          # a wild kangaroo with NEG in the table section


def test_each_mode_refuses_the_others_file(tmp_path):
    _, a, W, pub, recs = next(s for s in scripted_streams() if s[0] == "tame_wild")
    head, _ = host_args(a, W, pub, recs)
    v2, v1 = tmp_path / "v2.work", tmp_path / "v1.work"
    assert roundtrip("kangaroo-sym-roundtrip", a, W, pub, recs, 1, keep=v2).returncode == 0
    assert roundtrip("kangaroo-table-roundtrip", a, W, pub, [r for r in recs if r[0] in "TWD"], 1, keep=v1).returncode == 0
    assert WF2.parse(v2.read_bytes())["version"] == 2 and WF1.parse(v1.read_bytes())["version"] == 1
    # -selftest kangaroo-work prints both
    assert work_header(v1, head)[0].returncode == 0 and work_header(v2, head)[0].returncode == 0
    assert "version" not in work_header(v1)[1]
    base = [HOST, "-kangaroo", "-dir", str(tmp_path), "-d", "0", "-pk", head[0], "-pke", head[1], "-pb", head[2]]
    for extra, path, says in ((["-ksym"], v1, "has work file version 1, this host reads version 2"), ([], v2, "has work file version 2, this host reads version 1")):
        before = path.read_bytes()
        r = subprocess.run(base + extra + ["-wl", str(path)], capture_output=True, text=True, timeout=60)
        assert r.returncode not in (0, 3) and says in r.stderr, r.stderr
        assert path.read_bytes() == before and not (tmp_path / "kangaroo.work").exists()
    # a version-2 header that a version-2 reader must refuse: a jump count that is no power of two, a nonzero reserved word, a truncated extension
    data = v2.read_bytes()
    cases = {"jumps": data[:144] + (1000).to_bytes(4, "little") + data[148:], "reserved": data[:148] + b"\x01\0\0\0" + data[152:], "short": data[:150]}
    for what, blob in cases.items():
        p = tmp_path / (what + ".work")
        p.write_bytes(blob)
        r, _ = work_header(p)
        assert r.returncode != 0 and r.stderr.strip(), what
    # the fingerprint covers the jump count and the scale
    other = tmp_path / "other_jumps.work"
    other.write_bytes(data[:144] + (512).to_bytes(4, "little") + data[148:])
    r, _ = work_header(other, head)
    assert r.returncode != 0 and "other settings" in r.stderr


def test_ksym_options_are_checked_without_a_gpu():
    for extra in (["-kjumps", "1024"], ["-kjumpscale", "2"], ["-ksym", "-kjumps", "100"], ["-ksym", "-kjumps", "8192"], ["-ksym", "-kjumpscale", "0"]):
        r = subprocess.run([HOST, "-kangaroo"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stderr.strip(), extra
