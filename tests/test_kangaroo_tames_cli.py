"""CPU: the tame table file and the host's side of -ktamesgen / -ktames (host/host_kangaroo_tames.cpp) against the model (tests/kangaroo_tames_model.py):
the file round trip through -selftest kangaroo-tames, every refusal of the reader and of the command line (all before any device is looked for), the image
through -selftest kangaroo-tames-image, and the search rule on scripted records line for line (-selftest kangaroo-tames-search)."""
import hashlib
import os
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_tames_model as TM
from pybsgs.ecpy import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")

A, W, T, DP = 0x1F << 36, 1 << 20, 48, 2
KP = [0x2BCDE, 0x12345, 0xF00D, 0xFFFF0]                        # k_k - a of the keys
PUBS = [mul(A + k) for k in KP]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def host(args, stdin=None, cwd=None):
    assert os.path.exists(HOST), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([HOST] + args, capture_output=True, text=True, input=stdin, timeout=120, cwd=cwd)


@pytest.fixture(scope="module")
def table():
    """a small table from the model's generator, computed once"""
    f, steps, merges = TM.generate(A, W, T, DP, 8, 5)
    assert len(f["entries"]) == T and steps >= T
    for x, d in f["entries"][:8]:
        assert mul(d)[0] & TM.M64 == x and K.is_dp(mul(d)[0], DP)
    return f


def write(path, f, **kw):
    fields = dict(dp=f["dp"], pk=f["pk"], pke=f["pke"], steps=f["steps"], seed=f["seed"], m=f["m"], scalars=f["scalars"], entries=f["entries"])
    fields.update(kw)
    blob = TM.pack_file(**fields)
    with open(path, "wb") as o:
        o.write(blob)
    return blob


def test_plan_defaults():
    assert TM.plan(1 << 36, 16384, 6) == (1 << 15, 1 << 33, 1 << 32, 8 * ((1 << 16) + 64))
    assert TM.plan(1 << 64, 1 << 26, 10) == (1 << 27, 1 << 61, 1 << 32, 8 * ((1 << 28) + 1024))      # E: W / 8 where 4 m W / K is less
    assert TM.plan(1 << 20, 1 << 20, 4)[0] == 2 and TM.plan(1 << 20, 48, 2)[2] == 1 << 18


def test_file_round_trip(tmp_path, table):
    path = str(tmp_path / "kangaroo.tames")
    blob = write(path, table)
    assert len(blob) == 624 + 24 * T and TM.parse_file(blob) == table
    r = host(["-selftest", "kangaroo-tames", path])
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:9] == ["version 1", "dp %d" % DP, "pk %064x" % A, "pke %064x" % (A + W - 1), "entries %d" % T, "steps %d" % table["steps"],
                                        "seed 0x5", "mean jump %d" % table["m"], "ok"]
    assert host(["-selftest", "kangaroo-tames", path, "%x" % A, "%x" % (A + W - 1)]).returncode == 0
    r = host(["-selftest", "kangaroo-tames", path, "%x" % A, "%x" % (A + W)])
    assert r.returncode == 1 and r.stderr.strip() == "Tame table was made for another range"
    assert open(path, "rb").read() == blob


def damaged(table):
    e = table["entries"]
    zero = list(table["scalars"])
    zero[17] = 0
    blob = TM.pack_file(table["dp"], table["pk"], table["pke"], table["steps"], table["seed"], table["m"], table["scalars"], e)
    return {
        "magic": (dict(magic=b"KANGTAMF"), "is not a tame table (magic)"),
        "version": (dict(version=2), "tame table version 2, this program reads version 1"),
        "length": (blob[:-1], "wrong length for a tame table"),
        "length, entries missing": (blob[:-24], "wrong length for a tame table"),
        "ordering": (dict(entries=e[:5] + [e[6], e[5]] + e[7:]), "entries are not strictly ascending (entry 6)"),
        "ordering, twice": (dict(entries=e[:5] + [e[5], e[5]] + e[7:]), "entries are not strictly ascending (entry 6)"),
        "zero scalar": (dict(scalars=zero), "jump scalar 17 is zero"),
    }


@pytest.mark.parametrize("what", ["magic", "version", "length", "length, entries missing", "ordering", "ordering, twice", "zero scalar"])
def test_reader_refusals(tmp_path, table, what):
    change, message = damaged(table)[what]
    path = str(tmp_path / "kangaroo.tames")
    if isinstance(change, dict):
        blob = write(path, table, **change)
    else:
        blob = change
        open(path, "wb").write(blob)
    with pytest.raises(ValueError, match=what.split(",")[0]):
        TM.parse_file(blob)
    for r in (host(["-selftest", "kangaroo-tames", path]),
              host(["-kangaroo", "-ktames", path, "-pb", compressed(PUBS[0]), "-pk", "%x" % A, "-pke", "%x" % (A + W - 1), "-dir", str(tmp_path)])):
        lines = [ln for ln in (r.stdout + r.stderr).split("\n") if message in ln]
        assert r.returncode != 0 and len(lines) == 1, (r.stdout, r.stderr)
    assert open(path, "rb").read() == blob and sorted(os.listdir(tmp_path)) == ["kangaroo.tames"]


def test_another_range_is_refused(tmp_path, table):
    path = str(tmp_path / "kangaroo.tames")
    blob = write(path, table)
    for pk, pke in ((A - 1, A + W - 1), (A, A + W)):
        r = host(["-kangaroo", "-ktames", path, "-pb", compressed(PUBS[0]), "-pk", "%x" % pk, "-pke", "%x" % pke, "-dir", str(tmp_path)])
        assert r.returncode != 0 and "Tame table was made for another range" in r.stdout + r.stderr
        assert "GPU" not in r.stdout + r.stderr
    assert open(path, "rb").read() == blob


@pytest.mark.parametrize("extra, message", [
    (["-ksym"], "-ktames cannot be combined with -ksym"),
    (["-kwalk", "sym"], "-ktames cannot be combined with -kwalk sym"),
    (["-wl", "kangaroo.work"], "-ktames cannot be combined with -wl"),
    (["-dp", "6"], "-ktames cannot be combined with -dp"),
])
def test_refused_option_combinations(tmp_path, extra, message):
    # (the table file does not even exist: the options are refused first, and before any device is looked for)
    r = host(["-kangaroo", "-ktames", "none.tames", "-pb", compressed(PUBS[0]), "-pk", "%x" % A, "-pke", "%x" % (A + W - 1), "-dir", str(tmp_path)] + extra)
    out = r.stdout + r.stderr
    assert r.returncode != 0 and len([ln for ln in out.split("\n") if message in ln]) == 1 and "none.tames" not in out, out
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra, message", [
    (["-ktn", "64", "-wl", "kangaroo.work"], "-ktamesgen cannot be combined with -wl"),
    (["-ktn", "64", "-wt", "60"], "-ktamesgen cannot be combined with -wt"),
    ([], "-ktamesgen needs -ktn"),
    (["-ktn", "64", "-ktames", "x.tames"], "-ktamesgen and -ktames exclude each other"),
    (["-ktn", "64", "-pb", compressed(PUBS[0])], "-ktamesgen takes no -pb or -infile"),
])
def test_refused_generator_options(tmp_path, extra, message):
    r = host(["-kangaroo", "-ktamesgen", "t.tames", "-pk", "%x" % A, "-pke", "%x" % (A + W - 1), "-dir", str(tmp_path)] + extra)
    assert r.returncode != 0 and message in r.stdout + r.stderr, r.stdout + r.stderr
    assert os.listdir(tmp_path) == []


def test_image_selftest_digest():
    tags = TM.chain_tags(60) + [0, 1 << 63, 12345]
    r = host(["-selftest", "kangaroo-tames-image"], stdin=" ".join(("0x%x" if i & 1 else "%d") % t for i, t in enumerate(tags)) + "\n")
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:2] == ["lines 64", "digest " + hashlib.sha1(TM.image(tags)).hexdigest()]
    r = host(["-selftest", "kangaroo-tames-image"], stdin="5 6 5\n")
    assert r.returncode == 1 and "share the tag" in r.stderr


def script_lines(tmp_path, table, pubs, n_wild, limit, items):
    """items: ("R", x, d, w) | ("D", w) | ("L",) -> (the host's lines, the model's)"""
    path = str(tmp_path / "rule.tames")
    write(path, table)
    args = []
    rule = TM.SearchRule(table, pubs, n_wild, limit)
    want = rule.presolved_lines()
    for it in items:
        if it[0] == "R":
            args.append("R,%064x,%032x,%d" % (it[1], it[2] & K.M128, it[3]))
            want += rule.record(it[1], it[2], it[3])
        elif it[0] == "D":
            args.append("D,%d" % it[1])
            want += rule.dead(it[1])
        else:
            args.append("L")
            want += rule.launch()
    want.append(rule.summary())
    r = host(["-selftest", "kangaroo-tames-search", path, ",".join(compressed(p) for p in pubs), str(n_wild), str(limit)] + args)
    assert r.returncode == 0, r.stdout + r.stderr
    return [ln for ln in r.stdout.split("\n") if ln], want


def on_entry(table, e, k):
    """the record of a wild kangaroo of key k that stands on entry e's point: x(d_T * G), d_W = d_T - k'_k"""
    x64, d = table["entries"][e]
    x = mul(d)[0]
    assert x & TM.M64 == x64
    return x, d - KP[k]


def test_search_rule_on_scripted_records(tmp_path, table):
    # six wild kangaroos over three keys: 0 1 2 0 1 2
    x0, d0 = on_entry(table, 3, 0)
    x1, d1 = on_entry(table, 40, 1)
    items = [("R", mul(777)[0], 5, 0),                               # not in the table
             ("R", x1, d1 + 1, 1),                                   # a table entry's x, an offset that does not solve: false match, it walks on
             ("R", x1, d1 + W, 4),                                   # k' beyond the range
             ("D", 2),                                               # dead: starts afresh on its own key
             ("R", x0, d0, 3),                                       # tame match: key 0 found, kangaroos 0 and 3 go to the keys with the fewest
             ("R", x0, d0, 3),                                       # kangaroo 3 works on another key now: false for that one
             ("L",), ("L",), ("L",),                                 # limit 2: every kangaroo not started afresh meanwhile is aged at the third
             ("R", x1, d1, 1),                                       # key 1 found
             ("R", x1, d1, 4)]                                       # a kangaroo of key 1 reassigned already
    got, want = script_lines(tmp_path, table, PUBS[:3], 6, 2, items)
    assert got == want
    assert want[:5] == ["miss", "false", "false", "reseed 2 2", "found 0 %064x" % (A + KP[0])]
    assert want[5:7] == ["reassign 0 1", "reassign 3 2"] and want[7] == "false"
    assert [ln.split()[0] for ln in want[8:14]] == ["aged"] * 6 and want[14] == "found 1 %064x" % (A + KP[1])
    assert want[-1].startswith("summary 6 4 7 2")


def test_search_rule_equal_points_presolved_and_rest(tmp_path, table):
    pubs = [PUBS[3], mul(A), PUBS[3], PUBS[1]]                       # 0 and 2 are the same point, 1 is a*G
    x3, d3 = on_entry(table, 11, 3)
    x1, d1 = on_entry(table, 12, 1)
    items = [("R", x3, d3, 0), ("R", x3, d3, 1), ("R", x1, d1, 2), ("D", 0), ("L",), ("L",)]
    got, want = script_lines(tmp_path, table, pubs, 3, 1, items)
    assert got == want
    assert want[0] == "presolved 1" and want[1] == "found 0 %064x" % (A + KP[3]) and "found 2 %064x" % (A + KP[3]) in want
    assert any(ln.startswith("rest") for ln in want) and want[-1].endswith(" 4")
