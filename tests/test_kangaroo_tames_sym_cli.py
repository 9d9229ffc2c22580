"""CPU: the version-2 tame table file and the host's side of -ktamesgen -kwalk sym / -ktamessym (host/host_kangaroo_tames.cpp) against the model
(tests/kangaroo_tames_sym_model.py): the file round trip through -selftest kangaroo-tames sym, every refusal of the reader and of the command line (all before
any device is looked for), versions 1 and 2 refusing each other, and the symmetric search rule on scripted records line for line
(-selftest kangaroo-tames-search sym)."""
import os
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_tames_model as TM
import kangaroo_tames_sym_model as TS
from pybsgs.ecpy import N, mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")

A, W, T, DP, R = 0x1F << 36, 1 << 20, 48, 2, 64
MID = A + W // 2
KPP = [0x2BCDE - W // 2, 0x12345 - W // 2, 0xF00D - W // 2, W - W // 2 - 16]      # k''_k = k_k - (a + W/2): three below the middle, one at the top
PUBS = [mul(MID + k) for k in KPP]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def host(args, cwd=None):
    assert os.path.exists(HOST), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([HOST] + args, capture_output=True, text=True, timeout=120, cwd=cwd)


@pytest.fixture(scope="module")
def table():
    """a small table from the model's generator on the curve, computed once"""
    f, steps, merges = TS.generate(A, W, T, DP, 8, 5, R)
    assert len(f["entries"]) == T and steps >= T
    assert any(d < 0 for _, d in f["entries"]) and any(d > 0 for _, d in f["entries"])      # the representative's offset: either sign
    for x, d in f["entries"][:8]:
        p = mul(d % N)
        assert p[0] & TM.M64 == x and K.is_dp(p[0], DP) and p[1] & 1 == 0
    return f


def fields(f, **kw):
    out = dict(dp=f["dp"], pk=f["pk"], pke=f["pke"], steps=f["steps"], seed=f["seed"], m=f["m"], R=f["R"], scale=f["scale"], scalars=f["scalars"], entries=f["entries"])
    out.update(kw)
    return out


def write(path, f, **kw):
    blob = TS.pack_file(**fields(f, **kw))
    with open(path, "wb") as o:
        o.write(blob)
    return blob


def search_args(path, tmp_path, flag="-ktamessym", extra=(), pk=A, pke=A + W - 1):
    return ["-kangaroo", flag, path, "-pb", compressed(PUBS[0]), "-pk", "%x" % pk, "-pke", "%x" % pke, "-dir", str(tmp_path)] + list(extra)


def test_plan_defaults():
    # the GPU test's shape: 2^20 trail points over 512 kangaroos are 2048 steps each, m sqrt(n) = E / 2 with the integer root 45
    assert TS.plan(1 << 36, 16384, 6, 512) == ((1 << 32) // 90, 1 << 32, 1 << 30, 8 * ((1 << 16) + 64))
    # config 4 with the default herd of one MI355X: 185383 steps each, root 430
    assert TS.plan(1 << 64, 1 << 26, 10, 370688) == ((1 << 60) // 860, 1 << 60, 1 << 32, 8 * ((1 << 28) + 1024))
    assert TS.plan(W, T, DP, 8) == (W // 16 // 8, W // 16, W // 64, 8 * (W // (T << DP) + 4))      # 24 steps each, root 4
    assert TS.plan(1 << 40, 4, 0, 8)[0] == 1 << 37 and TS.plan(1 << 40, 1 << 20, 10, 1 << 40)[0] == 1 << 35      # never below W / 2K; n at least 1


def test_file_round_trip(tmp_path, table):
    path = str(tmp_path / "kangaroo.tames")
    blob = write(path, table)
    assert len(blob) == 128 + 8 * R + 24 * T and TS.parse_file(blob) == table
    r = host(["-selftest", "kangaroo-tames", "sym", path])
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:11] == ["version 2", "dp %d" % DP, "pk %064x" % A, "pke %064x" % (A + W - 1), "entries %d" % T, "steps %d" % table["steps"],
                                         "seed 0x5", "mean jump %d" % table["m"], "jumps %d" % R, "jump scale 1", "ok"]
    assert host(["-selftest", "kangaroo-tames", "sym", path, "%x" % A, "%x" % (A + W - 1)]).returncode == 0
    r = host(["-selftest", "kangaroo-tames", "sym", path, "%x" % A, "%x" % (A + W)])
    assert r.returncode == 1 and r.stderr.strip() == "Tame table was made for another range"
    assert open(path, "rb").read() == blob
    # more jump points and another scale
    big = dict(table, R=256, scale=0.5, scalars=[1 + j for j in range(256)])
    blob = write(path, big)
    assert len(blob) == 128 + 8 * 256 + 24 * T and TS.parse_file(blob) == big
    r = host(["-selftest", "kangaroo-tames", "sym", path])
    assert r.returncode == 0 and "jumps 256\njump scale 0.5\nok" in r.stdout, r.stdout + r.stderr


def damaged(table):
    e = table["entries"]
    zero = list(table["scalars"])
    zero[17] = 0
    blob = TS.pack_file(**fields(table))
    return {
        "magic": (dict(magic=b"KANGTAMF"), "is not a tame table (magic)"),
        "version": (dict(version=3), "tame table version 3, this program reads version 2"),
        "jumps, not a power of two": (dict(R=96, scalars=table["scalars"] + [5] * 32), "-kjumps 96"),
        "jumps, too few": (dict(R=32, scalars=table["scalars"][:32]), "-kjumps 32"),
        "jumps, too many": (dict(R=8192, scalars=table["scalars"] * 128), "-kjumps 8192"),
        "length": (blob[:-1], "wrong length for a tame table"),
        "length, entries missing": (blob[:-24], "wrong length for a tame table"),
        "length, scalars missing": (dict(scalars=table["scalars"][:63]), "wrong length for a tame table"),
        "length, the fixed part cut": (blob[:120], "wrong length for a tame table"),
        "ordering": (dict(entries=e[:5] + [e[6], e[5]] + e[7:]), "entries are not strictly ascending (entry 6)"),
        "ordering, twice": (dict(entries=e[:5] + [e[5], e[5]] + e[7:]), "entries are not strictly ascending (entry 6)"),
        "zero scalar": (dict(scalars=zero), "jump scalar 17 is zero"),
    }


@pytest.mark.parametrize("what", ["magic", "version", "jumps, not a power of two", "jumps, too few", "jumps, too many", "length", "length, entries missing",
                                  "length, scalars missing", "length, the fixed part cut", "ordering", "ordering, twice", "zero scalar"])
def test_reader_refusals(tmp_path, table, what):
    change, message = damaged(table)[what]
    path = str(tmp_path / "kangaroo.tames")
    if isinstance(change, dict):
        blob = write(path, table, **change)
    else:
        blob = change
        open(path, "wb").write(blob)
    with pytest.raises(ValueError, match=what.split(",")[0]):
        TS.parse_file(blob)
    for r in (host(["-selftest", "kangaroo-tames", "sym", path]), host(search_args(path, tmp_path))):
        out = r.stdout + r.stderr
        lines = [ln for ln in out.split("\n") if message in ln]
        assert r.returncode != 0 and len(lines) == 1 and "GPU" not in out, (r.stdout, r.stderr)
    assert open(path, "rb").read() == blob and sorted(os.listdir(tmp_path)) == ["kangaroo.tames"]


def test_another_range_is_refused(tmp_path, table):
    path = str(tmp_path / "kangaroo.tames")
    blob = write(path, table)
    for pk, pke in ((A - 1, A + W - 1), (A, A + W)):
        r = host(search_args(path, tmp_path, pk=pk, pke=pke))
        assert r.returncode != 0 and "Tame table was made for another range" in r.stdout + r.stderr
        assert "GPU" not in r.stdout + r.stderr
    assert open(path, "rb").read() == blob


def test_versions_refuse_each_other(tmp_path, table):
    """each reader meets the other's file: one line in the wording of the version check, which names the flag that is missing or too many"""
    v2 = str(tmp_path / "sym.tames")
    write(v2, table)
    v1 = str(tmp_path / "plain.tames")
    plain = TM.pack_file(table["dp"], table["pk"], table["pke"], table["steps"], table["seed"], table["m"], table["scalars"], table["entries"])
    open(v1, "wb").write(plain)
    assert TM.parse_file(plain)["entries"] == table["entries"]
    with pytest.raises(ValueError, match="version"):
        TM.parse_file(open(v2, "rb").read())
    with pytest.raises(ValueError, match="version"):
        TS.parse_file(plain)
    cases = [(search_args(v2, tmp_path, flag="-ktames"), "tame table version 2, this program reads version 1", "symmetric walk: -ktamessym"),
             (["-selftest", "kangaroo-tames", v2], "tame table version 2, this program reads version 1", "-ktamessym"),
             (search_args(v1, tmp_path), "tame table version 1, this program reads version 2", "plain walk: -ktames)"),
             (["-selftest", "kangaroo-tames", "sym", v1], "tame table version 1, this program reads version 2", "plain walk: -ktames)")]
    for args, message, flag in cases:
        r = host(args)
        out = r.stdout + r.stderr
        lines = [ln for ln in out.split("\n") if message in ln]
        assert r.returncode != 0 and len(lines) == 1 and flag in lines[0] and "GPU" not in out, out
    assert host(["-selftest", "kangaroo-tames", v1]).returncode == 0 and host(["-selftest", "kangaroo-tames", "sym", v2]).returncode == 0


def test_the_symmetric_table_has_its_flags(tmp_path):
    """-ktamessym goes on to its table (which is not there), -ktamesgen -kwalk sym to the generator's own checks; -ktames keeps refusing -kwalk sym (the table
    names its walk) and now says how such a table is searched"""
    r = host(search_args("none.tames", tmp_path))
    out = r.stdout + r.stderr
    assert r.returncode != 0 and "cannot open" in out and "none.tames" in out and "cannot be combined" not in out, out
    r = host(["-kangaroo", "-ktamesgen", "t.tames", "-kwalk", "sym", "-kjumps", "256", "-kjumpscale", "2", "-pk", "%x" % A, "-pke", "%x" % (A + W - 1), "-dir", str(tmp_path)])
    assert r.returncode != 0 and "-ktamesgen needs -ktn" in r.stdout + r.stderr
    r = host(search_args("none.tames", tmp_path, flag="-ktames", extra=("-kwalk", "sym")))
    lines = [ln for ln in (r.stdout + r.stderr).split("\n") if "-ktames cannot be combined with -kwalk sym" in ln]
    assert r.returncode != 0 and len(lines) == 1 and "-ktamessym" in lines[0]
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("mode, extra, message", [
    ("-ktames", ["-ksym"], "-ktames cannot be combined with -ksym"),
    ("-ktamesgen", ["-ksym", "-ktn", "64"], "-ktamesgen cannot be combined with -ksym"),
    ("-ktamessym", ["-ksym"], "-ktamessym cannot be combined with -ksym"),
    ("-ktamessym", ["-kwalk", "sym"], "-ktamessym cannot be combined with -kwalk sym"),
    ("-ktamessym", ["-ktames", "other.tames"], "-ktames and -ktamessym exclude each other"),
    ("-ktamessym", ["-ktamesgen", "other.tames", "-ktn", "64"], "-ktamesgen and -ktamessym exclude each other"),
    ("-ktamessym", ["-kjumps", "256"], "-ktamessym takes no -kjumps or -kjumpscale"),
    ("-ktamessym", ["-kjumpscale", "2"], "-ktamessym takes no -kjumps or -kjumpscale"),
    ("-ktamessym", ["-dp", "6"], "-ktamessym cannot be combined with -dp"),
    ("-ktamessym", ["-wl", "kangaroo.work"], "-ktamessym cannot be combined with -wl"),
])
def test_refused_option_combinations(tmp_path, mode, extra, message):
    args = ["-kangaroo", mode, "none.tames", "-pk", "%x" % A, "-pke", "%x" % (A + W - 1), "-dir", str(tmp_path)] + ([] if mode == "-ktamesgen" else ["-pb", compressed(PUBS[0])])
    r = host(args + extra)
    out = r.stdout + r.stderr
    lines = [ln for ln in out.split("\n") if message in ln]
    assert r.returncode != 0 and len(lines) == 1 and "cannot open" not in out, out
    if "-ksym" in extra:
        assert "-ktamesgen -kwalk sym" in lines[0] and "-ktamessym" in lines[0]      # the refusal names the options that do it
    assert os.listdir(tmp_path) == []


# ---- the search rule -------------------------------------------------------------------------------------------------------------------------------------
def script_lines(tmp_path, table, pubs, n_wild, limit, items):
    """items: ("W" | "N", x, d, w) | ("D", w) | ("C", w) | ("L",) -> (the host's lines, the model's)"""
    path = str(tmp_path / "rule.tames")
    write(path, table)
    args = []
    rule = TS.SearchRule(table, pubs, n_wild, limit)
    want = rule.presolved_lines()
    for it in items:
        if it[0] in "WN":
            args.append("%s,%064x,%032x,%d" % (it[0], it[1], it[2] & K.M128, it[3]))
            want += rule.record(it[1], it[2], it[3], neg=it[0] == "N")
        elif it[0] == "D":
            args.append("D,%d" % it[1])
            want += rule.dead(it[1])
        elif it[0] == "C":
            args.append("C,%d" % it[1])
            want += rule.cycle(it[1])
        else:
            args.append("L")
            want += rule.launch()
    want.append(rule.summary())
    r = host(["-selftest", "kangaroo-tames-search", "sym", path, ",".join(compressed(p) for p in pubs), str(n_wild), str(limit)] + args)
    assert r.returncode == 0, r.stdout + r.stderr
    return [ln for ln in r.stdout.split("\n") if ln], want


def on_entry(table, e, kpp, sigma, eps):
    """the record of a wild kangaroo of a key k'' that stands on the class of entry e: sigma Q + d_W G = eps d_T G, so d_W = eps d_T - sigma k'' ->
    (type letter, x, d_W)"""
    x64, dT = table["entries"][e]
    x = mul(dT % N)[0]
    assert x & TM.M64 == x64
    dW = eps * dT - sigma * kpp
    assert mul((sigma * kpp + dW) % N)[0] == x                       # the wild kangaroo does stand on that x
    return "W" if sigma > 0 else "N", x, dW


def test_search_rule_on_scripted_records(tmp_path, table):
    # eight wild kangaroos over four keys: 0 1 2 3 0 1 2 3
    r0 = on_entry(table, 3, KPP[0], 1, 1)                             # the first candidate, eps = +1
    r1 = on_entry(table, 40, KPP[1], -1, -1)                          # NEG, and only the second candidate solves
    r2 = on_entry(table, 7, KPP[2], 1, -1)                            # no NEG, the second candidate
    r3 = on_entry(table, 20, KPP[3], -1, 1)                           # NEG, the first candidate; the key at the top of the range
    items = [("W", mul(777)[0], 5, 0),                               # not in the table
             (r1[0], r1[1], r1[2] + 1, 1),                           # an entry's x, an offset that solves with neither sign: false match, it walks on
             ("W", r1[1], r1[2], 1),                                 # the right offset with the wrong sign of Q: false
             (r1[0], r1[1], r1[2] + W, 5),                           # k'' beyond the range
             ("D", 2), ("C", 6),                                     # dead, and retired by the cycle check: both start afresh on their own key
             r0 + (4,),                                              # key 0 found: kangaroos 0 and 4 go to the keys with the fewest
             r0 + (4,),                                              # kangaroo 4 works on another key now: false for that one
             ("L",), ("L",), ("L",),                                 # limit 2: every kangaroo not started afresh meanwhile is aged at the third
             r1 + (1,), r1 + (5,),                                   # key 1 found; a kangaroo of key 1 reassigned already
             r2 + (2,), r3 + (3,)]
    got, want = script_lines(tmp_path, table, PUBS, 8, 2, items)
    assert got == want
    assert want[:6] == ["miss", "false", "false", "false", "reseed 2 2", "reseed 6 2"]
    assert want[6] == "found 0 %064x" % (MID + KPP[0]) and want[7:9] == ["reassign 0 1", "reassign 4 2"] and want[9] == "false"
    assert [ln.split()[0] for ln in want[10:18]] == ["aged"] * 8 and want[18] == "found 1 %064x" % (MID + KPP[1])
    found = [ln for ln in want if ln.startswith("found")]
    assert found == ["found %d %064x" % (k, MID + KPP[k]) for k in range(4)]
    assert want[-1] == "summary 9 5 10 4 1"                          # nine matches, five of them false; two dead and eight aged; four keys; one cycle


def test_search_rule_stale_presolved_and_rest(tmp_path, table):
    pubs = [PUBS[3], mul(MID), PUBS[3], PUBS[1]]                     # 0 and 2 are the same point, 1 is the middle of the range itself
    r3 = on_entry(table, 11, KPP[3], 1, 1)
    r1 = on_entry(table, 12, KPP[1], -1, -1)
    items = [r3 + (0,), r3 + (1,), r1 + (2,), r1 + (2,), ("D", 0), ("C", 1), ("L",), ("L",)]      # the fourth: by a kangaroo that rests on a solved key
    got, want = script_lines(tmp_path, table, pubs, 3, 1, items)
    assert got == want
    assert want[0] == "presolved 1" and want[1] == "found 0 %064x" % (MID + KPP[3]) and "found 2 %064x" % (MID + KPP[3]) in want
    assert "stale" in want and "false" in want
    assert any(ln.startswith("rest") for ln in want) and want[-1].split()[4] == "4"
