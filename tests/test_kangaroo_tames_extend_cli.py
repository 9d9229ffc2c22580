"""CPU: the host's side of extending and merging tame tables (host/host_kangaroo_tames.cpp: -ktamesfrom, -ktnplan, -ktamesmerge) and the model of the load and
the sorted read (tests/kangaroo_tames_extend_model.py).  Files are made with the models' pack_file; no GPU is needed and none is visible to the host: -ktamesmerge
-noverify opens no device, and every refusal is made before one is looked for.  The model is checked against tests/kangaroo_tames_gen_model.py on the case
lists the GPU tests run (tests/kangaroo_tames_extend_cases.py)."""
import os
import subprocess
from collections import Counter

import pytest

import kangaroo_model as K
import kangaroo_tames_extend_cases as XC
import kangaroo_tames_extend_model as XM
import kangaroo_tames_gen_model as GM
import kangaroo_tames_model as TM
import kangaroo_tames_sym_model as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
PK, PKE = 0x800000000, 0xFFFFFFFFF
RANGE = ["-pk", "%x" % PK, "-pke", "%x" % PKE]


def host(args, cwd=None):
    assert os.path.exists(HOST), "host binary missing: run __graft_entry__.build()"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device is visible: a run that looked for one would end with another message
    return subprocess.run([HOST] + args, capture_output=True, text=True, timeout=120, cwd=cwd, env=env)


def refused(r, line, tmp_path, keep=()):
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stderr.strip().split("\n") == [line], r.stderr
    assert "GPU #" not in r.stdout and "No GPU found" not in r.stderr
    assert sorted(os.listdir(tmp_path)) == sorted(keep)


def fields(sym, **kw):
    rng = K.Stream(91)
    R = 64
    f = dict(dp=6, pk=PK, pke=PKE, steps=1000, seed=5, m=12345, scalars=[1 + rng.u64() % 20000 for _ in range(R)], entries=[])
    if sym:
        f.update(R=R, scale=1.0)
    f.update(kw)
    return f


def write(path, sym, **kw):
    f = fields(sym, **kw)
    blob = (TS if sym else TM).pack_file(**f)
    with open(path, "wb") as o:
        o.write(blob)
    return f


def three_tables(sym):
    """three tables of one walk, 200..300 entries each, 100 tags in all three; one holds tag 0"""
    rng = K.Stream(92 + sym)
    shared = XC.fresh_tags(rng, 100)
    own = [XC.fresh_tags(rng, n, avoid=shared) for n in (150, 100, 199)]
    assert len(set(own[0]) | set(own[1]) | set(own[2])) == 449
    tabs = []
    for k, mine in enumerate(own):
        tags = shared + mine + ([0] if k == 1 else [])
        tabs.append(sorted((t, K.signed128((XC.f(t) + (k if t in shared else 0)) & K.M128)) for t in tags))      # a shared tag has another d in each table
    assert [len(t) for t in tabs] == [250, 201, 299]
    return tabs


# ---- merge ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [False, True], ids=["plain", "sym"])
def test_merge(tmp_path, sym):
    tabs = three_tables(sym)
    walk = ["-kwalk", "sym"] if sym else []
    model = TS if sym else TM
    names = ["a.tames", "b.tames", "c.tames"]
    for k, (name, tab) in enumerate(zip(names, tabs)):
        write(str(tmp_path / name), sym, entries=tab, steps=1000 + k, seed=5 + k)
    want, dropped = XM.merge(tabs)
    assert len(want) == 100 + 449 + 1 and dropped == 200 and want[0][0] == 0
    r = host(["-kangaroo", "-dir", str(tmp_path), "-ktamesmerge", ",".join(names), "-ktamesgen", "out.tames", "-noverify"] + walk)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "550 distinct tags, 200 dropped" in r.stdout and "GPU #" not in r.stdout
    blob = open(str(tmp_path / "out.tames"), "rb").read()
    f = fields(sym, entries=want, steps=1000 + 1001 + 1002, seed=5)
    assert blob == model.pack_file(**f)                               # the sorted union, the first table's d for a shared tag, steps summed, the first seed
    assert model.parse_file(blob)["entries"] == want
    # -ktn: the lowest tags
    cut, _ = XM.merge(tabs, 300)
    r = host(["-kangaroo", "-dir", str(tmp_path), "-ktamesmerge", ",".join(names), "-ktamesgen", "cut.tames", "-ktn", "300", "-noverify"] + walk)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "200 dropped" in r.stdout
    assert open(str(tmp_path / "cut.tames"), "rb").read() == model.pack_file(**dict(f, entries=want[:300])) and cut == want[:300]
    # the order of the inputs decides whose d a shared tag keeps
    r = host(["-kangaroo", "-dir", str(tmp_path), "-ktamesmerge", "c.tames,a.tames", "-ktamesgen", "ca.tames", "-noverify"] + walk)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert model.parse_file(open(str(tmp_path / "ca.tames"), "rb").read())["entries"] == XM.merge([tabs[2], tabs[0]])[0]
    # the selftest reads the result as it is
    r = host(["-selftest", "kangaroo-tames"] + (["sym"] if sym else []) + [str(tmp_path / "out.tames"), "%x" % PK, "%x" % PKE])
    assert r.returncode == 0 and "entries 550\nsteps 3003\nseed 0x5\n" in r.stdout and r.stdout.strip().endswith("ok")


def test_merge_refusals(tmp_path):
    tabs = three_tables(False)
    a, b = str(tmp_path / "a.tames"), str(tmp_path / "b.tames")
    keep = ["a.tames", "b.tames"]
    fa = write(a, False, entries=tabs[0])

    def merge(extra=(), walk=()):
        return host(["-kangaroo", "-dir", str(tmp_path), "-ktamesmerge", "a.tames,b.tames", "-ktamesgen", "out.tames", "-noverify"] + list(extra) + list(walk))

    write(b, True, entries=tabs[1])                                   # another version
    refused(merge(), "-ktamesmerge: %s: tame table version 2, this program reads version 1 (version 2 is a table of the symmetric walk: -ktamessym)" % b, tmp_path, keep)
    refused(merge(walk=["-kwalk", "sym"]), "-ktamesmerge: %s: tame table version 1, this program reads version 2 with -ktamessym (version 1 is a table of the plain walk: -ktames)" % a,
            tmp_path, keep)
    write(b, False, entries=tabs[1], dp=7)
    refused(merge(), "-ktamesmerge: %s was not made by the walk of %s: -dp 7 against 6" % (b, a), tmp_path, keep)
    write(b, False, entries=tabs[1], pke=PKE - 1)
    refused(merge(), "-ktamesmerge: %s was not made by the walk of %s: the range [%064x, %064x] is another" % (b, a, PK, PKE - 1), tmp_path, keep)
    sc = list(fa["scalars"])
    sc[17] += 1
    write(b, False, entries=tabs[1], scalars=sc)
    refused(merge(), "-ktamesmerge: %s was not made by the walk of %s: jump scalar 17 differs" % (b, a), tmp_path, keep)
    write(b, False, entries=tabs[1], m=12346)
    refused(merge(), "-ktamesmerge: %s was not made by the walk of %s: mean jump 12346 against 12345" % (b, a), tmp_path, keep)
    rng = K.Stream(93)
    write(a, True, entries=tabs[0])
    write(b, True, entries=tabs[1], R=128, scalars=fa["scalars"] + [1 + rng.u64() % 20000 for _ in range(64)])      # another R
    refused(merge(walk=["-kwalk", "sym"]), "-ktamesmerge: %s was not made by the walk of %s: -kjumps 128 against 64" % (b, a), tmp_path, keep)
    write(b, True, entries=tabs[1], scale=2.0)
    refused(merge(walk=["-kwalk", "sym"]), "-ktamesmerge: %s was not made by the walk of %s: the jump scale differs" % (b, a), tmp_path, keep)
    # -ktn above the union: refused after the count, nothing written
    write(a, False, entries=tabs[0])
    write(b, False, entries=tabs[1])
    r = merge(extra=["-ktn", "352"])
    refused(r, "-ktamesmerge: -ktn 352 is above the 351 tags of the union; nothing written", tmp_path, keep)
    assert "351 distinct tags, 100 dropped" in r.stdout
    assert merge(extra=["-ktn", "351"]).returncode == 0
    os.remove(str(tmp_path / "out.tames"))
    # the command line
    r = host(["-kangaroo", "-dir", str(tmp_path), "-ktamesmerge", "a.tames,b.tames"])
    refused(r, "-ktamesmerge belongs to -ktamesgen (the file the merged table is written to)", tmp_path, keep)
    r = host(["-kangaroo", "-dir", str(tmp_path), "-ktamesmerge", "a.tames", "-ktamesgen", "out.tames", "-noverify"])
    refused(r, "-ktamesmerge needs at least two tables: A,B[,C...]", tmp_path, keep)


# ---- extend -----------------------------------------------------------------------------------------------------------------------------------------------
def test_extend_refusals(tmp_path):
    tabs = three_tables(False)
    a, s = str(tmp_path / "a.tames"), str(tmp_path / "s.tames")
    keep = ["a.tames", "s.tames"]
    write(a, False, entries=tabs[0])                                  # 250 entries, seed 5, dp 6
    write(s, True, entries=tabs[0])
    gen = ["-kangaroo", "-dir", str(tmp_path), "-ktamesgen", "out.tames"]
    msg = "-ktamesfrom belongs to -ktamesgen -ktamesdev (a table is extended in GPU memory)"
    refused(host(gen + ["-ktamesfrom", "a.tames", "-ktn", "500"] + RANGE), msg, tmp_path, keep)
    refused(host(["-kangaroo", "-dir", str(tmp_path), "-ktamesfrom", "a.tames", "-pb", "02" + "%064x" % 1] + RANGE), msg, tmp_path, keep)
    ext = gen + ["-ktamesdev", "-ktamesfrom", "a.tames"]
    for ktn in ("250", "100"):
        refused(host(ext + ["-ktn", ktn, "-kseed", "6"]), "-ktamesfrom: -ktn %s must be above the 250 entries of the table that is extended" % ktn, tmp_path, keep)
    refused(host(ext + ["-ktn", "500", "-kseed", "5"]), "-ktamesfrom: -kseed is the seed the table was made with (the new herd would retrace its starts): give another", tmp_path, keep)
    refused(host(ext + ["-ktn", "500", "-kseed", "6", "-dp", "5"]), "-ktamesfrom: -dp 5 differs from the table's -dp 6", tmp_path, keep)
    refused(host(ext + ["-ktn", "500", "-kseed", "6", "-pk", "%x" % PK, "-pke", "%x" % (PKE - 1)]), "-ktamesfrom: Tame table was made for another range", tmp_path, keep)
    # the file names its walk: version 2 without -kwalk sym, and the reverse
    refused(host(gen + ["-ktamesdev", "-ktamesfrom", "s.tames", "-ktn", "500", "-kseed", "6"]),
            "-ktamesfrom: %s: tame table version 2, this program reads version 1 (version 2 is a table of the symmetric walk: -ktamessym)" % s, tmp_path, keep)
    refused(host(ext + ["-ktn", "500", "-kseed", "6", "-kwalk", "sym"]),
            "-ktamesfrom: %s: tame table version 1, this program reads version 2 with -ktamessym (version 1 is a table of the plain walk: -ktames)" % a, tmp_path, keep)
    refused(host(gen + ["-ktamesdev", "-ktamesfrom", "s.tames", "-ktn", "500", "-kseed", "6", "-kwalk", "sym", "-kjumps", "128"]),
            "-ktamesfrom: -kjumps 128 differs from the table's 64", tmp_path, keep)
    # -ktnplan
    refused(host(gen + ["-ktamesdev", "-ktn", "500", "-ktnplan", "499"] + RANGE), "-ktnplan must not be below -ktn (it is the size the table is meant to reach)", tmp_path, keep)
    refused(host(ext + ["-ktn", "500", "-ktnplan", "1000"]), "-ktnplan cannot be combined with -ktamesfrom (the walk comes from the table that is extended)", tmp_path, keep)
    refused(host(["-kangaroo", "-dir", str(tmp_path), "-ktnplan", "1000", "-pb", "02" + "%064x" % 1] + RANGE), "-ktnplan belongs to -ktamesgen", tmp_path, keep)
    # what the command line names and the file confirms is accepted: the run gets as far as looking for a device
    r = host(ext + ["-ktn", "500", "-kseed", "6", "-dp", "6"] + RANGE)
    assert "-ktamesfrom" not in r.stderr and "Extending a table of 250 entries" in r.stdout


def test_the_model_refuses_what_the_host_refuses():
    assert XM.extend_refusal(250, 5, 6, 500, 6) is None and XM.extend_refusal(250, 5, 6, 500, 6, dp=6) is None
    assert "-ktamesdev" in XM.extend_refusal(250, 5, 6, 500, 6, ktamesdev=False)
    assert "-ktn" in XM.extend_refusal(250, 5, 6, 250, 6) and "-kseed" in XM.extend_refusal(250, 5, 6, 500, 5)
    assert "-dp" in XM.extend_refusal(250, 5, 6, 500, 6, dp=5) and "-ktnplan" in XM.extend_refusal(250, 5, 6, 500, 6, ktnplan=1000)
    with pytest.raises(ValueError):
        XM.merge([[(1, 1)], [(1, 2), (2, 2)]], 3)
    assert XM.merge([[(1, 1)], [(1, 2), (2, 2)]], 2) == ([(1, 1), (2, 2)], 1)


def test_the_help_names_the_flags():
    r = host(["-h"])
    assert all(flag in r.stdout for flag in ("-ktamesfrom", "-ktnplan", "-ktamesmerge"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert all(flag in readme for flag in ("-ktamesfrom", "-ktnplan", "-ktamesmerge"))


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(XC.load_cases()))
def test_model_load_is_the_insert_without_hand_backs(case):
    a = b = GM.new_table(XC.CAPACITY, XC.CAP)
    for what, items in XC.load_cases()[case]:
        if what == "insert":
            a, b = GM.insert(a, items)[0], GM.insert(b, items)[0]
            continue
        a, n = XM.load(a, items)
        b, back = GM.insert(b, [(t, d, 0) for t, d in items])
        by = Counter()
        for (_, reason), c in back.items():
            by[reason] += c
        assert n == {"stored": len(items) - sum(by.values()), "duplicate": by[GM.GEN_DUPLICATE], "zero": by[GM.GEN_TAG_ZERO], "full": by[GM.GEN_FULL]}
        assert sum(n.values()) == len(items)
    assert a == b and GM.entries(a) == len(a["cand"])


def test_model_load_counts():
    cases = XC.load_cases()
    t, n = XM.load(GM.new_table(XC.CAPACITY, XC.CAP), cases["equal_tags"][0][1])
    assert n == {"stored": 90, "duplicate": 70, "zero": 608, "full": 0}
    t, n = XM.load(GM.new_table(XC.CAPACITY, XC.CAP), cases["chain_wraps"][0][1])
    assert [s for s, v in enumerate(t["tags"]) if v] == list(range(39)) + [XC.SLOTS - 1]
    full = [(k + 1, k) for k in range(XC.SLOTS + 5)]                 # more tags than slots: the last five find none
    t, n = XM.load(GM.new_table(XC.CAPACITY, XC.CAP), full)
    assert n == {"stored": XC.SLOTS, "duplicate": 0, "zero": 0, "full": 5}


@pytest.mark.parametrize("case", sorted(XC.sort_cases()))
def test_model_sorted_read(case):
    tags, cut = XC.sort_cases()[case]
    pairs = [(t, XC.f(t)) for t in tags]
    table, n = XM.load(GM.new_table(max(1, len(tags)), XC.CAP), pairs)
    assert n["stored"] == len(tags) == GM.entries(table)
    got, count = XM.read_sorted(table, cut)
    assert count == len(tags) and [(t, next(iter(c))) for t, c in got] == sorted(pairs)[:cut]
    assert XM.radix_sort(pairs) == sorted(pairs)                      # the device's passes, tile by tile, give the same order
    want_passes = {"lowest_byte": [0], "top_56_shared": [0], "highest_byte": [56], "low_16_zero": [16, 24, 32, 40, 48, 56], "empty": [], "one": []}
    assert XM.sort_passes(tags) == want_passes.get(case, list(range(0, 64, 8)))
