"""GPU: the tame table behind a herd whose records carry a key (csrc/kangaroo_tames.hip: bsgs_kangaroo_tames_install_keys, bsgs_kangaroo_run_tames_keys)
against the models (tests/kangaroo_tames_sym_model.py match, tests/kangaroo_symlist_model.py walk), bit for bit: the kept records are the walk's own, their
`reserved` word still the key, the entry numbers in the parallel array; a table of one entry, chains that overflow their home line and wrap past the last line,
both record capacities, and the state errors.  Herds of 256 kangaroos with 64 jump points, images of 64 lines."""
import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_symlist_model as SL
import kangaroo_tames_model as TM
import kangaroo_tames_sym_model as TS
from pybsgs.ecpy import P, add, mul, neg

pytestmark = pytest.mark.gpu

A, W = 0x5A5A5A << 40, 1 << 40
KEYS = [A + 0x1234567890, A + 0xFEDCBA9876, A + 7]
N_K, R, DP, STEPS = 256, 64, 2, 40


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def got_key(r):
    return (r["x"], r["d"], r["kangaroo"], r["flags"], r["step"], r["key"], r["entry"])


_CASE = {}


def launch_case():
    """an all-wild keyed herd on three keys, one kangaroo of it standing on -J_j of a jump point whose x selects j itself (it dies at step 0), and the model's
    records of its one launch; computed once -> (Qs, scalars, jumps, states, final states, records)"""
    if not _CASE:
        nmid = neg(mul(A + W // 2))
        Qs = [add(mul(k), nmid) for k in KEYS]
        # a jump table with a fixed point of odd y: a kangaroo on its negative has even y, is its own representative, and the sum is infinity
        seed = next(s for s in range(1, 4000) if any(p[0] & (R - 1) == j and p[1] & 1 for j, p in enumerate(S.jump_table(K.Stream(s), 1 << 30, R)[1])))
        scalars, jumps = S.jump_table(K.Stream(seed), 1 << 30, R)
        j = next(j for j, p in enumerate(jumps) if p[0] & (R - 1) == j and p[1] & 1)
        rng = K.Stream(77)
        states = []
        for i in range(N_K):
            d = S.herd_offset(rng, W, True)
            p = K.start(Qs[i % 3], d, True)
            states.append((p[0], p[1], d & K.M128, K.WILD, i % 3))
        states[131] = (jumps[j][0], P - jumps[j][1], 7, K.WILD, 2)
        final, recs = SL.walk(states, jumps, scalars, STEPS, DP)
        _CASE["v"] = (Qs, scalars, jumps, states, final, recs)
    return _CASE["v"]


@pytest.mark.parametrize("per_thread, block", [(1, 256), (2, 64)])
@pytest.mark.parametrize("table", ["some", "one entry", "unrelated"])
def test_match_against_the_model(dev, per_thread, block, table):
    Qs, scalars, jumps, states, final, recs = launch_case()
    dead = [r for r in recs if r[3] & K.DEAD and not r[3] & S.CYCLE]
    assert [(r[2], r[4], r[5]) for r in dead] == [(131, 0, 2)] and len(recs) > N_K * STEPS // 8      # dp = 2: about one step in four is a DP
    xs = list(dict.fromkeys(r[0] & TM.M64 for r in recs if not r[3] & K.DEAD))
    if table == "some":
        tags = xs[::len(xs) // 100][:100]
    elif table == "one entry":
        tags = xs[500:501]
    else:
        tags = [t for t in ((v * 0x9E3779B97F4A7C15 + 12345) & TM.M64 for v in range(120)) if t not in set(xs)]
    assert TM.n_lines(len(tags)) == 64
    want = TS.match(recs, tags)
    dev.kangaroo_setup_sym_keys(jumps, scalars, DP, N_K, per_thread, 1 << 13)
    assert dev.kangaroo_geometry() == (N_K // per_thread, per_thread, block)
    dev.kangaroo_set_keys(Qs)
    dev.kangaroo_upload(0, states)
    dev.kangaroo_tames_install_keys(tags)
    got, seen, dropped, ms = dev.kangaroo_run_tames_keys(STEPS)
    print(table, "records", len(recs), "returned", len(got), "ms", ms)
    assert seen == len(recs) and dropped == 0
    assert sorted(got_key(r) for r in got) == want
    assert all(r["key"] == r["kangaroo"] % 3 for r in got)           # `reserved` is still the key the walk wrote
    n_dead = len([r for r in recs if r[3] & K.DEAD])
    if table == "unrelated":
        assert len(want) == n_dead and all(r[6] is None for r in want)      # a DEAD record that matched nothing: 0 in the array
    elif table == "one entry":
        assert len(want) == n_dead + 1 and [r[6] for r in want if not r[3] & K.DEAD] == [0]
    else:
        assert len(want) >= 100 + n_dead and {r[6] for r in want if r[6] is not None} == set(range(100))
    # the walk itself is the symmetric one, unchanged: the herd ends where kangaroo_run would have left it
    assert dev.kangaroo_download(0, N_K) == final
    # a second table replaces the first
    dev.kangaroo_upload(0, states)
    dev.kangaroo_tames_install_keys(xs[3:4])
    got2, seen2, _, _ = dev.kangaroo_run_tames_keys(STEPS)
    assert seen2 == len(recs) and sorted(got_key(r) for r in got2) == TS.match(recs, xs[3:4])


def probe_states(probe_tags):
    """256 kangaroos, kangaroo i standing on -J_j, j = i % 64, of a jump table whose J_j has x = probe_tags[j] (bits 0..5 of it are j) and an odd y: each
    dies at step 0 and writes one DEAD record of that x; its key is i % 5 -> (jumps, scalars, states)"""
    assert [t & 63 for t in probe_tags] == list(range(64))
    jumps = [(t, 1001 + 2 * j) for j, t in enumerate(probe_tags)]
    states = [(probe_tags[i % 64], P - (1001 + 2 * (i % 64)), i, K.WILD, i % 5) for i in range(N_K)]
    return jumps, [1 + j for j in range(64)], states


def probe(dev, table_tags, probe_tags, cap=N_K, max_recs=None):
    """-> ({tag: entry or None} as matched against table_tags, seen, dropped, the records)"""
    jumps, scalars, states = probe_states(probe_tags)
    want_states, recs = SL.walk(states, jumps, scalars, 1, 0)
    assert len(recs) == N_K and all(r[3] == K.WILD | K.DEAD and r[4] == 0 for r in recs)
    want = {r[:6]: r[6] for r in TS.match(recs, table_tags)}
    dev.kangaroo_setup_sym_keys(jumps, scalars, 0, N_K, 1, cap)
    dev.kangaroo_upload(0, states)
    dev.kangaroo_tames_install_keys(table_tags)
    got, seen, dropped, _ = dev.kangaroo_run_tames_keys(1, max_recs=max_recs)
    keys = [got_key(r) for r in got]
    assert len(set(keys)) == len(got) and all(want[k[:6]] == k[6] for k in keys)      # records of the model, each with the model's entry
    assert all(r["key"] == r["kangaroo"] % 5 and r["d"] == r["kangaroo"] for r in got)
    assert dev.kangaroo_download(0, N_K) == want_states
    out = {}
    for r in got:
        assert out.setdefault(r["x"], r["entry"]) == r["entry"]
    return out, seen, dropped, got


@pytest.mark.parametrize("first_line", [5, 60])                      # 5: the chain overflows its home line into the next ones; 60: it wraps past the last line
def test_chains(dev, first_line):
    tags = TM.chain_tags(first_line)
    L = TM.build(tags)
    assert len(L) == 64 and [L[(first_line + k) & 63][2] for k in range(16)] == [1] * 15 + [0]
    full = (N_K, 0)
    assert probe(dev, tags, tags)[:3] == ({t: e for e, t in enumerate(tags)},) + full
    others = TM.chain_tags(first_line, salt=2)                       # the same home line, never inserted
    assert not set(others) & set(tags) and {TM.home(t, 64) for t in others} == {first_line}
    assert probe(dev, tags, others)[:3] == ({t: None for t in others},) + full
    mixed = tags[:32] + others[32:]
    assert probe(dev, tags, mixed)[:3] == ({t: (j if j < 32 else None) for j, t in enumerate(mixed)},) + full
    # entries in another order get other numbers, and a table of one entry finds that one
    assert probe(dev, tags[::-1], tags)[0] == {t: 63 - e for e, t in enumerate(tags)}
    assert probe(dev, tags[9:10], tags)[0] == {t: (0 if j == 9 else None) for j, t in enumerate(tags)}


def test_capacity(dev):
    """more records than the record buffer holds: the 64 that fit are matched, the rest counted; and a host buffer smaller than what was kept"""
    tags = TM.chain_tags(60)
    out, seen, dropped, got = probe(dev, tags, tags, cap=64)
    assert seen == N_K and len(got) == 64 and dropped == N_K - 64
    out, seen, dropped, got = probe(dev, tags, tags, cap=N_K, max_recs=16)
    assert seen == N_K and len(got) == 16 and dropped == N_K - 16
    # the plain call on the same herd is as it was: every record with its key
    jumps, scalars, states = probe_states(tags)
    dev.kangaroo_upload(0, states)
    plain, dropped, _ = dev.kangaroo_run(1)
    assert len(plain) == N_K and dropped == 0 and all(r["key"] == r["kangaroo"] % 5 for r in plain)


def test_state_errors():
    import pybsgs
    d = pybsgs.Device(0)
    try:
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_setup first"):
            d.kangaroo_tames_install_keys([1, 2, 3])
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_setup first"):
            d.kangaroo_run_tames_keys(1)
        scalars, jumps = S.jump_table(K.Stream(4), 1 << 30, R)
        d.kangaroo_setup_sym_keys(jumps, scalars, 0, 64, 1, 64)
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_tames_install_keys first"):
            d.kangaroo_run_tames_keys(1)
        with pytest.raises(pybsgs.BsgsError, match="share the tag"):
            d.kangaroo_tames_install_keys([7, 8, 7])
        with pytest.raises(pybsgs.BsgsError, match="tame table serves"):      # the plain table's call keeps refusing this herd
            d.kangaroo_tames_install([1, 2, 3])
        d.kangaroo_tames_install_keys([1, 2, 3])
        d.kangaroo_setup_sym_keys(jumps, scalars, 0, 64, 1, 64)      # a new herd: the table is gone with the old one
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_tames_install_keys first"):
            d.kangaroo_run_tames_keys(1)
        for setup in (lambda: d.kangaroo_setup_sym(jumps, scalars, 0, 64, 1, 64), lambda: d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)):
            setup()                                                  # herds without a key word: their table is the plain one
            with pytest.raises(pybsgs.BsgsError, match="serves the herd of bsgs_kangaroo_setup_sym_keys"):
                d.kangaroo_tames_install_keys([1, 2, 3])
            d.kangaroo_tames_install([1, 2, 3])
            with pytest.raises(pybsgs.BsgsError, match="serves the herd of bsgs_kangaroo_setup_sym_keys"):
                d.kangaroo_run_tames_keys(1)
    finally:
        d.close()
