"""GPU: degenerate kangaroo steps at every slot, wave and block of the walks (csrc/kangaroo.hip: kangaroo_kernel, kangaroo_sym_kernel, kangaroo_sym_keys_kernel,
each with and without the block inversion) against the models, bit for bit.  The herds are those of tests/kangaroo_edge_cases.py -- every kind of degenerate
kangaroo at every slot of every block of five, ordinary kangaroos in every coupled set; tests/test_kangaroo_edge_cases.py checks that matrix on the CPU.
Integer equality throughout."""
import pytest

import kangaroo_edge_cases as E
import kangaroo_model as K
import kangaroo_sym_model as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def rec_key(case, r):
    return (r["x"], r["d"], r["kangaroo"], r["flags"], r["step"]) + ((r["key"],) if case.keyed else ())


def fresh_herd(dev, case):
    """setup, the block size intended, the herd uploaded but for its `never` kangaroos, and the download of what was put"""
    setup = dev.kangaroo_setup_sym_keys if case.keyed else dev.kangaroo_setup_sym if case.R else dev.kangaroo_setup
    setup(case.jumps, case.scalars, E.DP, case.geom.N, case.geom.G, E.RECORD_CAP)
    assert dev.kangaroo_geometry() == (case.geom.T, case.geom.G, 256 if case.geom.T in (E.BLOCK_T, E.CYCLE_BLOCK_T) else 64)
    idx = case.uploaded
    dev.kangaroo_upload_list(idx, [case.states[i] for i in idx])
    msg = E.mismatch(case, dev.kangaroo_download(0, case.geom.N), case.states)
    assert not msg, "after the upload\n" + msg


def record_diff(case, got, want):
    """'' when the lists are equal as sorted lists (every record exactly once); else the first records missing and extra, by position"""
    got, want = sorted(got), sorted(want)
    if got == want:
        return ""
    from collections import Counter
    g, w = Counter(got), Counter(want)
    missing, extra = sorted((w - g).elements()), sorted((g - w).elements())
    def show(r):
        return "%s step %d flags %#x x %#x d %#x" % (E.where(case.geom, r[2]) if r[2] < case.geom.N else "kangaroo %d" % r[2], r[4], r[3], r[0], r[1])
    return "\n".join(["%s: %d records missing, %d extra" % (case.name, len(missing), len(extra))] + ["  missing " + show(r) for r in missing[:4]] +
                     ["  extra   " + show(r) for r in extra[:4]])


def run_and_compare(dev, case, steps, want_states, want_recs, what):
    got, dropped, _ = dev.kangaroo_run(steps)
    assert dropped == 0, what
    msg = E.mismatch(case, dev.kangaroo_download(0, case.geom.N), want_states)
    assert not msg, what + "\n" + msg
    keys = [rec_key(case, r) for r in got]
    msg = record_diff(case, keys, want_recs)
    assert not msg, what + "\n" + msg
    return keys


@pytest.mark.parametrize("herd", E.PACKED, ids=["%s-T%d-G%d" % h for h in E.PACKED])
def test_packed_herd(dev, herd):
    case = E.packed_case(*herd)
    exp = E.expected("packed", *herd)
    dead = E.dead_records(case, exp)
    assert {s for s, _ in dead} == {0, 1}
    # one launch of three steps
    fresh_herd(dev, case)
    keys = run_and_compare(dev, case, E.STEPS, exp.after[-1], exp.one_launch, "one launch of %d steps" % E.STEPS)
    want_dead = sorted(r[:4] + (s,) + r[5:] for s, r in dead)                        # the step of the launch, the flags and (keyed) the key of each death
    assert sorted(k for k in keys if k[3] & K.DEAD) == want_dead
    if case.keyed:
        assert all(k[5] == k[2] + 1 for k in keys)
    # the same herd from a fresh upload, three launches of one step: the whole herd compared after each
    fresh_herd(dev, case)
    for launch in range(E.STEPS):
        keys = run_and_compare(dev, case, 1, exp.after[launch], exp.recs[launch], "launch %d of one step" % launch)
        assert sorted(k for k in keys if k[3] & K.DEAD) == [r for s, r in dead if s == launch]


@pytest.mark.parametrize("herd", E.CYCLE, ids=["%s-T%d-G%d" % h for h in E.CYCLE])
def test_cycle_herd(dev, herd):
    case = E.cycle_case(*herd)
    exp = E.expected("cycle", *herd)
    fresh_herd(dev, case)
    keys = run_and_compare(dev, case, case.steps, exp.after[0], exp.recs[0], "one launch of %d steps" % case.steps)
    placed = sorted(p.i for p in case.placements)
    cyc = sorted((k for k in keys if k[3] & S.CYCLE and k[2] in placed), key=lambda k: k[2])
    assert [k[2] for k in cyc] == placed                                             # one CYCLE record per placed kangaroo
    model = {r[2]: r for r in exp.recs[0] if r[3] & S.CYCLE}
    for k in cyc:
        assert k == model[k[2]] and k[4] == 2 and k[3] & (K.DEAD | S.CYCLE) == K.DEAD | S.CYCLE, E.where(case.geom, k[2])
        assert not case.keyed or k[5] == k[2] + 1
