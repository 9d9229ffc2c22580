"""GPU: the symmetric kangaroo walk (csrc/kangaroo.hip kangaroo_sym_kernel, through bsgs_kangaroo_setup_sym) against the model (tests/kangaroo_sym_model.py),
bit for bit: every state and the complete record list over several launches, with and without a cycle check, the equal-x cases and a hand-built 2-cycle inside
ordinary batches, and a walk carried through download and upload into a fresh herd."""
import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
from pybsgs.ecpy import P, add, mul, neg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def herd(seed, W, Q, n):
    """n kangaroos, the first half tame, from the model's seeded stream: y of either parity, no last index"""
    rng = K.Stream(seed)
    out = []
    for i in range(n):
        wild = i >= n // 2
        d = S.herd_offset(rng, W, wild)
        p = K.start(Q, d, wild)
        out.append((p[0], p[1], d & K.M128, K.WILD if wild else 0))
    return out


def rec_key(r):
    return (r["x"], r["d"], r["kangaroo"], r["flags"], r["step"])


def run_both(dev, states, jumps, scalars, launches, dp, check_each=()):
    """the launches on the GPU and in the model: (final model states, model records, GPU records), states compared after every launch named in check_each"""
    model_recs, gpu_recs = [], []
    n = len(states)
    for k, launch in enumerate(launches):
        states, recs = S.walk(states, jumps, scalars, launch, dp)
        model_recs += [r[:4] + (k, r[4]) for r in recs]
        got, dropped, _ = dev.kangaroo_run(launch)
        assert dropped == 0
        gpu_recs += [rec_key(r)[:4] + (k, r["step"]) for r in got]
        if k in check_each:
            assert dev.kangaroo_download(0, n) == states, k
    return states, model_recs, gpu_recs


# blocks of 256 threads (one inversion per block) / of 64 (one per thread); the table in device memory at both ends of its size
@pytest.mark.parametrize("n, per_thread, R, dp", [(2048, 8, 1024, 4), (1024, 16, 1024, 0), (2048, 8, 64, 0), (1024, 16, 64, 4)])
def test_walk_parity(dev, n, per_thread, R, dp):
    import pybsgs
    assert (pybsgs.KANGAROO_NEG, pybsgs.KANGAROO_CYCLE) == (S.NEG, S.CYCLE)
    W = 1 << 40
    a = 0x123456789 << 40
    Q = add(mul(a + 0x9876543210), neg(mul(a + W // 2)))
    scalars, jumps = S.jump_table(K.Stream(77), n * (W ** 0.5) / 4, R)
    dev.kangaroo_setup_sym(jumps, scalars, dp, n, per_thread, 1 << 17)
    assert dev.kangaroo_geometry() == (n // per_thread, per_thread, 256 if (n // per_thread) % 256 == 0 else 64)
    states = herd(1000 + n, W, Q, n)
    assert sum(s[1] & 1 for s in states) > n // 4 and sum(1 - (s[1] & 1) for s in states) > n // 4
    dev.kangaroo_upload(0, states)
    assert dev.kangaroo_download(0, n) == states
    # single steps, launches without a cycle check (S <= C), launches with one (S > C): 66 steps in all
    launches = [1, 1, 1, 8, S.WINDOW, S.WINDOW + 1, 22]
    final, model_recs, gpu_recs = run_both(dev, states, jumps, scalars, launches, dp, check_each=(0, 1, 2, 4, 5))
    assert dev.kangaroo_download(0, n) == final
    assert sorted(gpu_recs) == sorted(model_recs)
    assert all(s[1] & 1 == 0 and s[3] & S.LAST_VALID for s in final)
    assert any(s[3] & S.NEG for s in final[n // 2:]) and not any(s[3] & S.NEG for s in final[:n // 2])
    assert len(model_recs) > (n * 66 // 32 if dp else n * 66 - n)


def equal_x_table(even, R):
    for seed in range(1, 20000):
        scalars, jumps = S.jump_table(K.Stream(seed), 1 << 30, 64)
        for j, p in enumerate(jumps):
            if p[0] & 63 == j and p[0] & (R - 1) == j and (p[1] & 1 == 0) == even:
                more, mj = S.jump_table(K.Stream(seed + 50000), 1 << 30, R - 64) if R > 64 else ([], [])
                return scalars + more, jumps + mj, j
    raise AssertionError("no such table")


@pytest.mark.parametrize("R", [64, 1024])
def test_degenerate_steps_inside_ordinary_batches(dev, R):
    """kangaroos standing on the class of J_j with j their own index, in the batch of thread 0 next to ordinary kangaroos: with J_j.y even both J_j and -J_j
    double; with J_j.y odd both die (one dead record of the state they had, then they rest).  Everything else still matches the model."""
    n, per_thread = 1024, 4
    T = n // per_thread
    for even in (True, False):
        scalars, jumps, j = equal_x_table(even, R)
        jx, jy = jumps[j]
        states = herd(9, 1 << 32, mul(12345), n)
        states[0] = (jx, jy, scalars[j], 0)
        states[T] = (jx, P - jy, 7, K.WILD)
        kinds = [S.step(states[i], jumps, scalars)[1] for i in (0, T)]
        assert kinds == (["double", "double"] if even else ["dies", "dies"])
        dev.kangaroo_setup_sym(jumps, scalars, 0, n, per_thread, 1 << 14)
        dev.kangaroo_upload(0, states)
        want, recs = S.walk(states, jumps, scalars, 3, 0)
        got, dropped, _ = dev.kangaroo_run(3)
        assert dropped == 0
        assert dev.kangaroo_download(0, n) == want
        assert sorted(rec_key(r) for r in got) == sorted(recs)
        dead = sorted((r["kangaroo"], r["x"], r["d"], r["flags"], r["step"]) for r in got if r["flags"] & K.DEAD)
        assert dead == ([] if even else [(0, jx, scalars[j], K.DEAD, 0), (T, jx, 7, K.WILD | K.DEAD, 0)])
    # re-seeding by index list brings a dead one back
    dev.kangaroo_upload_list([T], [states[1]])
    assert dev.kangaroo_download(T, 1) == [states[1]]


@pytest.mark.parametrize("n, per_thread, R", [(2048, 8, 1024), (1024, 16, 64)])
def test_hand_built_cycle_in_a_herd(dev, n, per_thread, R):
    """the 2-cycle of the model's test, placed twice in a herd: launches of at most C steps leave it alone, the first longer launch retires it at the model's
    step with one CYCLE record, and its neighbours walk on as the model's do"""
    scalars, jumps, cyc, a, b = S.short_cycle_case(17, R)
    states = herd(5, 1 << 36, mul(0xABCDEF), n)
    places = [3, n // 2 + 70]
    for i in places:
        states[i] = cyc
    dev.kangaroo_setup_sym(jumps, scalars, 6, n, per_thread, 1 << 16)
    dev.kangaroo_upload(0, states)
    launches = [5, S.WINDOW, 40, 30]
    final, model_recs, gpu_recs = run_both(dev, states, jumps, scalars, launches, 6, check_each=(0, 1, 2))
    assert dev.kangaroo_download(0, n) == final
    assert sorted(gpu_recs) == sorted(model_recs)
    cyc_recs = [r for r in gpu_recs if r[3] & S.CYCLE]
    # launches 0 and 1 took 21 steps (odd: the kangaroo stands on the other point of the cycle); launch 2 marks after step 23 and finds the mark 2 steps later
    for i in places:
        mine = [r for r in cyc_recs if r[2] == i]
        assert len(mine) == 1 and mine[0][4:] == (2, 40 - S.WINDOW + 1) and mine[0][3] & K.DEAD
        assert final[i][3] & K.DEAD and final[i][3] & S.CYCLE
    assert sum(1 for s in final if s[3] & K.DEAD) <= n // 16                          # the neighbours walk on


def test_download_upload_continues_exactly(dev):
    """download -> a fresh herd -> upload -> continue equals the uninterrupted walk: the last index and NEG travel in the flags"""
    n, per_thread, R, dp = 1024, 4, 64, 3
    W = 1 << 44
    Q = mul(0x1234567890ABCDEF)
    scalars, jumps = S.jump_table(K.Stream(31), n * (W ** 0.5) / 4, R)
    states = herd(77, W, Q, n)
    dev.kangaroo_setup_sym(jumps, scalars, dp, n, per_thread, 1 << 16)
    dev.kangaroo_upload(0, states)
    first, _, _ = dev.kangaroo_run(20)
    mid = dev.kangaroo_download(0, n)
    second, _, _ = dev.kangaroo_run(30)
    end = dev.kangaroo_download(0, n)
    assert all(s[3] & S.LAST_VALID for s in mid) and any(s[3] & S.NEG for s in mid)
    import pybsgs
    other = pybsgs.Device(0)
    try:
        other.kangaroo_setup_sym(jumps, scalars, dp, n, per_thread, 1 << 16)
        other.kangaroo_upload(0, mid)
        again, dropped, _ = other.kangaroo_run(30)
        assert dropped == 0
        assert other.kangaroo_download(0, n) == end
        assert sorted(rec_key(r) for r in again) == sorted(rec_key(r) for r in second)
    finally:
        other.close()
    m1, r1 = S.walk(states, jumps, scalars, 20, dp)
    m2, r2 = S.walk(m1, jumps, scalars, 30, dp)
    assert (m1, m2) == (mid, end)
    assert sorted(rec_key(r) for r in first) == sorted(r1) and sorted(rec_key(r) for r in second) == sorted(r2)
    # a walk without the last index takes another path: the field is not decoration
    stripped = [(x, y, d, fl & ~S.LAST_MASK) for x, y, d, fl in mid]
    assert S.walk(stripped, jumps, scalars, 30, dp)[0] != end


def test_setup_sym_checks_its_arguments(dev):
    import pybsgs
    scalars, jumps = S.jump_table(K.Stream(1), 1 << 20, 128)
    for R in (32, 96):
        with pytest.raises(pybsgs.BsgsError):
            dev.kangaroo_setup_sym(jumps[:R], scalars[:R], 0, 256, 1, 100)
    with pytest.raises(pybsgs.BsgsError):
        dev.kangaroo_setup_sym(jumps, [0] + scalars[1:], 0, 256, 1, 100)
    with pytest.raises(pybsgs.BsgsError):
        dev.kangaroo_setup_sym(jumps, scalars, 0, 100, 1, 100)
