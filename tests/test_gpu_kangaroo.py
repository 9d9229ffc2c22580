"""GPU: the kangaroo walk (csrc/kangaroo.hip) against the model (tests/kangaroo_model.py) -- every state bit-exact, the complete record list, the
equal-x cases inside ordinary batches -- and bsgs_mi355x -kangaroo end to end.  At most two GPU processes at a time: pytest and one host."""
import os
import subprocess

import pytest

import kangaroo_model as K
from pybsgs.ecpy import add, mul, neg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
PUB_PUZZLE64 = "03100611c54dfef604163b8358f7b7fac13ce478e02cb224ae16d45526b25d9d4d"
KEY_PUZZLE64 = 0xF7051F27B09112D4


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def herd(seed, W, Q, n):
    """n kangaroos, the first half tame, from the model's seeded stream"""
    rng = K.Stream(seed)
    out = []
    for i in range(n):
        wild = i >= n // 2
        d = K.herd_offset(rng, W, wild)
        p = K.start(Q, d, wild)
        out.append((p[0], p[1], d & K.M128, K.WILD if wild else 0))
    return out


def rec_key(r):
    return (r["x"], r["d"], r["kangaroo"], r["flags"], r["step"])


@pytest.mark.parametrize("n, per_thread", [(2048, 8), (1024, 16)])          # blocks of 256 threads (one inversion per block) / of 64 (one per thread)
def test_walk_parity(dev, n, per_thread):
    W = 1 << 40
    a = 0x123456789 << 40
    Q = add(mul(a + 0x9876543210), neg(mul(a)))
    scalars, jumps = K.jump_table(K.Stream(77), n * (W ** 0.5) / 4)
    dev.kangaroo_setup(jumps, scalars, 4, n, per_thread, 1 << 16)
    assert dev.kangaroo_geometry() == (n // per_thread, per_thread, 256 if (n // per_thread) % 256 == 0 else 64)
    states = herd(1000 + n, W, Q, n)
    dev.kangaroo_upload(0, states)
    assert dev.kangaroo_download(0, n) == states
    sample = list(range(0, n, n // 64))
    model_recs, gpu_recs = [], []
    # single steps first (every sampled state after every step), then one long launch: 64 steps in all
    for launch in [1] * 8 + [56]:
        states, recs = K.walk(states, jumps, scalars, launch, 4)
        model_recs += recs
        got, dropped, ms = dev.kangaroo_run(launch)
        assert dropped == 0
        gpu_recs += [rec_key(r) for r in got]
        if launch == 1:
            down = dev.kangaroo_download(0, n)
            assert [down[i] for i in sample] == [states[i] for i in sample]
    assert dev.kangaroo_download(0, n) == states
    assert sorted(gpu_recs) == sorted(model_recs)
    assert len(model_recs) > n * 64 // 32                          # dp = 4: about one step in 16 is a DP


def test_degenerate_steps_inside_ordinary_batches(dev):
    """a kangaroo standing on J_j (its next step is a doubling) and one on -J_j (its next step is infinity: one dead record, then it rests), both in the batch
    of thread 0 next to ordinary kangaroos: everything else still matches the model"""
    seed = next(s for s in range(1, 2000) if any(p[0] & 63 == j for j, p in enumerate(K.jump_table(K.Stream(s), 1 << 30)[1])))
    scalars, jumps = K.jump_table(K.Stream(seed), 1 << 30)
    j = next(j for j, p in enumerate(jumps) if p[0] & 63 == j)
    n, per_thread = 1024, 4
    T = n // per_thread
    states = herd(9, 1 << 32, mul(12345), n)
    jx, jy = jumps[j]
    states[0] = (jx, jy, scalars[j], 0)                             # thread 0, slot 0: doubling
    states[T] = (jx, neg(jumps[j])[1], 7, K.WILD)                   # thread 0, slot 1: x + J_j = infinity
    assert K.step(states[0], jumps, scalars)[1] == "double" and K.step(states[T], jumps, scalars)[1] == "dies"
    dev.kangaroo_setup(jumps, scalars, 0, n, per_thread, 1 << 14)
    dev.kangaroo_upload(0, states)
    want, recs = K.walk(states, jumps, scalars, 3, 0)
    got, dropped, _ = dev.kangaroo_run(3)
    assert dropped == 0
    assert dev.kangaroo_download(0, n) == want
    assert sorted(rec_key(r) for r in got) == sorted(recs)
    first, _ = K.step(states[0], jumps, scalars)
    assert (first[0], first[1]) == mul(2 * scalars[j])
    dead = [r for r in got if r["flags"] & K.DEAD]
    assert len(dead) == 1 and dead[0]["kangaroo"] == T and dead[0]["x"] == jx and dead[0]["step"] == 0 and dead[0]["flags"] == K.WILD | K.DEAD
    # re-seeding by index list brings the dead one back
    dev.kangaroo_upload_list([T], [states[1]])
    assert dev.kangaroo_download(T, 1) == [states[1]]


def test_record_overflow_is_counted_not_fatal(dev):
    scalars, jumps = K.jump_table(K.Stream(4), 1 << 30)
    n = 256
    states = herd(4, 1 << 30, mul(99), n)
    dev.kangaroo_setup(jumps, scalars, 0, n, 1, 100)
    dev.kangaroo_upload(0, states)
    got, dropped, _ = dev.kangaroo_run(2)
    assert len(got) == 100 and dropped == 2 * n - 100
    want, recs = K.walk(states, jumps, scalars, 2, 0)
    assert dev.kangaroo_download(0, n) == want
    assert set(rec_key(r) for r in got) <= set(recs)


def run_host(args, cwd, timeout=300):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([EXE, "-kangaroo", "-dir", str(cwd)] + args, capture_output=True, text=True, timeout=timeout)


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


def solve_cli(tmp_path, key, lo, hi, extra=()):
    r = run_host(["-pb", compressed(mul(key)), "-pk", "%x" % lo, "-pke", "%x" % hi, "-kseed", "0x%x" % (key & 0xFFFF)] + list(extra), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    with open(os.path.join(tmp_path, "win.txt"), "rb") as f:
        lines = f.read().decode().split("\r\n")
    assert lines[0] == "KEY[1]: 0x%064x" % key
    assert lines[1] == " " * 3 + "Pub: " + compressed(mul(key))
    assert "KEY[1]: 0x%064x" % key in r.stdout
    return r.stdout


@pytest.mark.parametrize("bits, where", [(40, "low"), (40, "high"), (48, "mid"), (56, "low"), (56, "high"), (64, "mid")])
def test_cli_planted_keys(tmp_path, bits, where):
    lo = 0x3 << 100 | (0x5A << bits)
    W = 1 << bits
    k = lo + {"low": 0, "high": W - 1, "mid": W // 3}[where]
    solve_cli(tmp_path, k, lo, lo + W - 1)


def test_cli_puzzle64(tmp_path):
    r = run_host(["-pb", PUB_PUZZLE64, "-pk", "8000000000000000", "-pke", "ffffffffffffffff", "-kseed", "64"], tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert open(os.path.join(tmp_path, "win.txt"), "rb").read().decode().split("\r\n")[0] == "KEY[1]: 0x%064x" % KEY_PUZZLE64


def test_cli_72bit_key(tmp_path):
    lo = 0xC0FFEE << 80
    solve_cli(tmp_path, lo + 0x5DEECE66D12345678A, lo, lo + (1 << 72) - 1)


def test_cli_two_engines_share_one_table(tmp_path):
    lo = 0x77 << 60
    out = solve_cli(tmp_path, lo + 0x123456789ABC, lo, lo + (1 << 52) - 1, ["-d", "0,0"])
    assert "2 engine(s)" in out
    counts = [int(ln.split(": ")[1].split()[0]) for ln in out.split("\n") if ln.startswith("Engine ")]
    assert len(counts) == 2 and all(c > 0 for c in counts), out[-1500:]


def test_cli_rejects_flag_combinations_and_widths(tmp_path):
    pub = compressed(mul(1 << 30))
    for extra in (["-w", "30"], ["-htsz", "25"], ["-infile", "keys.txt"], ["-wl", "currentwork.txt"], ["-onlygen"],
                  ["-pk", "1", "-pke", "fffff"],                                    # 2^20 - 1 keys: too narrow
                  ["-pk", "1", "-pke", "%x" % (1 << 126)]):                          # wider than 2^125
        r = run_host(["-pb", pub] + extra, tmp_path, timeout=60)
        assert r.returncode != 0, (extra, r.stdout[-800:])
