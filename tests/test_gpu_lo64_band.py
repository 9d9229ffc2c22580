"""The low-64-bit squaring on the device (fe_sqr_add2_lo64 with the banded square fe_sqr_win69) on crafted lambdas: the largest dropped columns, w7' at and
just below its wrap margin, lo32(Rest) at the 4096 edge, non-canonical lambdas.  lo64_selftest_kernel with iters = 1 runs each thread's (lambda, c1, c2)
exactly as given (lambda = a[i], c1 = b[i] mod p, c2 = a[(7 i + 3) mod n] mod p); its counts must match the Python model's (tests/lo64_band_model.py)."""
import random

import pytest

from lo64_band_model import B, P, craft_rest_lo, crafted_lambdas, limbs, lo64, want, win69

pytestmark = pytest.mark.gpu


def _expect(a, b):
    """(mismatches, exact-path lanes) the model predicts for one selftest launch"""
    n = len(a)
    bad = slow = 0
    for i in range(n):
        lam, c1, c2 = a[i], b[i] % P, a[(7 * i + 3) % n] % P
        x, s, _, _ = lo64(lam, c1, c2)
        slow += s
        bad += (not s) and x != want(lam, c1, c2)
    assert bad == 0
    return bad, slow


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def test_crafted_classes(dev):
    rnd = random.Random(2026)
    for label, lams in crafted_lambdas(rnd):
        a = lams + [rnd.randrange(1 << 256) for _ in range(256 - len(lams))]     # random fill
        b = [rnd.randrange(P) for _ in a]
        got = dev.selftest_lo64(a, b, 1)
        exp_bad, exp_slow = _expect(a, b)
        assert got == (exp_bad, exp_slow, len(a)), label
        if label == "w7_near_wrap":
            assert exp_slow >= len(lams)                  # every near-wrap lane counted as exact-path


def test_rest_at_the_4096_edge(dev):
    rnd = random.Random(4096)
    n = 512
    a = [rnd.randrange(1 << 256) for _ in range(n)]
    b = [rnd.randrange(P) for _ in range(n)]
    targets = [0xFFFFEFFF, 0xFFFFEFFF - 1967, 0xFFFFF000, 0xFFFFFFFF]
    for i in range(n):
        b[i] = craft_rest_lo(a[i], a[(7 * i + 3) % n] % P, targets[i % 4], rnd)
    got = dev.selftest_lo64(a, b, 1)
    exp_bad, exp_slow = _expect(a, b)
    assert exp_slow >= n // 2
    assert got == (exp_bad, exp_slow, n)


def test_w7_near_wrap_only(dev):
    """a launch of near-wrap lanes only: all of them take the exact path, none is wrong"""
    from lo64_band_model import craft_w7
    rnd = random.Random(8)
    a = [craft_w7(rnd, B - 1 - (i % 8), low_ones=bool(i & 8)) for i in range(256)]
    b = [rnd.randrange(P) for _ in a]
    assert all(win69(limbs(x))[0] >= B - 8 for x in a)
    assert dev.selftest_lo64(a, b, 1) == (0, 256, 256)
