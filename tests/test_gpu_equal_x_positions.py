"""Equal-x giants (P = +-G2[i]: the batch element Px - Gx is zero, 2 Py takes its place, the plus probe is x(2P), code 4) at EVERY batch position of the
tile kernels of csrc/giant_kernel.hip.h.  Each unrolled position of a chain substitutes on its own, and most re-derive their neighbours' d and must substitute
there too; a site that forgets it zeroes the thread's product -- and, through fe_inv_block, that of lane l of all four waves of the block -- and a site that
takes the other tile's Py spoils every inverse behind the element.  Either way OTHER giants of the thread or block get wrong keys: silent misses.

So every case (tests/equal_x_cases.py; its lists are checked on the CPU by tests/test_equal_x_cases.py) comes with a table of every key that every thread of
the equal-x giant's 256-thread block probes, for both tiles of a pair, and the hit list must EQUAL the oracle's (o_tile_ref over that table) and contain the
completeness set the geometry demands: both records of every giant of the block.  Everything is an integer comparison.
  (a) the single-tile kernels, every slot, both signs        (b) the pair walk, every slot, six kinds of tile pairs; the same launches with one tile per block
  (c) list layouts 4 and 5 and the any-bucket kernels         (d) the instrumented instantiations: per-thread digests against the oracle's keys
  (e) the tail block's clamped lanes, a single partial wave   (f) the narrow batching of a one-tile launch"""
import os

import numpy as np
import pytest

import equal_x_cases as E
import ext_table_model as X
from test_gpu_multitile import _device
from test_gpu_round6 import InstalledTable, _kernel_name

pytestmark = pytest.mark.gpu

P10, P7 = (64, 8, 10), (64, 8, 7)


def _open(tpb, variant=None):
    """a Device that read BSGS_TILES_PER_BLOCK (and BSGS_KERNEL_VARIANT) when it was opened"""
    if variant is None:
        return _device(tpb)
    os.environ["BSGS_KERNEL_VARIANT"] = str(variant)
    try:
        return _device(tpb)
    finally:
        del os.environ["BSGS_KERNEL_VARIANT"]


def _giants_on(dev, geom):
    dev.upload_g2(E.giants(geom)[0], *geom)
    assert dev.engine_geometry() == (geom[0] * geom[1], geom[2])         # i = tid * p + j


def _check(bt, want, hits, n, tag):
    assert n == len(want) <= E.HIT_BUFFER, (tag, n, len(want))            # the reported total is the list's length: nothing overflowed
    assert hits == want, (tag, sorted(set(want) - set(hits))[:6], sorted(set(hits) - set(want))[:6])      # as lists: every record exactly once
    assert bt.complete <= set(hits), tag


def _run_list(dev, name, args, layout, kernel, tpb):
    """every case of a list through dev.run on its reference-format table; returns the hit lists, one per case"""
    out = []
    for n, bt in enumerate(E.built_list(name, *args)):
        gpu, want = E.expected(name, args, n)
        dev.upload_htgpu(gpu, 1 << E.HTSZ, len(bt.keys), layout)
        hits, nh, _ = dev.run(bt.case.centres, E.HIT_BUFFER)
        assert dev.last_kernel() == kernel and dev.last_tiles_per_block() == tpb, (bt.case.name, dev.last_kernel(), dev.last_tiles_per_block())
        _check(bt, want, hits, nh, (bt.case.name, kernel, tpb))
        out.append(hits)
    assert len(out) == len(E.CASE_LISTS[name](*args)) > 0
    return out


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,layout,variant,kernel", [
    (E.BASE, 2, None, "giant_pair2_kernel<2, false, true>"),              # quad chain, 64-byte lines: temporaries in LDS
    (E.BASE, 3, None, "giant_pair2_kernel<3, false, true>"),              # quad chain, 128-byte lines: temporaries in registers
    (E.BASE, 2, 10, "giant_pair2_kernel<2, false, false>"),               # pair chain, forced
    (P10, 2, None, "giant_pair2_kernel<2, false, false>"),                # pair chain by batch length (five pairs)
    (E.BASE, 2, 0, "giant_tile_kernel<2>"),                               # per-giant, forced
    (P7, 2, None, "giant_tile_kernel<2>"),                                # per-giant by an odd batch length
    (E.BASE, 1, None, "giant_tile_kernel<0>"),                            # CSR layout
], ids=["quad64", "quad128", "pair-v10", "pair-p10", "giant-v0", "giant-p7", "csr"])
def test_single_tile_kernels_every_slot(geom, layout, variant, kernel):
    """(a) one tile per launch and per block: the equal-x giant at every slot j of the chain with both signs of the centre, its thread among 0, 63, 64, 255,
    256 and T - 1"""
    dev = _open(1, variant)
    _giants_on(dev, geom)
    assert len(_run_list(dev, "single", (geom,), layout, kernel, 1)) == 2 * geom[2]
    dev.close()


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.WALK_KINDS)
def test_pair_walk_every_slot(kind):
    """(b) tile_pair_walk, elements (a, b, c, d) = (A_jl, B_jl, A_jh, B_jh): every substitution chooses between the two tiles' Py.  The equal-x giant at every
    slot in tile A, in tile B, in both (the same centre; G2[i] and -G2[i]; two slots of one thread, in one quad and in two; two threads of one block).  Both
    tiles' lists are the oracle's, and the same launches with one tile per block give the identical lists."""
    got = {}
    for tpb in (2, 1):
        dev = _open(tpb)
        _giants_on(dev, E.BASE)
        got[tpb] = _run_list(dev, "walk", (kind,), 2, "giant_pair2_kernel<2, false, true>", tpb)
        dev.close()
    assert got[1] == got[2] and len(got[2]) == (48 if kind == "two_slots" else 24)


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,kernel", [(4, "giant_pair2_kernel<2, false, true>"), (5, "giant_pair2_kernel<3, false, true>")])
def test_list_layouts(layout, kernel):
    """(c) lines + overflow list made from the reference-format image (no CSR image on the device).  The whole single-tile list -- at p = 12 every slot of the
    quad chain is a class of its own -- and, where the kernel pairs tiles, both one-sided lists of the pair walk."""
    dev = _open(1)
    _giants_on(dev, E.BASE)
    _run_list(dev, "single", (E.BASE,), layout, kernel, 1)
    dev.close()
    if layout == 4:
        dev = _open(2)
        _giants_on(dev, E.BASE)
        for kind in ("eq_random", "random_eq"):
            _run_list(dev, "walk", (kind,), layout, kernel, 2)
        dev.close()


@pytest.mark.parametrize("layout,M", [(4, 3073), (4, 4096), (5, 3 << 10)])
def test_any_bucket_kernels(layout, M):
    """(c) tables with any number of buckets, built test-side (tests/ext_table_model.py) and installed as tests/test_gpu_round6.py does: <4> (64-byte lines,
    bucket from 48 key bits), <2> by a bucket count, <3> with a bucket multiplier.  The oracle's list is o_tile_ref_ext over the table's own entries."""
    lplog = 3 if layout == 5 else 2
    lists = [("single", (E.BASE,), 1)] + ([("walk", ("eq_random",), 2), ("walk", ("random_eq",), 2)] if layout == 4 else [])
    for name, args, tpb in lists:
        dev = _open(tpb)
        _giants_on(dev, E.BASE)
        for n, bt in enumerate(E.built_list(name, *args)):
            tab = X.build_ext_table(bt.keys, M, lplog, bound_in_set=bool(n & 1), rng=np.random.default_rng(n))
            want = E.expected_ext(bt, tab["ck"], M)
            it = InstalledTable(dev, tab, len(bt.keys), M, layout)
            hits, nh, _ = dev.run(bt.case.centres, E.HIT_BUFFER)
            assert dev.last_kernel() == _kernel_name(layout, M) and dev.last_tiles_per_block() == tpb, (bt.case.name, dev.last_kernel())
            _check(bt, want, hits, nh, (bt.case.name, layout, M, tpb))
            del it
        dev.close()


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,args,tpb,kernel", [("single", (E.BASE,), 1, "giant_pair2_kernel<2, true, true>"), ("single", (P10,), 1, "giant_pair2_kernel<2, true, false>")] +
                         [("walk", (k,), 2, "giant_pair2_kernel<2, true, true>") for k in E.WALK_KINDS], ids=lambda v: str(v).replace(" ", ""))
def test_instrumented_instantiations_digest_per_thread(name, args, tpb, kernel):
    """(d) PHASE_PROBE = true is a kernel of its own: the instrumented quad chain (one tile per block and the pair walk) and, at p = 10, the instrumented pair
    chain <2, true, false>.  debug_flags & 8: every (tile, thread) of the affected block reports the xor and the wrapping sum of the keys it probed; both must
    be those of the ORACLE's keys of that thread (not merely another GPU path's), and the hit list the oracle's.  The lists of (a) at layout 2 are the p = 12
    and the p = 10 one; the p = 7 list cannot be digested -- bsgs_run_digest refuses an odd batch length, the per-giant kernel has no instrumented form."""
    cases = E.built_list(name, *args)
    geom = cases[0].case.geom
    dev = _open(tpb)
    _giants_on(dev, geom)
    for n, bt in enumerate(cases):
        gpu, want = E.expected(name, args, n)
        dev.upload_htgpu(gpu, 1 << E.HTSZ, len(bt.keys), 2)
        dg, hits, nh = dev.run_digest(bt.case.centres, E.HIT_BUFFER)
        assert dev.last_kernel() == kernel and dev.last_tiles_per_block() == tpb, (bt.case.name, dev.last_kernel())
        _check(bt, want, hits, nh, (bt.case.name, "digest", tpb))
        ref = E.thread_digests(bt)
        assert len(ref) == sum(hi - lo for lo, hi in E.thread_ranges(bt.case)) * len(bt.case.centres) >= 256
        for (tile, th), (x, s) in ref.items():
            assert (int(dg[tile, th, 0]), int(dg[tile, th, 1])) == (x, s), (bt.case.name, tile, th)
    assert len(cases) == (2 * geom[2] if name == "single" else 48 if args == ("two_slots",) else 24)
    dev.close()


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [False, True], ids=["quad", "walk"])
def test_clamped_lanes_and_partial_wave(pair):
    """(e) T = 288: the second block has 32 live threads and 224 lanes that shadow thread 287 -- they compute its batch (equal-x substitution included) and must
    report nothing.  The equal-x giant in thread 287 at a first, a middle and a last slot, in thread 0, and in the last thread of T = 32, a single partial wave.
    Every expected record exactly once: the lists are compared as lists."""
    tpb = 2 if pair else 1
    dev = _open(tpb)
    geom = None
    for n, bt in enumerate(E.built_list("clamped", pair)):
        if bt.case.geom != geom:
            geom = bt.case.geom
            _giants_on(dev, geom)
        gpu, want = E.expected("clamped", (pair,), n)
        dev.upload_htgpu(gpu, 1 << E.HTSZ, len(bt.keys), 2)
        hits, nh, _ = dev.run(bt.case.centres, E.HIT_BUFFER)
        assert dev.last_kernel() == "giant_pair2_kernel<2, false, true>" and dev.last_tiles_per_block() == tpb
        assert len(hits) == len(set(hits))
        _check(bt, want, hits, nh, (bt.case.name, tpb))
    dev.close()


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------------------------
def test_narrow_batching():
    """(f) a one-tile launch at -t 128 -b 2 -p 256 takes the narrow copy of the giants: 512 threads x 128 giants, 32 quads (bsgs_hip.hip pick_batching).  The
    equal-x giant at slots 0 .. 3 and 124 .. 127 of narrow thread 5 (wave 0, lane 5 of block 0).  fe_inv_block inverts ONE product for lane l of the block's
    four waves, so threads 5, 69, 133 and 197 share the equal-x thread's inversion: a zero or wrong batch element spoils all four.  A whole block is 65 536
    records, the hit buffer's size, so each table holds three of the four waves (wave 0 always, the case number picks the others): every case covers three of
    those four threads, the list as a whole all four (tests/test_equal_x_cases.py asserts it).  The equal-x giant itself sits in wave 0 only (the records of
    giants outside the table plus the table's 49 152 must fit the buffer: equal_x_cases.narrow_cases); lanes 5 of waves 1 .. 3 are covered as its victims."""
    import pybsgs
    dev = pybsgs.Device(0)
    dev.upload_g2(E.giants(E.NARROW)[0], *E.NARROW)
    assert dev.engine_geometry() == (256, 256)
    for n, bt in enumerate(E.built_list("narrow")):
        gpu, want = E.expected("narrow", (), n)
        dev.upload_htgpu(gpu, 1 << E.HTSZ, len(bt.keys), 2)
        hits, nh, _ = dev.run(bt.case.centres, E.HIT_BUFFER)
        assert dev.last_batching() == E.NARROW_ENGINE and dev.last_tiles_per_block() == 1              # the narrow copy
        assert dev.last_kernel() == "giant_pair2_kernel<2, false, true>"
        _check(bt, want, hits, nh, bt.case.name)
        lanes = {E.NARROW_THREAD + 64 * w for w in bt.case.waves}
        assert all((0, 2, th * 128 + j) in hits for th in lanes for j in (0, 127))
    dev.close()
