"""CPU: the image of a tame table (bsgs_kangaroo_tames_image, csrc/kangaroo_tames.hip; needs no device) byte for byte against the model
(tests/kangaroo_tames_model.py): random tags, a chain of 64 tags of one home line across 16 lines, the same chain wrapping past the last line, one entry, the
tag 0; a tag that occurs twice is refused."""
import random
import struct

import pytest

import kangaroo_tames_model as TM


def product(tags):
    import pybsgs
    return pybsgs.kangaroo_tames_image(tags)


def test_random_tags():
    rng = random.Random(1)
    tags = [rng.getrandbits(64) for _ in range(1000)]
    img, lines = product(tags)
    assert lines == TM.n_lines(1000) == 512 and img == TM.image(tags)
    L = TM.build(tags)
    assert [TM.lookup(L, t) for t in tags] == list(range(1000))
    assert all(TM.lookup(L, t ^ (1 << 63)) is None for t in tags[:100])


def test_line_counts():
    import pybsgs
    for n, want in [(1, 64), (128, 64), (129, 128), (256, 128), (257, 256), (1 << 20, 1 << 19), ((1 << 20) + 1, 1 << 20)]:
        assert TM.n_lines(n) == want
    for n in (129, 256, 257):
        assert pybsgs.kangaroo_tames_image(list(range(0, 64 * n, 64)))[1] == TM.n_lines(n)


@pytest.mark.parametrize("first_line", [5, 60])                      # 60: lines 60..63, then 0..11
def test_chain_of_one_home_line(first_line):
    tags = TM.chain_tags(first_line)
    assert len(set(tags)) == 64 and {TM.home(t, 64) for t in tags} == {first_line}
    img, lines = product(tags)
    assert lines == 64 and img == TM.image(tags)
    L = TM.build(tags)
    chain = [(first_line + k) & 63 for k in range(16)]
    assert [len(L[ln][0]) for ln in chain] == [4] * 16 and [L[ln][2] for ln in chain] == [1] * 15 + [0]
    assert sum(len(l[0]) for l in L) == 64
    assert [TM.lookup(L, t) for t in tags] == list(range(64))
    assert all(TM.lookup(L, t) is None for t in TM.chain_tags(first_line, salt=2))
    # byte layout of the first line of the chain: four tags, four entry numbers, count 4, overflowed 1, zero
    assert struct.unpack_from("<4Q4IIIQ", img, first_line * 64) == tuple(tags[:4]) + (0, 1, 2, 3, 4, 1, 0)


def test_one_entry_and_the_tag_zero():
    for tag in (0, 0xFFFFFFFFFFFFFFFF, 0x1234567890ABCDEF):
        img, lines = product([tag])
        assert lines == 64 and len(img) == 64 * 64 and img == TM.image([tag])
        assert struct.unpack_from("<4Q4IIIQ", img, TM.home(tag, 64) * 64) == (tag, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0)
    tags = [0, 64, 1]                                                 # the tag 0 next to others: told by the count, not by a sentinel
    assert product(tags)[0] == TM.image(tags) and TM.lookup(TM.build([64, 1]), 0) is None


def test_a_duplicate_tag_is_refused():
    import pybsgs
    rng = random.Random(2)
    tags = [rng.getrandbits(64) for _ in range(300)]
    for dup in ([tags[7]], [tags[299]]):
        with pytest.raises(pybsgs.BsgsError, match="share the tag"):
            product(tags + dup)
        with pytest.raises(ValueError):
            TM.build(tags + dup)
    chain = TM.chain_tags(60)                                         # the earlier entry sits 15 lines past the home line
    with pytest.raises(pybsgs.BsgsError, match="share the tag"):
        product(chain + [chain[63]])
    with pytest.raises(pybsgs.BsgsError):
        product([])
