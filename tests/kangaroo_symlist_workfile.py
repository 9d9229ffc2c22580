"""Reader of kangaroo.work version 4 (a list of keys searched with -kwalk sym; DESIGN.md 10 states the layout): the version-3 layout with the version-2 header
fields (jump points u32, a zero u32, jump scale f64, cycles retired u64) behind the fingerprint, links of 48 bytes (j u32, k u32, sigma1 i32, sigma2 i32,
d1 i128, d2 i128), NEG in bit 31 of an entry's owner word, and the key of a kangaroo in the first reserved word of its state.  A test helper: no product
code runs here."""
import struct

NEG_BIT = 1 << 31


def read(path):
    b = open(path, "rb").read()
    assert b[:8] == b"KANGWORK"
    version, engines, herd, dp, per_thread = struct.unpack_from("<IIQII", b, 8)
    seed, rng, steps, dps, dropped, false_matches, reseeds = struct.unpack_from("<7Q", b, 32)
    elapsed, table = struct.unpack_from("<dQ", b, 88)
    assert version == 4
    jumps, zero, jumpscale, cycles = struct.unpack_from("<IIdQ", b, 144)
    assert zero == 0
    w = {"version": version, "engines": engines, "herd": herd, "dp": dp, "per_thread": per_thread, "seed": seed, "rng": rng, "steps": steps, "dps": dps,
         "dropped": dropped, "false_matches": false_matches, "reseeds": reseeds, "elapsed": elapsed, "fingerprint": b[104:144].decode(), "jumps": jumps,
         "jumpscale": jumpscale, "cycles": cycles}
    pos = 168
    (L,) = struct.unpack_from("<I", b, pos)
    pos += 4
    keys = []
    for _ in range(L):
        st = b[pos]
        pos += 1
        assert st in (0, 1)
        if st:
            keys.append(int.from_bytes(b[pos:pos + 32], "little"))
            pos += 32
        else:
            keys.append(None)
    kept, resolved, nlinks = struct.unpack_from("<3Q", b, pos)
    pos += 24
    links = []
    for _ in range(nlinks):
        j, k, s1, s2 = struct.unpack_from("<IIii", b, pos)
        assert s1 in (1, -1) and s2 in (1, -1)
        links.append((j, s1, int.from_bytes(b[pos + 16:pos + 32], "little", signed=True), k, s2, int.from_bytes(b[pos + 32:pos + 48], "little", signed=True)))
        pos += 48
    entries = []
    for _ in range(table):
        x64, = struct.unpack_from("<Q", b, pos)
        d = int.from_bytes(b[pos + 8:pos + 24], "little", signed=True)
        kid, owner = struct.unpack_from("<II", b, pos + 24)
        entries.append((x64, d, kid, owner & ~NEG_BIT, bool(owner & NEG_BIT)))
        pos += 32
    herds, reseed = [], []
    for _ in range(engines):
        hd = []
        for i in range(herd):
            s = b[pos + 96 * i:pos + 96 * i + 96]
            fl, key, r1, r2 = struct.unpack_from("<4I", s, 80)
            assert r1 == 0 and r2 == 0
            hd.append((int.from_bytes(s[:32], "little"), int.from_bytes(s[32:64], "little"), int.from_bytes(s[64:80], "little"), fl, key))
        pos += 96 * herd
        (n,) = struct.unpack_from("<I", b, pos)
        reseed.append(list(struct.unpack_from("<%dI" % n, b, pos + 4)))
        pos += 4 + 4 * n
        herds.append(hd)
    assert pos == len(b)
    w.update(keys=keys, links=links, links_kept=kept, links_resolved=resolved, entries=entries, herds=herds, reseed=reseed)
    return w
