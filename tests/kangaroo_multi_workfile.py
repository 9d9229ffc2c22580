"""Reader of kangaroo.work version 3 (a search for a list of keys; DESIGN.md 10 states the layout byte by byte).  A test helper: no product code runs here."""
import struct


def read(path):
    b = open(path, "rb").read()
    assert b[:8] == b"KANGWORK"
    version, engines, herd, dp, per_thread = struct.unpack_from("<IIQII", b, 8)
    seed, rng, steps, dps, dropped, false_matches, reseeds = struct.unpack_from("<7Q", b, 32)
    elapsed, table = struct.unpack_from("<dQ", b, 88)
    w = {"version": version, "engines": engines, "herd": herd, "dp": dp, "per_thread": per_thread, "seed": seed, "rng": rng, "steps": steps, "dps": dps,
         "dropped": dropped, "false_matches": false_matches, "reseeds": reseeds, "elapsed": elapsed, "fingerprint": b[104:144].decode()}
    assert version == 3
    pos = 144
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
        j, k = struct.unpack_from("<II", b, pos)
        d = int.from_bytes(b[pos + 8:pos + 24], "little", signed=True)
        links.append((j, k, d))
        pos += 24
    entries = []
    for _ in range(table):
        x64, = struct.unpack_from("<Q", b, pos)
        d = int.from_bytes(b[pos + 8:pos + 24], "little", signed=True)
        kid, owner = struct.unpack_from("<II", b, pos + 24)
        entries.append((x64, d, kid, owner))
        pos += 32
    herds, reseed = [], []
    for _ in range(engines):
        hd = []
        for i in range(herd):
            s = b[pos + 96 * i:pos + 96 * i + 96]
            hd.append((int.from_bytes(s[:32], "little"), int.from_bytes(s[32:64], "little"), int.from_bytes(s[64:80], "little"), struct.unpack_from("<I", s, 80)[0]))
        pos += 96 * herd
        (n,) = struct.unpack_from("<I", b, pos)
        reseed.append(list(struct.unpack_from("<%dI" % n, b, pos + 4)))
        pos += 4 + 4 * n
        herds.append(hd)
    assert pos == len(b)
    w.update(keys=keys, links=links, links_kept=kept, links_resolved=resolved, entries=entries, herds=herds, reseed=reseed)
    return w
