"""Reader of a version-2 <dir>/kangaroo.work (bsgs_mi355x -kangaroo -ksym) as DESIGN.md 10 lays it out: the version-1 header, then at byte 144 the jump points
(u32), a zero (u32), the jump scale (f64) and the cycles retired (u64); the sections follow at byte 168 in the version-1 layout, a table entry's type being
0 tame, 1 wild, 3 wild with NEG.  A test helper, no product code."""
import struct

MAGIC = b"KANGWORK"
HEADER = 168


def parse(data):
    """-> dict: header fields, `entries` = [(x64, d mod 2^128, kangaroo, type)], `herds` = per engine [(x, y, d, flags)], `reseed` = per engine [index]"""
    assert len(data) >= HEADER and data[:8] == MAGIC, "not a work file"
    version, engines, herd, dp, per_thread = struct.unpack_from("<IIQII", data, 8)
    assert version == 2, "version %d" % version
    seed, rng, steps, dps, dropped, false_matches, reseeds = struct.unpack_from("<7Q", data, 32)
    (elapsed,) = struct.unpack_from("<d", data, 88)
    (table,) = struct.unpack_from("<Q", data, 96)
    jumps, zero, jumpscale, cycles = struct.unpack_from("<IIdQ", data, 144)
    assert zero == 0
    w = dict(version=version, engines=engines, herd=herd, dp=dp, per_thread=per_thread, seed=seed, rng=rng, steps=steps, dps=dps, dropped=dropped,
             false_matches=false_matches, reseeds=reseeds, elapsed=elapsed, table=table, fingerprint=data[104:144].decode("ascii"), jumps=jumps,
             jumpscale=jumpscale, cycles=cycles)
    pos = HEADER
    w["entries"] = []
    for _ in range(table):
        x64, dlo, dhi, kid, typ = struct.unpack_from("<QQQII", data, pos)
        assert typ in (0, 1, 3)
        w["entries"].append((x64, (dhi << 64) | dlo, kid, typ))
        pos += 32
    w["herds"], w["reseed"] = [], []
    for _ in range(engines):
        raw = data[pos:pos + 96 * herd]
        assert len(raw) == 96 * herd, "truncated herd"
        w["herds"].append([(int.from_bytes(raw[o:o + 32], "little"), int.from_bytes(raw[o + 32:o + 64], "little"), int.from_bytes(raw[o + 64:o + 80], "little"),
                            struct.unpack_from("<I", raw, o + 80)[0]) for o in range(0, 96 * herd, 96)])
        pos += 96 * herd
        (n,) = struct.unpack_from("<I", data, pos)
        w["reseed"].append(list(struct.unpack_from("<%dI" % n, data, pos + 4)))
        pos += 4 + 4 * n
    assert pos == len(data), "bytes after the last section"
    return w
