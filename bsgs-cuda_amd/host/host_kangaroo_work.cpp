// host_kangaroo_work.cpp -- the work file <dir>/kangaroo.work of kangaroo mode (DESIGN.md 10 states the layout byte by byte; tests/kangaroo_workfile.py and
// its -ksym and key-list siblings parse it): writer, reader and the settings fingerprints of its four versions, -selftest kangaroo-work, and the helpers the
// other -selftest kangaroo* items share.
#include "host_kangaroo.h"

using namespace kang;
namespace {
const char WORK_MAGIC[8] = {'K', 'A', 'N', 'G', 'W', 'O', 'R', 'K'};
const size_t WORK_HEADER = 144, WORK_HEADER_SYM = 168;        // versions 2 and 4: + jump points (u32), zero (u32), jump scale (f64), cycles retired (u64)
bool sym_header(uint32_t version) { return version == WORK_VERSION_SYM || version == WORK_VERSION_SYMKEYS; }
bool key_list(uint32_t version) { return version == WORK_VERSION_KEYS || version == WORK_VERSION_SYMKEYS; }
void put_header(std::vector<uint8_t> &b, const WorkHeader &h)
{
    b.assign(sym_header(h.version) ? WORK_HEADER_SYM : WORK_HEADER, 0);
    memcpy(&b[0], WORK_MAGIC, 8);
    memcpy(&b[8], &h.version, 4); memcpy(&b[12], &h.engines, 4); memcpy(&b[16], &h.herd, 8); memcpy(&b[24], &h.dp, 4); memcpy(&b[28], &h.per_thread, 4);
    memcpy(&b[32], &h.seed, 8); memcpy(&b[40], &h.rng, 8); memcpy(&b[48], &h.steps, 8); memcpy(&b[56], &h.dps, 8); memcpy(&b[64], &h.dropped, 8);
    memcpy(&b[72], &h.false_matches, 8); memcpy(&b[80], &h.reseeds, 8); memcpy(&b[88], &h.elapsed, 8); memcpy(&b[96], &h.table, 8);
    memcpy(&b[104], h.fingerprint.data(), std::min<size_t>(40, h.fingerprint.size()));
    if (sym_header(h.version)) { memcpy(&b[144], &h.jumps, 4); memcpy(&b[152], &h.jumpscale, 8); memcpy(&b[160], &h.cycles, 8); }
}
}  // namespace

// SHA-1, in the style of the BSGS fingerprint, over what a resumed run must share with the run that saved
std::string kang::kangaroo_fingerprint(const Affine &P, const Scalar &lo, const Scalar &hi, const WorkHeader &h)
{
    std::ostringstream s;
    s << hs::compress_pubkey(P) << hs::fe_to_hex(lo) << hs::fe_to_hex(hi) << "dp" << h.dp << "kn" << h.herd << "g" << h.per_thread << "e" << h.engines << "s" << h.seed;
    if (h.version == WORK_VERSION_SYM) {
        char js[40];
        snprintf(js, sizeof js, "%.17g", h.jumpscale);
        s << "sym1" << "r" << h.jumps << "js" << js;
    }
    return sha1_hex(s.str());
}
// version 3: every public key of the list in order, the range, the plan and keys<L>; version 4: plus what version 2 adds
std::string kang::keys_fingerprint(const std::vector<Affine> &P, const Scalar &lo, const Scalar &hi, const WorkHeader &h)
{
    std::ostringstream s;
    for (const Affine &p : P) s << hs::compress_pubkey(p);
    s << hs::fe_to_hex(lo) << hs::fe_to_hex(hi) << "dp" << h.dp << "kn" << h.herd << "g" << h.per_thread << "e" << h.engines << "s" << h.seed << "keys" << P.size();
    if (h.version == WORK_VERSION_SYMKEYS) {
        char js[40];
        snprintf(js, sizeof js, "%.17g", h.jumpscale);
        s << "sym1" << "r" << h.jumps << "js" << js;
    }
    return sha1_hex(s.str());
}
// written under kangaroo.temp and renamed, as save_checkpoint does
bool kang::write_work(const std::string &dst, const std::string &tmp, const WorkHeader &h, const std::vector<uint8_t> &table,
                const std::vector<const std::vector<bsgs_kangaroo_state> *> &herds, const std::vector<std::vector<uint32_t>> &reseed, const WorkKeys *keys)
{
    {
        std::ofstream f(tmp, std::ios::binary);
        if (!f) return false;
        std::vector<uint8_t> hb;
        put_header(hb, h);
        f.write((const char *)hb.data(), (std::streamsize)hb.size());
        if (keys) {                                                    // version 3: the key list's state between header and table
            std::vector<uint8_t> kb;
            const uint32_t L = (uint32_t)keys->solved.size();
            kb.insert(kb.end(), (const uint8_t *)&L, (const uint8_t *)&L + 4);
            for (uint32_t k = 0; k < L; k++) {
                kb.push_back(keys->solved[k]);
                if (keys->solved[k]) { uint8_t le[32]; hs::fe_to_le(keys->key[k], le); kb.insert(kb.end(), le, le + 32); }
            }
            const uint64_t counts[3] = {keys->kept, keys->resolved, keys->links.size()};
            kb.insert(kb.end(), (const uint8_t *)counts, (const uint8_t *)counts + 24);
            for (const WorkLink &l : keys->links) {
                uint8_t e[48];
                memcpy(e, &l.j, 4); memcpy(e + 4, &l.k, 4);
                if (h.version == WORK_VERSION_SYMKEYS) { memcpy(e + 8, &l.s1, 4); memcpy(e + 12, &l.s2, 4); memcpy(e + 16, &l.d1, 16); memcpy(e + 32, &l.d2, 16); }
                else memcpy(e + 8, &l.delta, 16);
                kb.insert(kb.end(), e, e + (h.version == WORK_VERSION_SYMKEYS ? 48 : 24));
            }
            f.write((const char *)kb.data(), (std::streamsize)kb.size());
        }
        f.write((const char *)table.data(), (std::streamsize)table.size());
        for (size_t e = 0; e < herds.size(); e++) {
            f.write((const char *)herds[e]->data(), (std::streamsize)(herds[e]->size() * sizeof(bsgs_kangaroo_state)));
            const uint32_t n = (uint32_t)reseed[e].size();
            f.write((const char *)&n, 4);
            f.write((const char *)reseed[e].data(), (std::streamsize)(4 * (size_t)n));
        }
        f.flush();
        if (!f) { remove(tmp.c_str()); return false; }
    }
    return rename(tmp.c_str(), dst.c_str()) == 0;
}
std::string kang::read_work(const std::string &path, WorkFile &w, bool with_body, uint32_t want)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return "cannot open " + path;
    const uint64_t size = (uint64_t)f.tellg();
    f.seekg(0);
    uint8_t b[WORK_HEADER];
    if (size < WORK_HEADER || !f.read((char *)b, WORK_HEADER)) return path + " is shorter than a work file's header";
    if (memcmp(b, WORK_MAGIC, 8) != 0) return path + " is not a kangaroo work file";
    uint32_t version;
    memcpy(&version, &b[8], 4);
    if (want ? version != want : (version < WORK_VERSION || version > WORK_VERSION_SYMKEYS))
        return path + " has work file version " + std::to_string(version) + ", this host reads version " + (want ? std::to_string(want) : "1, 2, 3 or 4");
    WorkHeader &h = w.h;
    h.version = version;
    uint64_t header = sym_header(version) ? WORK_HEADER_SYM : WORK_HEADER;
    if (sym_header(version)) {
        uint8_t x[WORK_HEADER_SYM - WORK_HEADER];
        uint32_t zero;
        if (size < header || !f.read((char *)x, sizeof x)) return path + " is shorter than a work file's header";
        memcpy(&h.jumps, &x[0], 4); memcpy(&zero, &x[4], 4); memcpy(&h.jumpscale, &x[8], 8); memcpy(&h.cycles, &x[16], 8);
        if (zero || h.jumps < 64 || h.jumps > BSGS_KANGAROO_SYM_MAX_JUMPS || (h.jumps & (h.jumps - 1)) || !(h.jumpscale > 0.0) || !std::isfinite(h.jumpscale))
            return path + ": header fields out of range";
    }
    memcpy(&h.engines, &b[12], 4); memcpy(&h.herd, &b[16], 8); memcpy(&h.dp, &b[24], 4); memcpy(&h.per_thread, &b[28], 4);
    memcpy(&h.seed, &b[32], 8); memcpy(&h.rng, &b[40], 8); memcpy(&h.steps, &b[48], 8); memcpy(&h.dps, &b[56], 8); memcpy(&h.dropped, &b[64], 8);
    memcpy(&h.false_matches, &b[72], 8); memcpy(&h.reseeds, &b[80], 8); memcpy(&h.elapsed, &b[88], 8); memcpy(&h.table, &b[96], 8);
    h.fingerprint.assign((const char *)&b[104], 40);
    if (h.engines > 64 || h.herd > (1ull << 26) || h.dp > 32 || h.table > (1ull << 32)) return path + ": header fields out of range";
    if (key_list(version)) {                                           // the key list's state: small, always read
        const uint64_t link_bytes = version == WORK_VERSION_SYMKEYS ? 48 : 24;
        WorkKeys &K = w.keys;
        uint32_t L = 0;
        if (header + 4 > size || !f.read((char *)&L, 4)) return path + " is truncated (key list)";
        if (!L || L > BSGS_KANGAROO_MAX_KEYS) return path + ": header fields out of range";
        header += 4;
        K.solved.assign(L, 0); K.key.assign(L, Scalar());
        for (uint32_t k = 0; k < L; k++) {
            uint8_t st = 0, le[32];
            if (header + 1 > size || !f.read((char *)&st, 1)) return path + " is truncated (key list)";
            if (st > 1) return path + ": key " + std::to_string(k) + " has status " + std::to_string(st);
            header += 1;
            if (st) {
                if (header + 32 > size || !f.read((char *)le, 32)) return path + " is truncated (key list)";
                K.key[k] = hs::fe_from_le(le);
                header += 32;
            }
            K.solved[k] = st;
        }
        uint64_t counts[3];
        if (header + 24 > size || !f.read((char *)counts, 24)) return path + " is truncated (links)";
        header += 24;
        K.kept = counts[0]; K.resolved = counts[1];
        if (counts[2] > (1ull << 32) || header + link_bytes * counts[2] > size) return path + " is truncated (links)";
        K.links.resize(counts[2]);
        for (WorkLink &l : K.links) {
            uint8_t e[48];
            if (!f.read((char *)e, (std::streamsize)link_bytes)) return path + " is truncated (links)";
            memcpy(&l.j, e, 4); memcpy(&l.k, e + 4, 4);
            if (version == WORK_VERSION_SYMKEYS) {
                l.delta = 0;
                memcpy(&l.s1, e + 8, 4); memcpy(&l.s2, e + 12, 4); memcpy(&l.d1, e + 16, 16); memcpy(&l.d2, e + 32, 16);
                if ((l.s1 != 1 && l.s1 != -1) || (l.s2 != 1 && l.s2 != -1)) return path + ": a link has a sign other than +-1";
            } else memcpy(&l.delta, e + 8, 16);
            if (l.j >= L || l.k >= L || l.j == l.k) return path + ": a link names key " + std::to_string(std::max(l.j, l.k));
        }
        header += link_bytes * counts[2];
    }
    uint64_t pos = header + 32 * h.table;
    if (pos > size) return path + " is truncated (table)";
    if (with_body) {
        w.table.resize(32 * h.table);
        if (h.table && !f.read((char *)w.table.data(), (std::streamsize)w.table.size())) return path + " is truncated (table)";
        w.herds.assign(h.engines, {}); w.reseed.assign(h.engines, {});
    }
    for (uint32_t e = 0; e < h.engines; e++) {
        if (pos + h.herd * 96 + 4 > size) return path + " is truncated (herd of engine " + std::to_string(e) + ")";
        if (with_body) {
            w.herds[e].resize(h.herd * 96);
            if (!f.read((char *)w.herds[e].data(), (std::streamsize)w.herds[e].size())) return path + " is truncated";
        } else f.seekg((std::streamoff)(pos + h.herd * 96));
        uint32_t n = 0;
        if (!f.read((char *)&n, 4)) return path + " is truncated";
        pos += h.herd * 96 + 4;
        if (n > h.herd || pos + 4ull * n > size) return path + " is truncated (re-seed list of engine " + std::to_string(e) + ")";
        if (with_body) {
            w.reseed[e].resize(n);
            if (n && !f.read((char *)w.reseed[e].data(), (std::streamsize)(4ull * n))) return path + " is truncated";
            for (uint32_t v : w.reseed[e]) if (v >= h.herd) return path + ": re-seed list names kangaroo " + std::to_string(v);
        } else f.seekg((std::streamoff)(pos + 4ull * n));
        pos += 4ull * n;
    }
    if (pos != size) return path + " has " + std::to_string(size - pos) + " bytes after its last section";
    return "";
}

bool kang::parse_pubs(const std::string &csv, std::vector<Affine> &pubs)
{
    std::stringstream ss(csv);
    std::string tok;
    while (std::getline(ss, tok, ',')) {
        Affine P;
        if (!hs::parse_pubkey(P, cut_hex(tok)) || !hs::on_curve(P)) return false;
        pubs.push_back(P);
    }
    return true;
}
bool kang::parse_range_pubs(const std::string &pk, const std::string &pke, const std::string &csv, Scalar &lo, Scalar &hi, u128 &W, std::vector<Affine> &pubs)
{
    if (!hs::fe_from_hex(lo, pk) || !hs::fe_from_hex(hi, pke)) return false;
    const Scalar w = hs::sc_sub(hi, lo);
    if (w.l[2] || w.l[3]) return false;
    W = (((u128)w.l[1] << 64) | w.l[0]) + 1;
    return parse_pubs(csv, pubs);
}
std::string kang::selftest_work_path(bool &keep)
{
    const char *named = getenv("BSGS_SELFTEST_WORK");
    keep = named != nullptr;
    if (keep) return named;
    char tmpl[] = "/tmp/kangaroo_work_XXXXXX";
    const int fd = mkstemp(tmpl);
    if (fd < 0) return "";
    close(fd);
    return tmpl;
}
std::vector<std::string> kang::split_commas(const std::string &rec)
{
    std::vector<std::string> f;
    std::stringstream ss(rec);
    std::string tok;
    while (std::getline(ss, tok, ',')) f.push_back(tok);
    return f;
}

// -selftest kangaroo-work <file> [<pk hex> <pke hex> <pubkey>]: the header of a work file, one "key value" per line, no GPU.  A file that is not a complete
// work file ends with rc 1.  A version-2 file (-ksym) prints "version", "jumps", "jumpscale" and "cycles" first; a version-3 file (-infile) "version", "keys",
// "solved", "links"; a version-4 file (-infile -kwalk sym) all seven, in that order.  With the range and the public key the settings fingerprint is recomputed from them and the header's plan: "fingerprint-check ok",
// or the resume path's refusal and rc 1.
int kangaroo_work_selftest(const std::vector<std::string> &a)
{
    if (a.size() != 1 && a.size() != 4) return 2;
    WorkFile w;
    const std::string bad = read_work(a[0], w, false, 0);
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    if (w.h.version != WORK_VERSION) printf("version %u\n", w.h.version);
    if (sym_header(w.h.version)) printf("jumps %u\njumpscale %.17g\ncycles %llu\n", w.h.jumps, w.h.jumpscale, (unsigned long long)w.h.cycles);
    if (key_list(w.h.version)) {
        uint32_t solved = 0;
        for (uint8_t st : w.keys.solved) solved += st;
        printf("keys %zu\nsolved %u\nlinks %zu\n", w.keys.solved.size(), solved, w.keys.links.size());
    }
    printf("steps %llu\ndps %llu\ntable %llu\nengines %u\nherd %llu\nfingerprint %s\nrng 0x%llx\n", (unsigned long long)w.h.steps, (unsigned long long)w.h.dps,
           (unsigned long long)w.h.table, w.h.engines, (unsigned long long)w.h.herd, w.h.fingerprint.c_str(), (unsigned long long)w.h.rng);
    if (a.size() == 4) {
        Scalar lo, hi; u128 W;
        std::vector<Affine> Ps;
        if (key_list(w.h.version)) {                                  // the public keys of the list, comma separated
            if (!parse_pubs(a[3], Ps) || !hs::fe_from_hex(lo, a[1]) || !hs::fe_from_hex(hi, a[2])) return 2;
            if (keys_fingerprint(Ps, lo, hi, w.h) != w.h.fingerprint) { fprintf(stderr, "Recovery file was made with other settings\n"); return 1; }
            printf("fingerprint-check ok\n");
            return 0;
        }
        if (!parse_range_pubs(a[1], a[2], a[3], lo, hi, W, Ps) || Ps.size() != 1) return 2;
        if (kangaroo_fingerprint(Ps[0], lo, hi, w.h) != w.h.fingerprint) { fprintf(stderr, "Recovery file was made with other settings\n"); return 1; }
        printf("fingerprint-check ok\n");
    }
    return 0;
}
