// host_kangaroo.cpp -- bsgs_mi355x -kangaroo: Pollard's kangaroo (lambda) search of ONE public key in [pk, pke] for ranges too wide for a baby table
// (include/bsgs_hip.h "Kangaroo" states the walk).  Herds of tame and wild kangaroos on every engine (-d, one engine per listed device), one
// host table of distinguished points shared by all engines and fed by a collector thread, the key written to win.txt through the JobList as the BSGS path
// writes it.  Start points come from the GPU (bsgs_kangaroo_seed; -kcpuseed: the host's comb).  The whole search is saved to <dir>/kangaroo.work every -wt
// seconds and when a run stops without the key, and -wl continues from such a file (layout and consistency rule: DESIGN.md 10).  -selftest kangaroo drives
// the table with a scripted record stream and no GPU; -selftest kangaroo-work / kangaroo-table-roundtrip do the same for the work file.
// -ksym runs the symmetric walk (the negation map; include/bsgs_hip.h "Kangaroo, symmetric walk"): offsets counted from the middle of the range, R jump points
// (-kjumps) of mean -kjumpscale * N_k sqrt(W) / 4, the collision rule with signs, cycles counted, a version-2 work file; -selftest kangaroo-sym / kangaroo-sym-roundtrip.
#include "host_kangaroo.h"

#include <csignal>
#include <random>
#include <unordered_map>

using namespace kang;
namespace {

// -ksym (tests/kangaroo_sym_model.py herd_offset): tame uniform in [0, W/2), wild uniform in [-W/4, W/4), the same stream
i128 herd_offset_sym(uint64_t &state, u128 W, bool wild)
{
    u128 r = draw128(state) % (W / 2);
    while (!wild && !r) r = draw128(state) % (W / 2);                 // a tame kangaroo at 0 would stand on the point at infinity: the next draw
    return wild ? (i128)r - (i128)(W / 4) : (i128)r;
}
// v / 2 mod n
Scalar sc_half(Scalar v)
{
    uint64_t top = 0;
    if (v.l[0] & 1) {
        unsigned __int128 c = 0;
        for (int i = 0; i < 4; i++) { c += (unsigned __int128)v.l[i] + hs::SC_N.l[i]; v.l[i] = (uint64_t)c; c >>= 64; }
        top = (uint64_t)c;
    }
    for (int i = 0; i < 3; i++) v.l[i] = (v.l[i] >> 1) | (v.l[i + 1] << 63);
    v.l[3] = (v.l[3] >> 1) | (top << 63);
    return v;
}
bool parse_hex128(const std::string &s, u128 &v)
{
    Scalar t;
    if (!hs::fe_from_hex(t, s) || t.l[2] || t.l[3]) return false;
    v = ((u128)t.l[1] << 64) | t.l[0];
    return true;
}

// the start point of a kangaroo at offset d: d*G (tame) or Q + d*G (wild)
std::vector<Affine> herd_points(const Comb &C, const Affine &Q, const std::vector<i128> &d, const std::vector<bool> &wild)
{
    std::vector<hs::Jac> j(d.size());
    for (size_t k = 0; k < d.size(); k++) {
        const bool neg = d[k] < 0;
        hs::Jac p = C.mul(neg ? (u128)-d[k] : (u128)d[k]);
        if (neg && !p.inf) p.y = hs::fe_neg(p.y);
        if (wild[k]) p = hs::jac_add_affine(p, Q);
        j[k] = p;
    }
    return hs::batch_to_affine(j);
}
bsgs_kangaroo_state to_state(const Affine &p, i128 d, bool wild)
{
    bsgs_kangaroo_state s;
    memset(&s, 0, sizeof s);
    hs::affine_to_le(p, s.x, s.y);
    memcpy(s.d, &d, 16);
    s.flags = wild ? BSGS_KANGAROO_WILD : 0u;
    return s;
}
}  // namespace

// ---- the table of distinguished points: keyed on the low 64 bits of x, shared by all engines ---------------------------------------------------------
class KangarooTable {
public:
    enum Verdict { NEW, FOUND, RESEED, FALSE_MATCH, REPEAT };
    // sym: the rule of the symmetric walk (include/bsgs_hip.h "Kangaroo, symmetric walk"; tests/kangaroo_sym_model.py SymTable)
    KangarooTable(const Scalar &a, u128 W, const Affine &P, bool sym = false) : a_(a), W_(W), P_(P), sym_(sym)
    {
        map_.reserve(1u << 20);
        mid_ = hs::sc_add(a, hs::sc_from_u128(W / 2));
        hi_ = hs::sc_add(a, hs::sc_from_u128(W - 1));
    }
    // one record: FOUND (*key = k), RESEED (the record's kangaroo follows another of its type, or died), FALSE_MATCH (tame and wild x agree in the key but the
    // difference does not solve: counted, ignored), REPEAT (the same kangaroo's own point again), NEW (stored)
    Verdict add(const uint8_t x[32], u128 d, uint32_t kid, uint32_t flags, Scalar *key)
    {
        if (flags & BSGS_KANGAROO_DEAD) { reseeds_++; if (flags & BSGS_KANGAROO_CYCLE) cycles_++; return RESEED; }
        uint64_t k64;
        memcpy(&k64, x, 8);
        if (sym_) return add_sym(k64, d, kid, flags, key);
        const bool wild = flags & BSGS_KANGAROO_WILD;
        auto it = map_.find(k64);
        if (it == map_.end()) { map_.emplace(k64, Entry{d, kid, wild, false}); return NEW; }
        const Entry &e = it->second;
        if (e.wild == wild) {
            if (e.kid == kid) return REPEAT;
            reseeds_++;
            return RESEED;
        }
        const i128 k = (i128)(wild ? e.d - d : d - e.d);
        if (k >= 0 && (u128)k < W_) {
            const Scalar cand = hs::sc_add(a_, hs::sc_from_u128((u128)k));
            const Affine q = hs::point_mul(hs::G, cand);
            if (!q.inf && hs::fe_equal(q.x, P_.x) && hs::fe_equal(q.y, P_.y)) { *key = cand; return FOUND; }
        }
        false_++;
        return FALSE_MATCH;
    }
    size_t size() const { return map_.size(); }
    uint64_t false_matches() const { return false_; }
    uint64_t reseeds() const { return reseeds_; }
    uint64_t cycles() const { return cycles_; }
    void set_cycles(uint64_t c) { cycles_ = c; }
    // the work file's view: one 32-byte entry per stored point -- low 64 bits of x, d, kangaroo, type (0 tame, 1 wild) -- and the two counters
    void write_entries(std::vector<uint8_t> &out) const
    {
        for (const auto &kv : map_) {
            uint8_t e[32];
            const uint32_t type = (kv.second.wild ? 1u : 0u) | (kv.second.neg ? 2u : 0u);       // (version 2: 3 = a wild kangaroo with NEG)
            memcpy(e, &kv.first, 8); memcpy(e + 8, &kv.second.d, 16); memcpy(e + 24, &kv.second.kid, 4); memcpy(e + 28, &type, 4);
            out.insert(out.end(), e, e + 32);
        }
    }
    bool restore(const uint8_t *entries, uint64_t n, uint64_t false_matches, uint64_t reseeds)
    {
        for (uint64_t i = 0; i < n; i++) {
            const uint8_t *e = entries + 32 * i;
            uint64_t k64; Entry en; uint32_t type;
            memcpy(&k64, e, 8); memcpy(&en.d, e + 8, 16); memcpy(&en.kid, e + 24, 4); memcpy(&type, e + 28, 4);
            if (type > 1u && !(sym_ && type == 3u)) return false;
            en.wild = type & 1u; en.neg = type == 3u;
            if (!map_.emplace(k64, en).second) return false;
        }
        false_ = false_matches; reseeds_ = reseeds;
        return true;
    }
private:
    struct Entry { u128 d; uint32_t kid; bool wild, neg; };
    // a record's point is sigma Q + d G, sigma = 0 tame, +1 wild, -1 wild with NEG; equal x: sigma1 Q + d1 G = +-(sigma2 Q + d2 G), so for each sign with
    // sigma1 -+ sigma2 != 0 the candidate is k'' = (+-d2 - d1) / (sigma1 -+ sigma2) mod n (the divisor is +-1 or +-2), the key a + W/2 + k''
    Verdict add_sym(uint64_t k64, u128 d, uint32_t kid, uint32_t flags, Scalar *key)
    {
        const bool wild = flags & BSGS_KANGAROO_WILD, neg = wild && (flags & BSGS_KANGAROO_NEG);
        auto it = map_.find(k64);
        if (it == map_.end()) { map_.emplace(k64, Entry{d, kid, wild, neg}); return NEW; }
        const Entry &e = it->second;
        if (e.kid == kid) return REPEAT;
        const int s1 = e.wild ? (e.neg ? -1 : 1) : 0, s2 = wild ? (neg ? -1 : 1) : 0;
        const Scalar d1 = sc_from_i128((i128)e.d), d2 = sc_from_i128((i128)d);
        bool tried = false;
        for (int sign = 1; sign >= -1; sign -= 2) {
            const int den = s1 - sign * s2;
            if (!den) continue;
            tried = true;
            Scalar k = hs::sc_sub(sign > 0 ? d2 : hs::sc_neg(d2), d1);
            if (den == 2 || den == -2) k = sc_half(k);
            if (den < 0) k = hs::sc_neg(k);
            const Scalar cand = hs::sc_add(mid_, k);
            if (hs::fe_cmp(cand, a_) < 0 || hs::fe_cmp(cand, hi_) > 0) continue;
            const Affine q = hs::point_mul(hs::G, cand);
            if (!q.inf && hs::fe_equal(q.x, P_.x) && hs::fe_equal(q.y, P_.y)) { *key = cand; return FOUND; }
        }
        if (tried) false_++;
        reseeds_++;
        return RESEED;
    }
    const Scalar a_;
    const u128 W_;
    const Affine P_;
    const bool sym_;
    Scalar mid_, hi_;
    std::unordered_map<uint64_t, Entry> map_;
    uint64_t false_ = 0, reseeds_ = 0, cycles_ = 0;
};

// ---- the work file <dir>/kangaroo.work (DESIGN.md 10 states the layout byte by byte; tests/test_kangaroo_work.py parses it) -------------------------
namespace {
const char WORK_MAGIC[8] = {'K', 'A', 'N', 'G', 'W', 'O', 'R', 'K'};
const size_t WORK_HEADER = 144, WORK_HEADER_SYM = 168;        // version 2: + jump points (u32), zero (u32), jump scale (f64), cycles retired (u64)
// SHA-1, in the style of the BSGS fingerprint, over what a resumed run must share with the run that saved
std::string kangaroo_fingerprint(const Affine &P, const Scalar &lo, const Scalar &hi, const WorkHeader &h)
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
void put_header(std::vector<uint8_t> &b, const WorkHeader &h)
{
    b.assign(h.version == WORK_VERSION_SYM ? WORK_HEADER_SYM : WORK_HEADER, 0);
    memcpy(&b[0], WORK_MAGIC, 8);
    memcpy(&b[8], &h.version, 4); memcpy(&b[12], &h.engines, 4); memcpy(&b[16], &h.herd, 8); memcpy(&b[24], &h.dp, 4); memcpy(&b[28], &h.per_thread, 4);
    memcpy(&b[32], &h.seed, 8); memcpy(&b[40], &h.rng, 8); memcpy(&b[48], &h.steps, 8); memcpy(&b[56], &h.dps, 8); memcpy(&b[64], &h.dropped, 8);
    memcpy(&b[72], &h.false_matches, 8); memcpy(&b[80], &h.reseeds, 8); memcpy(&b[88], &h.elapsed, 8); memcpy(&b[96], &h.table, 8);
    memcpy(&b[104], h.fingerprint.data(), std::min<size_t>(40, h.fingerprint.size()));
    if (h.version == WORK_VERSION_SYM) { memcpy(&b[144], &h.jumps, 4); memcpy(&b[152], &h.jumpscale, 8); memcpy(&b[160], &h.cycles, 8); }
}
// written under kangaroo.temp and renamed, as save_checkpoint does; herds by pointer: they are the large part
bool write_work(const std::string &dst, const std::string &tmp, const WorkHeader &h, const std::vector<uint8_t> &table,
                const std::vector<const std::vector<bsgs_kangaroo_state> *> &herds, const std::vector<std::vector<uint32_t>> &reseed, const WorkKeys *keys = nullptr)
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
                uint8_t e[24];
                memcpy(e, &l.j, 4); memcpy(e + 4, &l.k, 4); memcpy(e + 8, &l.delta, 16);
                kb.insert(kb.end(), e, e + 24);
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
// "" when the file is a complete work file of version `want` (0: of either version), else what is wrong with it; with_body = false reads the header and checks
// the sections' sizes only
std::string read_work(const std::string &path, WorkFile &w, bool with_body, uint32_t want = WORK_VERSION)
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
    if (want ? version != want : (version != WORK_VERSION && version != WORK_VERSION_SYM && version != WORK_VERSION_KEYS))
        return path + " has work file version " + std::to_string(version) + ", this host reads version " + (want ? std::to_string(want) : "1, 2 or 3");
    WorkHeader &h = w.h;
    h.version = version;
    uint64_t header = version == WORK_VERSION_SYM ? WORK_HEADER_SYM : WORK_HEADER;
    if (version == WORK_VERSION_SYM) {
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
    if (version == WORK_VERSION_KEYS) {                                // the key list's state: small, always read
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
        if (counts[2] > (1ull << 32) || header + 24 * counts[2] > size) return path + " is truncated (links)";
        K.links.resize(counts[2]);
        for (WorkLink &l : K.links) {
            uint8_t e[24];
            if (!f.read((char *)e, 24)) return path + " is truncated (links)";
            memcpy(&l.j, e, 4); memcpy(&l.k, e + 4, 4); memcpy(&l.delta, e + 8, 16);
            if (l.j >= L || l.k >= L || l.j == l.k) return path + ": a link names key " + std::to_string(std::max(l.j, l.k));
        }
        header += 24 * counts[2];
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
bool parse_range_pub(const std::string &pk, const std::string &pke, const std::string &pub, Scalar &lo, Scalar &hi, Affine &P, u128 &W)
{
    if (!hs::fe_from_hex(lo, pk) || !hs::fe_from_hex(hi, pke) || !hs::parse_pubkey(P, cut_hex(pub)) || !hs::on_curve(P)) return false;
    const Scalar w = hs::sc_sub(hi, lo);
    if (w.l[2] || w.l[3]) return false;
    W = (((u128)w.l[1] << 64) | w.l[0]) + 1;
    return true;
}
// one scripted record (T|W|D,<x hex>,<d hex>,<kangaroo>; sym: also N, a wild kangaroo with NEG, and C, a cycle's dead record) into the table: prints the
// verdict line of -selftest kangaroo
bool scripted_record(KangarooTable &tab, const std::string &rec, bool sym = false)
{
    std::vector<std::string> f;
    std::stringstream ss(rec);
    std::string tok;
    while (std::getline(ss, tok, ',')) f.push_back(tok);
    if (f.size() != 4 || f[0].size() != 1 || !strchr(sym ? "TWDNC" : "TWD", f[0][0])) return false;
    Scalar x;
    u128 d;
    if (!hs::fe_from_hex(x, f[1]) || !parse_hex128(f[2], d)) return false;
    uint8_t xb[32];
    hs::fe_to_le(x, xb);
    const uint32_t flags = f[0] == "W" ? BSGS_KANGAROO_WILD : f[0] == "D" ? BSGS_KANGAROO_DEAD : f[0] == "N" ? BSGS_KANGAROO_WILD | BSGS_KANGAROO_NEG :
                           f[0] == "C" ? BSGS_KANGAROO_DEAD | BSGS_KANGAROO_CYCLE : 0u;
    Scalar key;
    switch (tab.add(xb, d, (uint32_t)strtoul(f[3].c_str(), nullptr, 10), flags, &key)) {
    case KangarooTable::NEW: printf("new\n"); break;
    case KangarooTable::FOUND: printf("found %s\n", hs::fe_to_hex(key).c_str()); break;
    case KangarooTable::RESEED: printf("reseed %s\n", f[3].c_str()); break;
    case KangarooTable::FALSE_MATCH: printf("false\n"); break;
    case KangarooTable::REPEAT: printf("repeat\n"); break;
    }
    return true;
}
}  // namespace

bool kang::write_work_file(const std::string &dst, const std::string &tmp, const WorkHeader &h, const std::vector<uint8_t> &table,
                           const std::vector<const std::vector<bsgs_kangaroo_state> *> &herds, const std::vector<std::vector<uint32_t>> &reseed, const WorkKeys *keys)
{
    return write_work(dst, tmp, h, table, herds, reseed, keys);
}
std::string kang::read_work_file(const std::string &path, WorkFile &w, bool with_body, uint32_t want) { return read_work(path, w, with_body, want); }
// version 3: every public key of the list in order, the range, the plan and keys<L>
std::string kang::keys_fingerprint(const std::vector<Affine> &P, const Scalar &lo, const Scalar &hi, const WorkHeader &h)
{
    std::ostringstream s;
    for (const Affine &p : P) s << hs::compress_pubkey(p);
    s << hs::fe_to_hex(lo) << hs::fe_to_hex(hi) << "dp" << h.dp << "kn" << h.herd << "g" << h.per_thread << "e" << h.engines << "s" << h.seed << "keys" << P.size();
    return sha1_hex(s.str());
}

// -selftest kangaroo <pk hex> <pke hex> <pubkey> <record>...  record = T|W|D,<x hex>,<d hex: 128-bit two's complement>,<kangaroo> (D: a dead record).
// Prints one line per record: "new", "found <key hex>", "reseed <kangaroo>", "false", "repeat"; then "summary <stored> <false matches> <reseeds>".
int kangaroo_selftest(const std::vector<std::string> &a)
{
    if (a.size() < 3) return 2;
    Scalar lo, hi; Affine P; u128 W;
    if (!parse_range_pub(a[0], a[1], a[2], lo, hi, P, W)) return 2;
    KangarooTable tab(lo, W, P);
    for (size_t i = 3; i < a.size(); i++) if (!scripted_record(tab, a[i])) return 2;
    printf("summary %zu %llu %llu\n", tab.size(), (unsigned long long)tab.false_matches(), (unsigned long long)tab.reseeds());
    return 0;
}

// -selftest kangaroo-sym <pk hex> <pke hex> <pubkey> <record>...: as -selftest kangaroo through the symmetric table (record types T, W, N, D, C); the summary
// line is "summary <stored> <false matches> <reseeds> <cycles>".
int kangaroo_sym_selftest(const std::vector<std::string> &a)
{
    if (a.size() < 3) return 2;
    Scalar lo, hi; Affine P; u128 W;
    if (!parse_range_pub(a[0], a[1], a[2], lo, hi, P, W)) return 2;
    KangarooTable tab(lo, W, P, true);
    for (size_t i = 3; i < a.size(); i++) if (!scripted_record(tab, a[i], true)) return 2;
    printf("summary %zu %llu %llu %llu\n", tab.size(), (unsigned long long)tab.false_matches(), (unsigned long long)tab.reseeds(), (unsigned long long)tab.cycles());
    return 0;
}

// -selftest kangaroo-work <file> [<pk hex> <pke hex> <pubkey>]: the header of a work file, one "key value" per line, no GPU.  A file that is not a complete
// work file ends with rc 1.  A version-2 file (-ksym) prints "version", "jumps", "jumpscale" and "cycles" first.  With the range and the public key the settings fingerprint is recomputed from them and the header's plan: "fingerprint-check ok",
// or the resume path's refusal and rc 1.
int kangaroo_work_selftest(const std::vector<std::string> &a)
{
    if (a.size() != 1 && a.size() != 4) return 2;
    WorkFile w;
    const std::string bad = read_work(a[0], w, false, 0);
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    if (w.h.version == WORK_VERSION_SYM)
        printf("version %u\njumps %u\njumpscale %.17g\ncycles %llu\n", w.h.version, w.h.jumps, w.h.jumpscale, (unsigned long long)w.h.cycles);
    if (w.h.version == WORK_VERSION_KEYS) {
        uint32_t solved = 0;
        for (uint8_t st : w.keys.solved) solved += st;
        printf("version %u\nkeys %zu\nsolved %u\nlinks %zu\n", w.h.version, w.keys.solved.size(), solved, w.keys.links.size());
    }
    printf("steps %llu\ndps %llu\ntable %llu\nengines %u\nherd %llu\nfingerprint %s\nrng 0x%llx\n", (unsigned long long)w.h.steps, (unsigned long long)w.h.dps,
           (unsigned long long)w.h.table, w.h.engines, (unsigned long long)w.h.herd, w.h.fingerprint.c_str(), (unsigned long long)w.h.rng);
    if (a.size() == 4) {
        Scalar lo, hi; Affine P; u128 W;
        if (w.h.version == WORK_VERSION_KEYS) {                       // the public keys of the list, comma separated
            std::vector<Affine> Ps;
            std::stringstream ss(a[3]);
            std::string tok;
            while (std::getline(ss, tok, ',')) { if (!hs::parse_pubkey(P, cut_hex(tok)) || !hs::on_curve(P)) return 2; Ps.push_back(P); }
            if (!hs::fe_from_hex(lo, a[1]) || !hs::fe_from_hex(hi, a[2])) return 2;
            if (keys_fingerprint(Ps, lo, hi, w.h) != w.h.fingerprint) { fprintf(stderr, "Recovery file was made with other settings\n"); return 1; }
            printf("fingerprint-check ok\n");
            return 0;
        }
        if (!parse_range_pub(a[1], a[2], a[3], lo, hi, P, W)) return 2;
        if (kangaroo_fingerprint(P, lo, hi, w.h) != w.h.fingerprint) { fprintf(stderr, "Recovery file was made with other settings\n"); return 1; }
        printf("fingerprint-check ok\n");
    }
    return 0;
}

// -selftest kangaroo-table-roundtrip <pk hex> <pke hex> <pubkey> <split> <record>...: the first <split> records into a table, the table into a work file
// without herds (a temporary file; BSGS_SELFTEST_WORK names a path to write and keep instead), the file into a fresh table, the other records into that one.
// Prints what -selftest kangaroo prints for the undivided stream.
static int roundtrip_selftest(const std::vector<std::string> &a, bool sym);
int kangaroo_roundtrip_selftest(const std::vector<std::string> &a) { return roundtrip_selftest(a, false); }
// -selftest kangaroo-sym-roundtrip: the same through the symmetric table and a version-2 file (1024 jump points, jump scale 1); summary as -selftest kangaroo-sym
int kangaroo_sym_roundtrip_selftest(const std::vector<std::string> &a) { return roundtrip_selftest(a, true); }
static int roundtrip_selftest(const std::vector<std::string> &a, bool sym)
{
    if (a.size() < 4) return 2;
    Scalar lo, hi; Affine P; u128 W;
    if (!parse_range_pub(a[0], a[1], a[2], lo, hi, P, W)) return 2;
    const size_t split = (size_t)strtoull(a[3].c_str(), nullptr, 10);
    if (split > a.size() - 4) return 2;
    const char *keep = getenv("BSGS_SELFTEST_WORK");
    std::string path = keep ? keep : "";
    if (!keep) {
        char tmpl[] = "/tmp/kangaroo_work_XXXXXX";
        const int fd = mkstemp(tmpl);
        if (fd < 0) return 2;
        close(fd);
        path = tmpl;
    }
    {
        KangarooTable first(lo, W, P, sym);
        for (size_t i = 0; i < split; i++) if (!scripted_record(first, a[4 + i], sym)) return 2;
        WorkHeader h;
        if (sym) { h.version = WORK_VERSION_SYM; h.jumps = 1024; h.jumpscale = 1.0; h.cycles = first.cycles(); }
        std::vector<uint8_t> entries;
        first.write_entries(entries);
        h.table = first.size(); h.false_matches = first.false_matches(); h.reseeds = first.reseeds();
        for (size_t i = 0; i < split; i++) if (a[4 + i][0] != 'D' && a[4 + i][0] != 'C') h.dps++;
        h.fingerprint = kangaroo_fingerprint(P, lo, hi, h);
        if (!write_work(path, path + ".temp", h, entries, {}, {})) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
    }
    WorkFile w;
    const std::string bad = read_work(path, w, true, sym ? WORK_VERSION_SYM : WORK_VERSION);
    if (!keep) remove(path.c_str());
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    KangarooTable second(lo, W, P, sym);
    if (!second.restore(w.table.data(), w.h.table, w.h.false_matches, w.h.reseeds)) { fprintf(stderr, "the table section does not load\n"); return 1; }
    second.set_cycles(w.h.cycles);
    for (size_t i = 4 + split; i < a.size(); i++) if (!scripted_record(second, a[i], sym)) return 2;
    if (sym) printf("summary %zu %llu %llu %llu\n", second.size(), (unsigned long long)second.false_matches(), (unsigned long long)second.reseeds(), (unsigned long long)second.cycles());
    else printf("summary %zu %llu %llu\n", second.size(), (unsigned long long)second.false_matches(), (unsigned long long)second.reseeds());
    return 0;
}

namespace {
const double KSYM_JUMPSCALE = 2.0;                 // DESIGN.md 10, "jump scale": the best of the measured sweep
}  // namespace

KangConfig kang::parse_kangaroo_args(int argc, char **argv)
{
    KangConfig c;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        for (auto &ch : a) ch = (char)tolower(ch);
        auto next = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
        if (a == "-kangaroo") continue;
        else if (a == "-h") { usage(Config()); exit(0); }
        else if (a == "-pb") { c.pub = cut_hex(next()); c.pub_given = true; }
        else if (a == "-infile") c.infile = next();
        else if (a == "-pk") c.pk = cut_hex(next());
        else if (a == "-pke") c.pke = cut_hex(next());
        else if (a == "-d") c.devices = next();
        else if (a == "-dir") c.dir = next();
        else if (a == "-dp") { c.dp = atoi(next().c_str()); if (c.dp < 0 || c.dp > 32) die("-dp must be 0..32"); }
        else if (a == "-kn") c.kn = strtoull(next().c_str(), nullptr, 10);
        else if (a == "-kseed") { c.seed = strtoull(next().c_str(), nullptr, 0); c.seed_given = true; }
        else if (a == "-wl") c.wl = next();
        else if (a == "-wt") c.wt = std::max(30, atoi(next().c_str()));
        else if (a == "-ksteps") { c.ksteps = strtoull(next().c_str(), nullptr, 10); if (!c.ksteps) die("-ksteps must be at least 1"); }
        else if (a == "-kcpuseed") c.cpuseed = true;
        else if (a == "-ksym") c.sym = true;
        else if (a == "-kjumps") { c.jumps = (uint32_t)strtoul(next().c_str(), nullptr, 10); if (c.jumps < 64 || c.jumps > BSGS_KANGAROO_SYM_MAX_JUMPS || (c.jumps & (c.jumps - 1))) die("-kjumps must be a power of two, 64..4096"); }
        else if (a == "-kjumpscale") { c.jumpscale = atof(next().c_str()); if (!(c.jumpscale >= 1.0 / 64 && c.jumpscale <= 64.0)) die("-kjumpscale must be 1/64..64"); }
        else if (a == "-w" || a == "-htsz" || a == "-onlygen") die("-kangaroo cannot be combined with " + a + " (no baby table)");
        else die("Unknown parameter with -kangaroo: " + a);
    }
    if (!c.sym && (c.jumps || c.jumpscale != 0.0)) die("-kjumps and -kjumpscale belong to -ksym");
    if (!c.infile.empty()) {
        if (c.pub_given) die("-kangaroo: -pb and -infile exclude each other (the keys come from the file)");
        if (c.sym) die("-kangaroo -ksym cannot be combined with -infile: the symmetric walk keeps its last jump index in the flag bits that carry the key of a wild kangaroo, and its collision rule across keys is not built");
    }
    return c;
}

Plan kang::plan_herd(double sqrtW, uint32_t engines, int cus, int dp_arg, uint64_t kn_arg)
{
    Plan pl;
    pl.engines = engines;
    pl.dp = dp_arg >= 0 ? (uint32_t)dp_arg : (uint32_t)std::min(32.0, std::max(0.0, std::ceil(std::log2(2.0 * sqrtW / 33554432.0))));
    const uint64_t full = (uint64_t)cus * 1024 * 16;
    uint64_t kn = kn_arg ? kn_arg : (uint64_t)std::min((double)full, sqrtW / 8.0 / std::ldexp(1.0, (int)pl.dp) / pl.engines);
    kn = std::max<uint64_t>(kn, 64);
    pl.G = 16;                                                        // fewer kangaroos per thread only while the GPU would have less than two waves per SIMD
    while (pl.G > 1 && kn / pl.G < (uint64_t)cus * 512) pl.G /= 2;
    pl.kn = std::max<uint64_t>(64ull * pl.G, kn / (64ull * pl.G) * (64ull * pl.G));
    pl.S = pl.cap = 0; pl.expected = 0.0;
    return pl;
}

namespace {

// what the engines, the collector and the saver share
struct Shared {
    std::atomic<bool> stop{false}, found{false};
    std::atomic<uint64_t> steps{0}, dps{0}, dropped{0};
    std::mutex rng_m;
    uint64_t rng = 0;                              // the seeded stream: initial herds in engine order, then every re-seed
    std::mutex q_m; std::condition_variable q_cv;
    std::deque<std::pair<uint32_t, std::vector<bsgs_kangaroo_record>>> queue;     // (engine, records of one launch)
    bool collector_busy = false;                   // (under q_m) a batch has left the queue and is not in the table yet
    std::vector<std::unique_ptr<std::mutex>> reseed_m;
    std::vector<std::vector<uint32_t>> reseed;     // per engine: kangaroos (local index) to start afresh
    std::vector<uint64_t> engine_records;
    std::mutex err_m; std::string err;
    Scalar key;
    // saving ("a save is a consistent cut"): engines park between two launches with their herd downloaded
    std::atomic<bool> save_req{false};
    std::mutex save_m; std::condition_variable save_cv;
    uint32_t parked = 0, running = 0;              // (under save_m) engines waiting for the save to end / engine threads alive
    std::vector<std::vector<bsgs_kangaroo_state>> saved;      // per engine: the herd as downloaded at the last park or at the end
};

volatile sig_atomic_t signalled = 0;
void on_signal(int) { signalled = 1; }
}  // namespace

int kangaroo_main(int argc, char **argv)
{
    printf("BSGS MI355X kangaroo mode on %s\n", bsgs_version());
    const KangConfig c = parse_kangaroo_args(argc, argv);
    if (!c.infile.empty()) return kangaroo_multi_main(c);
    Affine P;
    if (!hs::parse_pubkey(P, c.pub) || !hs::on_curve(P)) die("Invalid Public Key (-pb) length!!!");
    Scalar lo, hi;
    if (!hs::fe_from_hex(lo, c.pk) || hs::fe_is_zero(lo)) die("Start range can`t be zero");
    if (!hs::fe_from_hex(hi, c.pke)) die("Invalid range (-pkend) length!!!");
    if (hs::fe_cmp(hi, lo) <= 0) die("End range must be more then start range");
    const Scalar wm1 = hs::sc_sub(hi, lo);
    if (wm1.l[2] || wm1.l[3] || (wm1.l[1] >> 61)) die("-kangaroo: the range width must be at most 2^125");
    const u128 W = (((u128)wm1.l[1] << 64) | wm1.l[0]) + 1;
    if (W < ((u128)1 << 20)) die("-kangaroo: the range width must be at least 2^20");
    const double Wd = (double)W, sqrtW = std::sqrt(Wd);
    // -wl: the work file is read before any device is looked for; a file that is missing or is not a kangaroo work file ends the run here
    const bool resume = !c.wl.empty();
    WorkFile wf;
    std::string wl_path = c.wl;
    if (resume) {
        struct stat sb;
        if (stat(wl_path.c_str(), &sb) != 0 && stat((c.dir + "/" + c.wl).c_str(), &sb) == 0) wl_path = c.dir + "/" + c.wl;
        const std::string bad = read_work(wl_path, wf, true, c.sym ? WORK_VERSION_SYM : WORK_VERSION);
        if (!bad.empty()) die("-kangaroo -wl: " + bad + " (only a kangaroo.work file can be resumed here; a BSGS recovery file is not supported in kangaroo mode)");
        // the settings: what the command line names must be what the file was made with, and the rest is taken from the file
        std::vector<std::string> dl;
        { std::stringstream ss(c.devices); std::string tok; while (std::getline(ss, tok, ',')) dl.push_back(tok); }
        if (kangaroo_fingerprint(P, lo, hi, wf.h) != wf.h.fingerprint || (c.dp >= 0 && (uint32_t)c.dp != wf.h.dp) || (c.kn && c.kn != wf.h.herd) ||
            (c.seed_given && c.seed != wf.h.seed) || (c.jumps && c.jumps != wf.h.jumps) || (c.jumpscale != 0.0 && c.jumpscale != wf.h.jumpscale) || (!dl.empty() && dl.size() != wf.h.engines) || !wf.h.engines || !wf.h.herd || !wf.h.per_thread ||
            wf.h.herd % (64ull * wf.h.per_thread))
            die("Recovery file was made with other settings");
    }
    printf("Kangaroo range [%s, %s], width 2^%.2f\n", hs::fe_to_hex(lo).c_str(), hs::fe_to_hex(hi).c_str(), std::log2(Wd));
    // -ksym: offsets are counted from the middle of the range, k'' = k - (a + W/2) (include/bsgs_hip.h "Kangaroo, symmetric walk")
    const Scalar base = c.sym ? hs::sc_add(lo, hs::sc_from_u128(W / 2)) : lo;
    const Affine Q = hs::point_add(P, hs::affine_neg(hs::point_mul(hs::G, base)));
    JobList jobs({c.pub}, Recovery(), c.dir, [](int, const std::string &, const Scalar &) {});      // win.txt as the BSGS path writes it
    { Config rc; rc.dir = c.dir; read_recovery(rc); }                                                  // (win.txt starts empty, as there: the key was not found yet)
    jobs.open_lanes(1);
    JobList::Claim cl;
    jobs.claim(0, cl);
    printf("\nFindpubkey  : %s\n", hs::compress_pubkey(P).c_str());

    // engines
    std::vector<int> gpus;
    {
        int ngpu = 0;
        CK(bsgs_dev_count(&ngpu));
        if (ngpu <= 0) die("No GPU found");
        if (c.devices.empty()) for (int i = 0; i < ngpu; i++) gpus.push_back(i);
        else { std::stringstream ss(c.devices); std::string tok; while (std::getline(ss, tok, ',')) gpus.push_back(atoi(tok.c_str())); }
    }
    if (resume && gpus.size() != wf.h.engines) die("Recovery file was made with other settings");
    int cus = 256;
    { bsgs_dev *d = nullptr; CK(bsgs_dev_open(gpus[0], &d)); bsgs_dev_cu_count(d, &cus); bsgs_dev_close(d); }
    // defaults from W: expected DPs (2 sqrt(W) / 2^dp) within 2^25 host entries, DP overhead N_k 2^dp at most sqrt(W) / 8, a full herd is 16 kangaroos
    // per thread at four waves per SIMD (one batch inversion per block costs about 70 multiplications per thread: 16 kangaroos share it)
    Plan pl = plan_herd(sqrtW, (uint32_t)gpus.size(), cus, resume ? (int)wf.h.dp : c.dp, c.kn);
    uint64_t kn = pl.kn;
    if (resume) { kn = wf.h.herd; pl.G = wf.h.per_thread; }          // the plan of the run that saved, not this GPU's
    if (kn > (1ull << 26)) die("-kn: at most 2^26 kangaroos per engine");
    pl.kn = kn;
    const double Nk = (double)kn * pl.engines;
    pl.expected = 2.0 * sqrtW + Nk * std::ldexp(1.0, (int)pl.dp);
    pl.S = (uint32_t)std::max(c.sym ? 2.0 * BSGS_KANGAROO_CYCLE_WINDOW : 8.0, std::min(1024.0, pl.expected / Nk / 8.0));   // -ksym: a launch longer than the cycle window
    const double per_launch = Nk / pl.engines * pl.S / std::ldexp(1.0, (int)pl.dp);
    pl.cap = (uint32_t)std::min<double>(1u << 22, 2.0 * per_launch + 65536.0);
    uint64_t seed = c.seed;
    if (resume) seed = wf.h.seed;
    else if (!c.seed_given) { std::random_device rd; seed = ((uint64_t)rd() << 32) ^ rd(); }
    printf("Kangaroo: %u engine(s) x %llu kangaroos (%u per thread), -dp %u, %u steps per launch, -kseed 0x%llx\n", pl.engines, (unsigned long long)kn, pl.G, pl.dp, pl.S,
           (unsigned long long)seed);
    printf("Expected steps: 2^%.2f (2 sqrt(W) + DP overhead), expected DPs 2^%.2f\n", std::log2(pl.expected), std::log2(2.0 * sqrtW / std::ldexp(1.0, (int)pl.dp) + 1.0));
    if (c.dp < 0 && 2.0 * sqrtW / std::ldexp(1.0, (int)pl.dp) > 67108864.0) printf("WARNING: the expected DP count exceeds 2^26 host entries even at -dp 32\n");
    WorkHeader wh;                                                     // what every save of this run shares
    wh.engines = pl.engines; wh.dp = pl.dp; wh.per_thread = pl.G; wh.herd = kn; wh.seed = seed;
    if (c.sym) {
        wh.version = WORK_VERSION_SYM;
        wh.jumps = resume ? wf.h.jumps : c.jumps ? c.jumps : 1024u;
        wh.jumpscale = resume ? wf.h.jumpscale : c.jumpscale != 0.0 ? c.jumpscale : KSYM_JUMPSCALE;
        printf("Kangaroo: symmetric walk (negation map), %u jump points, jump scale %g\n", wh.jumps, wh.jumpscale);
    }
    wh.fingerprint = kangaroo_fingerprint(P, lo, hi, wh);
    const std::string work_path = c.dir + "/kangaroo.work", work_tmp = c.dir + "/kangaroo.temp";

    // jump table: s_j uniform in [1, 2m), mean m = N_k sqrt(W) / 4 (at most 2^62): a function of the seed and the plan, never saved
    Shared sh;
    sh.rng = seed;
    const double mean = std::max(1.0, std::min(std::ldexp(1.0, 62), (c.sym ? wh.jumpscale : 1.0) * Nk * sqrtW / 4.0));
    const int njumps = c.sym ? (int)wh.jumps : BSGS_KANGAROO_JUMPS;
    std::vector<uint64_t> js(njumps);
    std::vector<uint8_t> jxy(64 * (size_t)njumps);
    for (int j = 0; j < njumps; j++) {
        const uint64_t span = (uint64_t)(2.0 * mean) > 1 ? (uint64_t)(2.0 * mean) - 1 : 1;
        js[j] = 1 + splitmix64(sh.rng) % span;
        const Affine J = hs::point_mul(hs::G, hs::fe_from_u64(js[j]));
        hs::affine_to_le(J, &jxy[64 * j], &jxy[64 * j + 32]);
    }
    // the host's comb: -kcpuseed, and Q at infinity (the key is -pk itself: no affine Q to hand to the kernel; the host's additions take it as it is)
    const bool cpuseed = c.cpuseed || Q.inf;
    std::unique_ptr<Comb> comb;
    if (cpuseed) comb.reset(new Comb());
    uint8_t qxy[64];
    hs::affine_to_le(Q, qxy, qxy + 32);
    sh.reseed.resize(pl.engines);
    sh.saved.resize(pl.engines);
    sh.engine_records.assign(pl.engines, 0);
    for (uint32_t e = 0; e < pl.engines; e++) sh.reseed_m.emplace_back(new std::mutex);
    KangarooTable table(lo, W, P, c.sym);
    double elapsed_before = 0.0;
    if (resume) {
        if (!table.restore(wf.table.data(), wf.h.table, wf.h.false_matches, wf.h.reseeds)) die("-kangaroo -wl: the table section of " + wl_path + " does not load");
        std::vector<uint8_t>().swap(wf.table);
        table.set_cycles(wf.h.cycles);
        sh.rng = wf.h.rng; sh.steps = wf.h.steps; sh.dps = wf.h.dps; sh.dropped = wf.h.dropped;
        elapsed_before = wf.h.elapsed;
        for (uint32_t e = 0; e < pl.engines; e++) sh.reseed[e] = wf.reseed[e];
        printf("Resumed: %llu steps, %zu DPs\n", (unsigned long long)wf.h.steps, table.size());
    }
    const auto t0 = Clock::now();
    auto key_from_infinite_start = [&](i128 d) {                       // Q + u G = infinity: k' = -u
        std::lock_guard<std::mutex> lk(sh.rng_m);
        sh.key = hs::sc_add(base, sc_from_i128(-d));
        sh.found = true; sh.stop = true;
    };

    // a kangaroo's start: offsets from the shared stream (under its lock), in the order of idx
    auto draw = [&](const std::vector<uint32_t> &idx, std::vector<i128> &d, std::vector<uint32_t> &fl) {
        d.resize(idx.size()); fl.resize(idx.size());
        std::lock_guard<std::mutex> lk(sh.rng_m);
        for (size_t k = 0; k < idx.size(); k++) {
            fl[k] = idx[k] >= kn / 2 ? BSGS_KANGAROO_WILD : 0u;
            d[k] = c.sym ? herd_offset_sym(sh.rng, W, fl[k] != 0u) : herd_offset(sh.rng, W, fl[k] != 0u);
        }
    };
    // -kcpuseed: the points on the calling thread; a wild start at infinity IS the key
    auto host_states = [&](const std::vector<i128> &d, const std::vector<uint32_t> &fl, std::vector<bsgs_kangaroo_state> &out) {
        std::vector<bool> wild(d.size());
        for (size_t k = 0; k < d.size(); k++) wild[k] = fl[k] != 0u;
        const std::vector<Affine> pts = herd_points(*comb, Q, d, wild);
        out.resize(d.size());
        for (size_t k = 0; k < d.size(); k++) {
            if (pts[k].inf) key_from_infinite_start(d[k]);
            out[k] = to_state(pts[k], d[k], wild[k]);
        }
    };
    // initial herds: the offsets in engine order from the seeded stream, whoever computes the points
    std::vector<std::vector<i128>> offsets(pl.engines);
    std::vector<std::vector<bsgs_kangaroo_state>> herds(pl.engines);  // -kcpuseed: the host's states; -wl: the file's
    if (!resume) {
        for (uint32_t e = 0; e < pl.engines; e++) {
            offsets[e].resize(kn);
            for (uint64_t i = 0; i < kn; i++) offsets[e][i] = c.sym ? herd_offset_sym(sh.rng, W, i >= kn / 2) : herd_offset(sh.rng, W, i >= kn / 2);
        }
        if (cpuseed) {
            for (uint32_t e = 0; e < pl.engines; e++) {
                herds[e].resize(kn);
                const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
                std::vector<std::thread> tt;
                for (unsigned q = 0; q < nt; q++) tt.emplace_back([&, q]() {
                    const uint64_t b0 = kn * q / nt, b1 = kn * (q + 1) / nt;
                    std::vector<i128> dd(offsets[e].begin() + (long)b0, offsets[e].begin() + (long)b1);
                    std::vector<uint32_t> ff(b1 - b0);
                    for (uint64_t i = b0; i < b1; i++) ff[i - b0] = i >= kn / 2 ? BSGS_KANGAROO_WILD : 0u;
                    std::vector<bsgs_kangaroo_state> st;
                    host_states(dd, ff, st);
                    std::copy(st.begin(), st.end(), herds[e].begin() + (long)b0);
                });
                for (auto &t : tt) t.join();
                std::vector<i128>().swap(offsets[e]);
            }
            printf("[startup] %-44s %.3fs\n", "herds (host)", since(t0));
        }
    } else {
        for (uint32_t e = 0; e < pl.engines; e++) {
            herds[e].resize(kn);
            memcpy(herds[e].data(), wf.herds[e].data(), kn * sizeof(bsgs_kangaroo_state));
            std::vector<uint8_t>().swap(wf.herds[e]);
        }
    }

    // engines: one thread each, all calls for a device from the thread that opened it
    auto engine = [&](uint32_t e) {
        bsgs_dev *dev = nullptr;
        auto bad = [&](const char *what) { std::lock_guard<std::mutex> lk(sh.err_m); if (sh.err.empty()) sh.err = std::string(what) + ": " + bsgs_last_error(); sh.stop = true; };
        auto leave = [&]() {
            if (dev) bsgs_dev_close(dev);
            std::lock_guard<std::mutex> lk(sh.save_m);
            sh.running--;
            sh.save_cv.notify_all();
        };
        if (bsgs_dev_open(gpus[e], &dev) != BSGS_OK) { bad("bsgs_dev_open"); leave(); return; }
        if ((c.sym ? bsgs_kangaroo_setup_sym(dev, jxy.data(), js.data(), wh.jumps, pl.dp, (uint32_t)kn, pl.G, pl.cap)
                   : bsgs_kangaroo_setup(dev, jxy.data(), js.data(), pl.dp, (uint32_t)kn, pl.G, pl.cap)) != BSGS_OK) { bad("bsgs_kangaroo_setup"); leave(); return; }
        if (!herds[e].empty()) {
            if (bsgs_kangaroo_upload(dev, 0, (uint32_t)kn, herds[e].data()) != BSGS_OK) { bad("bsgs_kangaroo_upload"); leave(); return; }
            std::vector<bsgs_kangaroo_state>().swap(herds[e]);
        } else {
            const auto ts = Clock::now();
            std::vector<uint32_t> fl(kn);
            for (uint64_t i = 0; i < kn; i++) fl[i] = i >= kn / 2 ? BSGS_KANGAROO_WILD : 0u;
            uint32_t ninf = 0, first = 0;
            if (bsgs_kangaroo_seed(dev, qxy, nullptr, 0, (uint32_t)kn, (const uint8_t *)offsets[e].data(), fl.data(), &ninf, &first) != BSGS_OK) { bad("bsgs_kangaroo_seed"); leave(); return; }
            if (ninf) key_from_infinite_start(offsets[e][first]);
            std::vector<i128>().swap(offsets[e]);
            std::lock_guard<std::mutex> lk(sh.err_m);
            printf("[startup] %-44s %.3fs\n", ("herds (GPU), engine " + std::to_string(e)).c_str(), since(ts));
        }
        std::vector<bsgs_kangaroo_record> recs(pl.cap);
        bool have_herd = true;
        while (!sh.stop.load()) {
            std::vector<uint32_t> rs;
            { std::lock_guard<std::mutex> lk(*sh.reseed_m[e]); rs.swap(sh.reseed[e]); }
            if (!rs.empty()) {
                std::sort(rs.begin(), rs.end());
                rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
                std::vector<i128> d;
                std::vector<uint32_t> fl;
                draw(rs, d, fl);
                if (cpuseed) {
                    std::vector<bsgs_kangaroo_state> st;
                    host_states(d, fl, st);
                    if (bsgs_kangaroo_upload_list(dev, rs.data(), (uint32_t)rs.size(), st.data()) != BSGS_OK) { bad("bsgs_kangaroo_upload_list"); have_herd = false; break; }
                } else {
                    uint32_t ninf = 0, first = 0;
                    if (bsgs_kangaroo_seed(dev, qxy, rs.data(), 0, (uint32_t)rs.size(), (const uint8_t *)d.data(), fl.data(), &ninf, &first) != BSGS_OK) { bad("bsgs_kangaroo_seed"); have_herd = false; break; }
                    if (ninf) key_from_infinite_start(d[first]);
                }
                if (sh.stop.load()) break;
            }
            uint32_t n = 0;
            uint64_t dropped = 0;
            if (bsgs_kangaroo_run(dev, pl.S, recs.data(), pl.cap, &n, &dropped, nullptr) != BSGS_OK) { bad("bsgs_kangaroo_run"); have_herd = false; break; }
            const uint64_t total = (sh.steps += kn * pl.S);
            sh.dropped += dropped;
            { std::lock_guard<std::mutex> lk(sh.q_m); sh.queue.emplace_back(e, std::vector<bsgs_kangaroo_record>(recs.begin(), recs.begin() + n)); }
            sh.q_cv.notify_one();
            if (c.ksteps && total >= c.ksteps) sh.stop = true;
            if (sh.save_req.load() && !sh.stop.load()) {               // between two launches: the herd as it stands, then wait for the file
                sh.saved[e].resize(kn);
                if (bsgs_kangaroo_download(dev, 0, (uint32_t)kn, sh.saved[e].data()) != BSGS_OK) { bad("bsgs_kangaroo_download"); have_herd = false; break; }
                std::unique_lock<std::mutex> lk(sh.save_m);
                sh.parked++;
                sh.save_cv.notify_all();
                while (sh.save_req.load() && !sh.stop.load()) sh.save_cv.wait_for(lk, std::chrono::milliseconds(100));
                sh.parked--;
            }
        }
        if (have_herd && !sh.found.load()) {                           // the run stops without the key: the herd goes into the last save
            sh.saved[e].resize(kn);
            if (bsgs_kangaroo_download(dev, 0, (uint32_t)kn, sh.saved[e].data()) != BSGS_OK) bad("bsgs_kangaroo_download");
        }
        leave();
    };
    // the collector: every engine's records into the one table
    std::atomic<bool> engines_done{false};
    std::thread collector([&]() {
        for (;;) {
            std::pair<uint32_t, std::vector<bsgs_kangaroo_record>> b;
            {
                std::unique_lock<std::mutex> lk(sh.q_m);
                sh.collector_busy = false;
                sh.q_cv.wait_for(lk, std::chrono::milliseconds(100), [&] { return !sh.queue.empty() || engines_done.load(); });
                if (sh.queue.empty()) { if (engines_done.load()) return; continue; }
                b = std::move(sh.queue.front());
                sh.queue.pop_front();
                sh.collector_busy = true;
            }
            if (sh.found.load()) continue;
            sh.engine_records[b.first] += b.second.size();
            for (const bsgs_kangaroo_record &r : b.second) {
                u128 d;
                memcpy(&d, r.d, 16);
                Scalar key;
                const KangarooTable::Verdict v = table.add(r.x, d, (uint32_t)(b.first * kn + r.kangaroo), r.flags, &key);
                if (!(r.flags & BSGS_KANGAROO_DEAD)) sh.dps++;
                if (v == KangarooTable::FOUND) { sh.key = key; sh.found = true; sh.stop = true; break; }
                if (v == KangarooTable::RESEED) { std::lock_guard<std::mutex> lk(*sh.reseed_m[b.first]); sh.reseed[b.first].push_back(r.kangaroo); }
            }
        }
    });
    // the work file from the state as it stands: callers make sure that no engine walks and the collector's queue is empty
    auto write_state = [&]() {
        WorkHeader h = wh;
        h.rng = sh.rng; h.steps = sh.steps.load(); h.dps = sh.dps.load(); h.dropped = sh.dropped.load();
        h.false_matches = table.false_matches(); h.reseeds = table.reseeds(); h.table = table.size(); h.cycles = table.cycles();
        h.elapsed = elapsed_before + since(t0);
        std::vector<uint8_t> entries;
        entries.reserve(32 * table.size());
        table.write_entries(entries);
        std::vector<const std::vector<bsgs_kangaroo_state> *> hp;
        std::vector<std::vector<uint32_t>> rs(pl.engines);
        for (uint32_t e = 0; e < pl.engines; e++) { hp.push_back(&sh.saved[e]); std::lock_guard<std::mutex> lk(*sh.reseed_m[e]); rs[e] = sh.reseed[e]; }
        if (!write_work(work_path, work_tmp, h, entries, hp, rs)) fprintf(stderr, "WARNING: cannot write %s\n", work_path.c_str());
    };
    signalled = 0;
    signal(SIGINT, on_signal);
    signal(SIGTERM, on_signal);
    std::vector<std::thread> th;
    sh.running = sh.stop.load() ? 0 : pl.engines;
    if (!sh.stop.load()) for (uint32_t e = 0; e < pl.engines; e++) th.emplace_back(engine, e);
    auto last_t = Clock::now(), last_save = Clock::now();
    uint64_t last_steps = sh.steps.load();
    bool gave_up = false, interrupted = false;
    while (!sh.stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        const auto now = Clock::now();
        if (signalled) { interrupted = true; sh.stop = true; sh.save_cv.notify_all(); break; }
        if (std::chrono::duration<double>(now - last_t).count() >= 2.0) {
            const uint64_t st = sh.steps.load();
            const double rate = (st - last_steps) / std::chrono::duration<double>(now - last_t).count();
            printf("\r[%u] %.3e steps/s  steps 2^%.2f of expected 2^%.2f  DPs %llu  %.0fs   ", pl.engines, rate, st ? std::log2((double)st) : 0.0, std::log2(pl.expected),
                   (unsigned long long)sh.dps.load(), elapsed_before + since(t0));
            fflush(stdout);
            last_steps = st; last_t = now;
        }
        if ((double)sh.steps.load() > 20.0 * pl.expected) { gave_up = true; sh.stop = true; }
        if (!sh.stop.load() && std::chrono::duration<double>(now - last_save).count() >= (double)c.wt) {
            // -wt: every engine parks between two launches with its herd downloaded and its last records queued; the collector empties the queue; then
            // table, counters, stream, herds and re-seed lists belong to one moment of the search
            const auto ts = Clock::now();
            sh.save_req = true;
            {
                std::unique_lock<std::mutex> lk(sh.save_m);
                while (sh.parked != sh.running && !sh.stop.load() && !signalled) sh.save_cv.wait_for(lk, std::chrono::milliseconds(100));
            }
            for (;;) {
                { std::lock_guard<std::mutex> lk(sh.q_m); if ((sh.queue.empty() && !sh.collector_busy) || sh.stop.load()) break; }
                std::this_thread::sleep_for(std::chrono::milliseconds(1));
            }
            bool all_parked;
            { std::lock_guard<std::mutex> lk(sh.save_m); all_parked = sh.parked == pl.engines; }
            if (all_parked && !sh.stop.load()) { write_state(); printf("\n[save] %s in %.2fs\n", work_path.c_str(), since(ts)); }
            { std::lock_guard<std::mutex> lk(sh.save_m); sh.save_req = false; }
            sh.save_cv.notify_all();
            last_save = Clock::now();
        }
    }
    sh.save_cv.notify_all();
    for (auto &t : th) t.join();
    engines_done = true;
    sh.q_cv.notify_all();
    collector.join();
    signal(SIGINT, SIG_DFL);
    signal(SIGTERM, SIG_DFL);
    if (!sh.err.empty()) die(sh.err);
    const double secs = elapsed_before + since(t0);
    const bool budget = !sh.found.load() && !gave_up && !interrupted && c.ksteps && sh.steps.load() >= c.ksteps;
    std::string text, win;
    if (sh.found.load()) {
        std::string console;
        win = key_lines(cl.listpos, sh.key, P, console);
        text = console;
        remove(work_path.c_str());                                     // a stale file never outlives its job
    } else {
        bool have = true;
        for (uint32_t e = 0; e < pl.engines; e++) have = have && sh.saved[e].size() == kn;
        if (have) write_state();                                       // engines joined, queue drained: the state is final
        char line[160];
        snprintf(line, sizeof line, "\nKangaroo: stopped after %llu steps (%s)\n", (unsigned long long)sh.steps.load(), budget ? "-ksteps" : "signal");
        text = gave_up ? "\nKangaroo: no key after 20 times the expected steps (is the key in the range?)\n" : (budget || interrupted) ? line : "\nReached end of space\n";
    }
    char tail[512];
    snprintf(tail, sizeof tail, "Job time %.2fs, %.3e kangaroo steps, %llu DPs (%zu in the table, %llu dropped), %llu false matches, %llu re-seeds\n", secs,
             (double)sh.steps.load(), (unsigned long long)sh.dps.load(), table.size(), (unsigned long long)sh.dropped.load(), (unsigned long long)table.false_matches(),
             (unsigned long long)table.reseeds());
    text += tail;
    if (c.sym) text += "Symmetric walk: " + std::to_string(table.cycles()) + " cycles retired\n";
    for (uint32_t e = 0; e < pl.engines; e++) text += "Engine " + std::to_string(e) + " (GPU #" + std::to_string(gpus[e]) + "): " + std::to_string(sh.engine_records[e]) + " records\n";
    fputs(text.c_str(), stdout);                                       // one lane: the JobList leaves the console to the job (it appends win.txt)
    jobs.finish(0, text, sh.found.load(), win);
    printf("Found %d of %zu\n", jobs.found(), jobs.size());
    fflush(stdout);
    return sh.found.load() ? 0 : (budget || interrupted) ? 3 : 1;
}
