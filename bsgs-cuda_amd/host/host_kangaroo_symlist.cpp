// host_kangaroo_symlist.cpp -- bsgs_mi355x -kangaroo -infile FILE -kwalk sym: a LIST of public keys in one range searched by one herd of the symmetric walk
// (include/bsgs_hip.h "Kangaroo, many keys, symmetric walk" states the rule; tests/kangaroo_symlist_model.py SymListTable restates it).  Here: the table -- an
// entry holds an owner and NEG, a link both ends' signs and offsets, a solved key's entries act as tame ones --, -selftest kangaroo-symlist /
// kangaroo-symlist-roundtrip, which drive it with a scripted record stream and no GPU, and SymListMode, the symmetric walk's part of what a list search puts behind the driver's
// seam (host_kangaroo_list.h): a herd of bsgs_kangaroo_setup_sym_keys per engine, whose records name their key in their fourth word, saved to kangaroo.work
// version 4 and continued with -wl.  Everything the two list searches share -- the key file, the assignment of wild kangaroos, seeding, the
// KEY[n] blocks and win.txt, the give-up bound, the command -- is ListSearch and list_main of host_kangaroo_list.h.
#include "host_kangaroo_list.h"

using namespace kang;

namespace {
const uint32_t OWNER_NEG = 0x80000000u;            // an entry's owner word: 0 tame, 1 + k a wild kangaroo of key k, bit 31: it stands at -Q_k + d*G
const double SYMLIST_JUMPSCALE = 2.0;              // as -ksym ("jump scale")

class SymListTable {
public:
    enum What { NEW, REPEAT, RESEED, FALSE_MATCH, LINK, FOUND };
    struct Event { What what; uint32_t a, b; Scalar key; };
    SymListTable(const Scalar &a, u128 W, const std::vector<Affine> &pubs)
        : W_(W), mid_(hs::sc_add(a, hs::sc_from_u128(W / 2))), pubs_(pubs), known_(pubs.size(), false), key_(pubs.size()), kpp_(pubs.size(), 0), adj_(pubs.size())
    {
        map_.reserve(1u << 16);
    }
    const Scalar &mid() const { return mid_; }
    // a key known before the search (P_k == (a + W/2)*G, or one a work file reports as solved); callers pass keys of the range
    void presolve(uint32_t k, const Scalar &key)
    {
        const bool below = hs::fe_cmp(key, mid_) < 0;
        const Scalar o = below ? hs::sc_sub(mid_, key) : hs::sc_sub(key, mid_);
        const i128 m = (i128)(((u128)o.l[1] << 64) | o.l[0]);
        known_[k] = true; key_[k] = key; kpp_[k] = below ? -m : m;
        solved_++;
    }
    // key k is found (a collision; or learnt outside the table, from a wild start at infinity: the same consequences).  Its links, in the order they were kept, each give two candidates for the other key; a verified one is followed before the next link of k (depth first, as
    // the model's recursion; an explicit stack: a chain can be as long as the list)
    void found(uint32_t k, const Scalar &key, std::vector<Event> &ev)
    {
        if (known_[k]) return;
        struct Frame { uint32_t k; size_t pos; };
        std::vector<Frame> stack;
        auto enter = [&](uint32_t kk, const Scalar &kv) {
            presolve(kk, kv);
            ev.push_back(Event{FOUND, kk, 0, kv});
            stack.push_back(Frame{kk, 0});
        };
        enter(k, key);
        while (!stack.empty()) {
            Frame &f = stack.back();
            if (f.pos == adj_[f.k].size()) { std::vector<uint32_t>().swap(adj_[f.k]); stack.pop_back(); continue; }
            Link &l = links_[adj_[f.k][f.pos++]];
            if (!l.alive) continue;
            l.alive = false;
            live_links_--;
            const bool from_j = l.j == f.k;
            const uint32_t other = from_j ? l.k : l.j;
            if (known_[other]) continue;                              // solved on another path meanwhile: nothing left to learn from this link
            // sigma1 k''_j + d1 = eps (sigma2 k''_k + d2): the known end's side, then the other end from it for both eps
            const i128 side = from_j ? l.s1 * kpp_[f.k] + l.d1 : l.s2 * kpp_[f.k] + l.d2;
            const i128 so = from_j ? l.s2 : l.s1, dof = from_j ? l.d2 : l.d1;
            Scalar kv;
            if (verify(other, so * (side - dof), &kv) || verify(other, so * (-side - dof), &kv)) { resolved_++; enter(other, kv); }      // (enter() grows the stack: f is not used after it)
            else false_++;
        }
    }
    // one record into the table; key: the record's fourth word, the key of its kangaroo (below the list's length for a wild record)
    void add(const uint8_t x[32], u128 d, uint32_t kid, uint32_t flags, uint32_t key, std::vector<Event> &ev)
    {
        if (dead(kid, flags, ev)) return;
        uint64_t k64;
        memcpy(&k64, x, 8);
        const uint32_t owner = record_owner(flags, key);
        auto it = map_.find(k64);                                     // look the tag up ...
        if (it == map_.end()) { map_.emplace(k64, Entry{(i128)d, kid, owner}); ev.push_back(Event{NEW, 0, 0, Scalar()}); return; }
        judge(it->second, (i128)d, kid, owner, ev);                   // ... and judge this record against that entry
    }
    // -kdpkeys: a record the device table handed back as a duplicate, against the stored entry it came with (d, kangaroo, owner word): exactly the events
    // add() gives for a record that meets that entry in the map; never NEW, and the map is not touched
    void add_pair(i128 entry_d, uint32_t entry_kid, uint32_t entry_owner, u128 d, uint32_t kid, uint32_t flags, uint32_t key, std::vector<Event> &ev)
    {
        if (dead(kid, flags, ev)) return;                             // (never: the device hands a DEAD record back alone)
        judge(Entry{entry_d, entry_kid, entry_owner}, (i128)d, kid, record_owner(flags, key), ev);
    }
    bool owner_fits(uint32_t owner) const { return (owner & ~OWNER_NEG) <= pubs_.size() && owner != OWNER_NEG; }      // an owner word of this list
    bool known(uint32_t k) const { return known_[k]; }
    const Scalar &key(uint32_t k) const { return key_[k]; }
    uint32_t solved() const { return solved_; }
    size_t size() const { return map_.size(); }
    uint64_t false_matches() const { return false_; }
    uint64_t reseeds() const { return reseeds_; }
    uint64_t cycles() const { return cycles_; }
    uint64_t links_kept() const { return kept_; }
    uint64_t links_resolved() const { return resolved_; }
    // the work file's view (version 4): one 32-byte entry per stored point -- low 64 bits of x, d, kangaroo, owner word -- and the key list's state
    void write_entries(std::vector<uint8_t> &out) const
    {
        for (const auto &kv : map_) {
            uint8_t e[32];
            memcpy(e, &kv.first, 8); memcpy(e + 8, &kv.second.d, 16); memcpy(e + 24, &kv.second.kid, 4); memcpy(e + 28, &kv.second.owner, 4);
            out.insert(out.end(), e, e + 32);
        }
    }
    void write_keys(WorkKeys &out) const
    {
        out.solved.assign(pubs_.size(), 0); out.key.assign(pubs_.size(), Scalar());
        for (size_t k = 0; k < pubs_.size(); k++) if (known_[k]) { out.solved[k] = 1; out.key[k] = key_[k]; }
        out.links.clear();
        for (const Link &l : links_) if (l.alive) out.links.push_back(WorkLink{l.j, l.k, 0, l.s1, l.s2, l.d1, l.d2});
        out.kept = kept_; out.resolved = resolved_;
    }
    // a fresh table from a work file: false when a solved key, an entry or a link does not fit the list
    bool restore(const uint8_t *entries, uint64_t n, const WorkHeader &h, const WorkKeys &keys)
    {
        if (keys.solved.size() != pubs_.size()) return false;
        for (size_t k = 0; k < pubs_.size(); k++) {
            if (!keys.solved[k] || known_[k]) continue;
            const Affine q = hs::point_mul(hs::G, keys.key[k]);       // a solved key of the file is the key of its point, and presolve() wants it near the range
            const Scalar o = hs::fe_cmp(keys.key[k], mid_) < 0 ? hs::sc_sub(mid_, keys.key[k]) : hs::sc_sub(keys.key[k], mid_);
            if (o.l[2] || o.l[3] || (o.l[1] >> 62) || q.inf || !hs::fe_equal(q.x, pubs_[k].x) || !hs::fe_equal(q.y, pubs_[k].y)) return false;
            presolve((uint32_t)k, keys.key[k]);
        }
        for (uint64_t i = 0; i < n; i++) {
            const uint8_t *e = entries + 32 * i;
            uint64_t k64; Entry en;
            memcpy(&k64, e, 8); memcpy(&en.d, e + 8, 16); memcpy(&en.kid, e + 24, 4); memcpy(&en.owner, e + 28, 4);
            if ((en.owner & ~OWNER_NEG) > pubs_.size() || en.owner == OWNER_NEG || !map_.emplace(k64, en).second) return false;
        }
        for (const WorkLink &l : keys.links) {
            if (l.j >= pubs_.size() || l.k >= pubs_.size() || l.j == l.k || (l.s1 != 1 && l.s1 != -1) || (l.s2 != 1 && l.s2 != -1)) return false;
            adj_[l.j].push_back((uint32_t)links_.size());
            adj_[l.k].push_back((uint32_t)links_.size());
            links_.push_back(Link{l.j, l.k, l.s1, l.s2, l.d1, l.d2, true});
            live_links_++;
        }
        false_ = h.false_matches; reseeds_ = h.reseeds; cycles_ = h.cycles; kept_ = keys.kept; resolved_ = keys.resolved;
        return true;
    }
private:
    struct Entry { i128 d; uint32_t kid, owner; };
    static uint32_t record_owner(uint32_t flags, uint32_t key) { return flags & BSGS_KANGAROO_WILD ? (1u + key) | (flags & BSGS_KANGAROO_NEG ? OWNER_NEG : 0u) : 0u; }
    bool dead(uint32_t kid, uint32_t flags, std::vector<Event> &ev)
    {
        if (!(flags & BSGS_KANGAROO_DEAD)) return false;
        reseeds_++;
        if (flags & BSGS_KANGAROO_CYCLE) cycles_++;
        ev.push_back(Event{RESEED, kid, 0, Scalar()});
        return true;
    }
    // a record (d, kid, owner), not DEAD, against the stored entry of its x
    void judge(const Entry &e, i128 d, uint32_t kid, uint32_t owner, std::vector<Event> &ev)
    {
        // its own point again with the offset and the owner it had: the walk is a function of x, so it runs a cycle longer than the window.  (A kangaroo's
        // number outlives a re-seed: on a point of its earlier life, with another offset, key or sign, it is taken as any other kangaroo below.)
        if (e.kid == kid && e.owner == owner && e.d == d) {
            reseeds_++; cycles_++;
            ev.push_back(Event{REPEAT, 0, 0, Scalar()});
            ev.push_back(Event{RESEED, kid, 0, Scalar()});
            return;
        }
        // sigma and key of both; an owner whose key is solved counts as tame: d' = d + sigma k''
        i128 d1 = e.d, d2 = d;
        int s1 = sigma(e.owner), s2 = sigma(owner);
        const uint32_t k1 = (e.owner & ~OWNER_NEG) - 1u, k2 = (owner & ~OWNER_NEG) - 1u;      // (meaningless for sigma 0)
        if (s1 && known_[k1]) { d1 += s1 * kpp_[k1]; s1 = 0; }
        if (s2 && known_[k2]) { d2 += s2 * kpp_[k2]; s2 = 0; }
        auto reseed = [&]() { reseeds_++; ev.push_back(Event{RESEED, kid, 0, Scalar()}); };
        if (!s1 && !s2) { reseed(); return; }
        Scalar kv;
        if (!s1 || !s2) {                                             // tame d_T, wild (sigma, d_W) of key k: k'' = sigma (eps d_T - d_W)
            const i128 dt = s1 ? d2 : d1, dw = s1 ? d1 : d2;
            const int sw = s1 ? s1 : s2;
            const uint32_t k = s1 ? k1 : k2;
            if (verify(k, sw * (dt - dw), &kv) || verify(k, sw * (-dt - dw), &kv)) { found(k, kv, ev); return; }
            false_++;
            ev.push_back(Event{FALSE_MATCH, 0, 0, Scalar()});
            reseed();
            return;
        }
        if (k1 == k2) {                                               // the rule of one key: (sigma1 - eps sigma2) k'' = eps d2 - d1, the divisor +-2 or 0
            bool tried = false;
            for (int eps = 1; eps >= -1; eps -= 2) {
                const int den = s1 - eps * s2;
                if (!den) continue;
                tried = true;
                const i128 num = eps * d2 - d1;
                if (num & 1) continue;                                // (no integer solves it: mod n it lies far outside the interval)
                if (verify(k1, num / den, &kv)) { found(k1, kv, ev); return; }
            }
            if (tried) { false_++; ev.push_back(Event{FALSE_MATCH, 0, 0, Scalar()}); }
            reseed();
            return;
        }
        adj_[k1].push_back((uint32_t)links_.size());
        adj_[k2].push_back((uint32_t)links_.size());
        links_.push_back(Link{k1, k2, s1, s2, d1, d2, true});
        kept_++; live_links_++;
        ev.push_back(Event{LINK, k1, k2, Scalar()});
        reseed();
    }
    struct Link { uint32_t j, k; int s1, s2; i128 d1, d2; bool alive; };     // sigma1 k''_j + d1 = +-(sigma2 k''_k + d2)
    static int sigma(uint32_t owner) { return !owner ? 0 : owner & OWNER_NEG ? -1 : 1; }
    // k'' in [-floor(W/2), ceil(W/2)) and (a + floor(W/2) + k'')*G == P_k
    bool verify(uint32_t k, i128 kpp, Scalar *key) const
    {
        if (kpp < -(i128)(W_ / 2) || kpp >= (i128)(W_ - W_ / 2)) return false;
        const Scalar cand = hs::sc_add(mid_, sc_from_i128(kpp));
        const Affine q = hs::point_mul(hs::G, cand);
        if (q.inf || !hs::fe_equal(q.x, pubs_[k].x) || !hs::fe_equal(q.y, pubs_[k].y)) return false;
        *key = cand;
        return true;
    }
    const u128 W_;
    const Scalar mid_;
    const std::vector<Affine> pubs_;
    std::vector<bool> known_;
    std::vector<Scalar> key_;
    std::vector<i128> kpp_;                                       // k''_k = k_k - (a + W/2) of a solved key
    std::unordered_map<uint64_t, Entry> map_;
    std::vector<Link> links_;
    std::vector<std::vector<uint32_t>> adj_;                      // per key: its links, in the order they were kept
    uint64_t false_ = 0, reseeds_ = 0, cycles_ = 0, kept_ = 0, resolved_ = 0, live_links_ = 0;
    uint32_t solved_ = 0;
};

// one scripted record into the table, its event lines printed; false: the record does not parse.  dpt (-selftest kangaroo-dpkeys sym): the record goes through
// DevDpTable::take as the device would hand it back -- paired: as the duplicate behind the stored half taken before it, never a dead record -- and is judged
// as take() names it
bool scripted_record(SymListTable &tab, size_t n_keys, const std::string &rec, DevDpTable *dpt = nullptr, bool paired = false)
{
    const std::vector<std::string> f = split_commas(rec);
    if (f.size() != 4 || f[0].empty() || !strchr(paired ? "TWN" : "TWNDC", f[0][0])) return false;
    const char t = f[0][0];
    bsgs_kangaroo_record r;
    memset(&r, 0, sizeof r);
    r.flags = t == 'D' ? BSGS_KANGAROO_DEAD : t == 'C' ? BSGS_KANGAROO_DEAD | BSGS_KANGAROO_CYCLE : 0u;
    if (t == 'W' || t == 'N') {
        if (f[0].size() < 2) return false;
        const unsigned long k = strtoul(f[0].c_str() + 1, nullptr, 10);
        if (k >= n_keys) return false;
        r.reserved = (uint32_t)k;                                     // the key beside the flags
        r.flags = BSGS_KANGAROO_WILD | (t == 'N' ? BSGS_KANGAROO_NEG : 0u);
    } else if (f[0].size() != 1) return false;
    Scalar x, dd;
    if (!hs::fe_from_hex(x, f[1]) || !hs::fe_from_hex(dd, f[2]) || dd.l[2] || dd.l[3]) return false;
    hs::fe_to_le(x, r.x);
    memcpy(r.d, &dd.l[0], 16);
    r.kangaroo = (uint32_t)strtoul(f[3].c_str(), nullptr, 10);
    DevDpTable off;
    const DevDpTable::Taken tk = (dpt ? dpt : &off)->take_scripted(r, r.reserved, paired);
    const u128 d = ((u128)dd.l[1] << 64) | dd.l[0];
    std::vector<SymListTable::Event> ev;
    if (tk.kind == DevDpTable::PAIR) {
        if (!tab.owner_fits(tk.stored->flags)) { fprintf(stderr, "the table is damaged: an entry names owner %u, the list has %zu keys\n", tk.stored->flags, n_keys); return false; }
        i128 ed;
        memcpy(&ed, tk.stored->d, 16);
        tab.add_pair(ed, tk.stored->kangaroo, tk.stored->flags, d, r.kangaroo, r.flags, tk.walk.reserved, ev);
    } else if (tk.kind == DevDpTable::ALONE || tk.kind == DevDpTable::NOT_MINE) tab.add(r.x, d, r.kangaroo, r.flags, tk.walk.reserved, ev);
    else return false;
    for (const SymListTable::Event &e : ev) switch (e.what) {
        case SymListTable::NEW: printf("new\n"); break;
        case SymListTable::REPEAT: printf("repeat\n"); break;
        case SymListTable::RESEED: printf("reseed %u\n", e.a); break;
        case SymListTable::FALSE_MATCH: printf("false\n"); break;
        case SymListTable::LINK: printf("link %u %u\n", e.a, e.b); break;
        case SymListTable::FOUND: printf("found %u %s\n", e.a, hs::fe_to_hex(e.key).c_str()); break;
    }
    return true;
}
// the keys equal to (pk + W/2)*G are solved up front: "presolved <k>"
void presolve_scripted(SymListTable &tab, const std::vector<Affine> &pubs)
{
    const Affine mG = hs::point_mul(hs::G, tab.mid());
    for (size_t k = 0; k < pubs.size(); k++)
        if (hs::fe_equal(pubs[k].x, mG.x) && hs::fe_equal(pubs[k].y, mG.y)) { tab.presolve((uint32_t)k, tab.mid()); printf("presolved %zu\n", k); }
}
void print_summary(const SymListTable &tab)
{
    printf("summary %zu %llu %llu %llu %llu %u %llu\n", tab.size(), (unsigned long long)tab.false_matches(), (unsigned long long)tab.reseeds(),
           (unsigned long long)tab.links_kept(), (unsigned long long)tab.links_resolved(), tab.solved(), (unsigned long long)tab.cycles());
}
}  // namespace

// -selftest kangaroo-symlist <pk hex> <pke hex> <pubkey>[,<pubkey>...] <record>...   record = T|W<k>|N<k>|D|C,<x hex>,<d hex: 128-bit two's complement>,<kangaroo>
// (W<k>: a wild kangaroo of the key at list position k, from 0; N<k>: one with NEG; D: a dead record; C: a cycle's dead record).  A key equal to
// (pk + W/2)*G is solved up front: "presolved <k>".  One line per event of a record, as -selftest kangaroo-multi; then
// "summary <stored> <false matches> <reseeds> <links kept> <links resolved> <keys solved> <cycles>".
// -selftest kangaroo-dpkeys sym ...: the symmetric walk's part of -selftest kangaroo-dpkeys (host_kangaroo_multi.cpp describes the items); an owner word is
// decimal, bit 31 for NEG
static int symlist_selftest(const std::vector<std::string> &a, bool dpkeys)
{
    if (a.size() < 3) return 2;
    Scalar lo, hi; u128 W;
    std::vector<Affine> pubs;
    if (!parse_range_pubs(a[0], a[1], a[2], lo, hi, W, pubs) || pubs.empty() || pubs.size() > BSGS_KANGAROO_MAX_KEYS) return 2;
    SymListTable tab(lo, W, pubs);
    presolve_scripted(tab, pubs);
    DevDpTable dpt;
    dpt.on = dpt.keyed = dpkeys;
    if (!dpt.scripted_items(a, [&](const std::string &rec, bool paired) { return scripted_record(tab, pubs.size(), rec, &dpt, paired); })) return 2;
    print_summary(tab);
    return 0;
}
int kangaroo_symlist_selftest(const std::vector<std::string> &a) { return symlist_selftest(a, false); }
int kangaroo_dpkeys_sym_selftest(const std::vector<std::string> &a) { return symlist_selftest(a, true); }

// -selftest kangaroo-symlist-roundtrip <pk hex> <pke hex> <pubkeys> <split> <record>...: the first <split> records into a table, the table into a version-4
// work file without herds (a temporary file; BSGS_SELFTEST_WORK names a path to write and keep instead; 1024 jump points, jump scale 1), the file into a fresh
// table, the other records into that one.  Prints what -selftest kangaroo-symlist prints for the undivided stream.
int kangaroo_symlist_roundtrip_selftest(const std::vector<std::string> &a)
{
    if (a.size() < 4) return 2;
    Scalar lo, hi; u128 W;
    std::vector<Affine> pubs;
    if (!parse_range_pubs(a[0], a[1], a[2], lo, hi, W, pubs) || pubs.empty() || pubs.size() > BSGS_KANGAROO_MAX_KEYS) return 2;
    const size_t split = (size_t)strtoull(a[3].c_str(), nullptr, 10);
    if (split > a.size() - 4) return 2;
    bool keep;
    const std::string path = selftest_work_path(keep);
    if (path.empty()) return 2;
    WorkHeader h;
    h.version = WORK_VERSION_SYMKEYS; h.jumps = 1024; h.jumpscale = 1.0;
    {
        SymListTable first(lo, W, pubs);
        presolve_scripted(first, pubs);
        for (size_t i = 0; i < split; i++) if (!scripted_record(first, pubs.size(), a[4 + i])) return 2;
        std::vector<uint8_t> entries;
        WorkKeys wk;
        first.write_entries(entries);
        first.write_keys(wk);
        h.table = first.size(); h.false_matches = first.false_matches(); h.reseeds = first.reseeds(); h.cycles = first.cycles();
        for (size_t i = 0; i < split; i++) if (a[4 + i][0] != 'D' && a[4 + i][0] != 'C') h.dps++;
        h.fingerprint = keys_fingerprint(pubs, lo, hi, h);
        if (!write_work(path, path + ".temp", h, entries, {}, {}, &wk)) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
    }
    WorkFile wf;
    const std::string bad = read_work(path, wf, true, WORK_VERSION_SYMKEYS);
    if (!keep) remove(path.c_str());
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    if (keys_fingerprint(pubs, lo, hi, wf.h) != wf.h.fingerprint) { fprintf(stderr, "Recovery file was made with other settings\n"); return 1; }
    SymListTable second(lo, W, pubs);
    if (!second.restore(wf.table.data(), wf.h.table, wf.h, wf.keys)) { fprintf(stderr, "the table section does not load\n"); return 1; }
    for (size_t i = 4 + split; i < a.size(); i++) if (!scripted_record(second, pubs.size(), a[i])) return 2;
    print_summary(second);
    return 0;
}

// ---- bsgs_mi355x -kangaroo -infile FILE -kwalk sym: what ListSearch (host_kangaroo_list.h) leaves to the walk ----------------------------------------
namespace {
struct SymListMode : ListSearch<SymListTable> {
    SymListMode(const KangConfig &c, const std::vector<Affine> &P) : ListSearch(c, P)
    {
        version = WORK_VERSION_SYMKEYS;
        min_launch = 2.0 * BSGS_KANGAROO_CYCLE_WINDOW;                             // a launch longer than the cycle window
        wl_flag = "-kangaroo -infile -kwalk sym -wl"; wl_kind = "a kangaroo.work file of a key list searched with -kwalk sym";
    }
    void own_settings(Prologue &p) override
    {
        const WorkHeader &f = p.wf.h;
        if (p.resume && ((c.jumps && c.jumps != f.jumps) || (c.jumpscale != 0.0 && c.jumpscale != f.jumpscale))) die("Recovery file was made with other settings");
        jumps = p.wh.jumps = p.resume ? f.jumps : c.jumps ? c.jumps : 1024u;
        jumpscale = p.wh.jumpscale = p.resume ? f.jumpscale : c.jumpscale != 0.0 ? c.jumpscale : SYMLIST_JUMPSCALE;
    }
    // offsets are counted from the middle of the range: Q_k = P_k - (a + W/2)*G; a wild start at infinity: k''_key = -d
    Scalar origin(const Prologue &p) const override { return hs::sc_add(p.lo, hs::sc_from_u128(p.W / 2)); }
    SymListTable *new_table(const Prologue &p) const override { return new SymListTable(p.lo, p.W, P); }
    bool restore_table(Prologue &p) override { return table->restore(p.wf.table.data(), p.wf.h.table, p.wf.h, p.wf.keys); }
    i128 offset(uint64_t &rng, bool wild) const override { return herd_offset_sym(rng, pro->W, wild); }
    // the key beside the flags, which hold the last jump index
    uint32_t state_key(const bsgs_kangaroo_state &s) const override { return s.reserved[0]; }
    void put_key(bsgs_kangaroo_state &s, uint32_t key) const override { s.reserved[0] = key; }
    void print_expectation(const Prologue &p) const override
    {
        printf("Kangaroo: symmetric walk (negation map), %u jump points, jump scale %g\n", p.wh.jumps, p.wh.jumpscale);
        printf("Expected steps for %u keys: below the plain walk's 2^%.2f (2 sqrt(L W)) to 2^%.2f (L 2 sqrt(W)), DP overhead included\n", open0, std::log2(exp_lo), std::log2(exp_hi));
    }
    const char *setup(bsgs_dev *dev) override
    {
        const Plan &pl = pro->pl;
        if (bsgs_kangaroo_setup_sym_keys(dev, pro->jxy.data(), pro->js.data(), jumps, pl.dp, (uint32_t)pl.kn, pl.G, pl.cap) != BSGS_OK) return "bsgs_kangaroo_setup_sym_keys";
        if (bsgs_kangaroo_set_keys(dev, qxy.data(), L) != BSGS_OK) return "bsgs_kangaroo_set_keys";
        return dpt.begin(dev);
    }
    void add_record(const bsgs_kangaroo_record &r, uint32_t kid, std::vector<SymListTable::Event> &ev) override
    {
        if ((r.flags & BSGS_KANGAROO_WILD) && !(r.flags & BSGS_KANGAROO_DEAD) && r.reserved >= L) return;       // (the device names keys of the list only)
        u128 d;
        memcpy(&d, r.d, 16);
        table->add(r.x, d, kid, r.flags, r.reserved, ev);
    }
    void add_pair_record(const bsgs_kangaroo_record &st, const bsgs_kangaroo_record &r, uint32_t kid, std::vector<SymListTable::Event> &ev) override
    {
        if ((r.flags & BSGS_KANGAROO_WILD) && r.reserved >= L) return;                                           // (as above)
        u128 d; i128 ed;
        memcpy(&d, r.d, 16); memcpy(&ed, st.d, 16);
        table->add_pair(ed, st.kangaroo, st.flags, d, kid, r.flags, r.reserved, ev);
    }
    // (verify_q stays null: the engines hold the key list)  the owner word as the verification's flags: WILD | NEG | k << 8
    uint32_t entry_flags(uint32_t owner) const override
    {
        const uint32_t o = owner & ~OWNER_NEG;
        return o ? BSGS_KANGAROO_WILD | (owner & OWNER_NEG ? BSGS_KANGAROO_NEG : 0u) | (o - 1u) << BSGS_KANGAROO_KEY_SHIFT : 0u;
    }
    void save_own(WorkHeader &h) const override { h.cycles = table->cycles(); }
    void closing() const override { printf("Symmetric walk: %llu cycles retired\n", (unsigned long long)table->cycles()); }
};
}  // namespace

int kangaroo_symlist_main(const KangConfig &c) { return list_main<SymListMode>(c); }
