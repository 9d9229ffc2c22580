// host_kangaroo_multi.cpp -- the table of distinguished points for a LIST of public keys in one range (include/bsgs_hip.h "Kangaroo, many keys" states the
// rule; tests/kangaroo_multi_model.py MultiTable restates it): an owner per entry, links between two unsolved keys, a solved key's entries acting as tame
// ones, -selftest kangaroo-multi / kangaroo-multi-roundtrip, which drive the table with a scripted record stream and no GPU, and ListMode, the plain
// walk's part of what bsgs_mi355x -kangaroo -infile puts behind the driver's seam (host_kangaroo_list.h): saved to kangaroo.work version 3 and continued with
// -wl.
#include "host_kangaroo_list.h"

namespace {
typedef unsigned __int128 u128;
typedef __int128 i128;
}  // namespace

MultiKeyTable::MultiKeyTable(const Scalar &a, u128 W, const std::vector<Affine> &pubs)
    : a_(a), W_(W), pubs_(pubs), known_(pubs.size(), false), key_(pubs.size()), off_(pubs.size(), 0), adj_(pubs.size())
{
    map_.reserve(1u << 16);
}

void MultiKeyTable::presolve(uint32_t k, const Scalar &key)
{
    const Scalar o = hs::sc_sub(key, a_);                              // (callers pass keys of the range: key - a is below W <= 2^125)
    known_[k] = true; key_[k] = key; off_[k] = (i128)(((u128)o.l[1] << 64) | o.l[0]);
    solved_++;
}

bool MultiKeyTable::verify(uint32_t k, i128 off, Scalar *key) const
{
    if (off < 0 || (u128)off >= W_) return false;
    const Scalar cand = hs::sc_add(a_, hs::sc_from_u128((u128)off));
    const Affine q = hs::point_mul(hs::G, cand);
    if (q.inf || !hs::fe_equal(q.x, pubs_[k].x) || !hs::fe_equal(q.y, pubs_[k].y)) return false;
    *key = cand;
    return true;
}

// key k is found: its links, in the order they were kept, each give a candidate for the other key; a verified one is followed before the next link of k
// (depth first, as the model's recursion; an explicit stack: a chain can be as long as the list)
void MultiKeyTable::found(uint32_t k, const Scalar &key, std::vector<Event> &ev)
{
    if (known_[k]) return;                                            // (a key is reported once)
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
        const uint32_t other = l.j == f.k ? l.k : l.j;
        if (known_[other]) continue;                                  // solved on another path meanwhile: nothing left to learn from this link
        const i128 off = l.j == f.k ? off_[f.k] - l.delta : off_[f.k] + l.delta;      // k_j = k_k + delta
        Scalar kv;
        if (verify(other, off, &kv)) { resolved_++; enter(other, kv); }               // (enter() grows the stack: f is not used after it)
        else false_++;
    }
}

void MultiKeyTable::add(const uint8_t x[32], u128 d, uint32_t kid, uint32_t flags, std::vector<Event> &ev)
{
    if (flags & BSGS_KANGAROO_DEAD) { reseeds_++; ev.push_back(Event{RESEED, kid, 0, Scalar()}); return; }
    uint64_t k64;
    memcpy(&k64, x, 8);
    const uint32_t owner = record_owner(flags);
    auto it = map_.find(k64);                                         // look the tag up ...
    if (it == map_.end()) { map_.emplace(k64, Entry{(i128)d, kid, owner}); ev.push_back(Event{NEW, 0, 0, Scalar()}); return; }
    judge(it->second, (i128)d, kid, owner, ev);                       // ... and judge this record against that entry
}

void MultiKeyTable::add_pair(i128 entry_d, uint32_t entry_kid, uint32_t entry_owner, u128 d, uint32_t kid, uint32_t flags, std::vector<Event> &ev)
{
    if (flags & BSGS_KANGAROO_DEAD) { reseeds_++; ev.push_back(Event{RESEED, kid, 0, Scalar()}); return; }      // (never: the device hands a DEAD record back alone)
    judge(Entry{entry_d, entry_kid, entry_owner}, (i128)d, kid, record_owner(flags), ev);
}

// a record (d, kid, owner), not DEAD, against the stored entry of its x
void MultiKeyTable::judge(const Entry &e, i128 d, uint32_t kid, uint32_t owner, std::vector<Event> &ev)
{
    if (e.kid == kid) { ev.push_back(Event{REPEAT, 0, 0, Scalar()}); return; }
    // an owner whose key is solved counts as tame: d' = d + (k_k - a)
    i128 d1 = e.d, d2 = d;
    uint32_t o1 = e.owner, o2 = owner;
    if (o1 && known_[o1 - 1]) { d1 += off_[o1 - 1]; o1 = 0; }
    if (o2 && known_[o2 - 1]) { d2 += off_[o2 - 1]; o2 = 0; }
    if (o1 == o2) { reseeds_++; ev.push_back(Event{RESEED, kid, 0, Scalar()}); return; }
    if (!o1 || !o2) {
        const uint32_t k = (o1 ? o1 : o2) - 1u;
        Scalar key;
        if (verify(k, o1 ? d2 - d1 : d1 - d2, &key)) { found(k, key, ev); return; }     // d_T - d_W
        false_++;
        ev.push_back(Event{FALSE_MATCH, 0, 0, Scalar()});
        return;
    }
    // wild of j (stored) and wild of k (the record), both unsolved: k_j = k_k + d_k - d_j
    const uint32_t j = o1 - 1u, k = o2 - 1u;
    adj_[j].push_back((uint32_t)links_.size());
    adj_[k].push_back((uint32_t)links_.size());
    links_.push_back(Link{j, k, d2 - d1, true});
    kept_++; live_links_++; reseeds_++;
    ev.push_back(Event{LINK, j, k, Scalar()});
    ev.push_back(Event{RESEED, kid, 0, Scalar()});
}

void MultiKeyTable::write_entries(std::vector<uint8_t> &out) const
{
    for (const auto &kv : map_) {
        uint8_t e[32];
        memcpy(e, &kv.first, 8); memcpy(e + 8, &kv.second.d, 16); memcpy(e + 24, &kv.second.kid, 4); memcpy(e + 28, &kv.second.owner, 4);
        out.insert(out.end(), e, e + 32);
    }
}
void MultiKeyTable::write_keys(kang::WorkKeys &out) const
{
    out.solved.assign(pubs_.size(), 0); out.key.assign(pubs_.size(), Scalar());
    for (size_t k = 0; k < pubs_.size(); k++) if (known_[k]) { out.solved[k] = 1; out.key[k] = key_[k]; }
    out.links.clear();
    for (const Link &l : links_) if (l.alive) out.links.push_back(kang::WorkLink{l.j, l.k, l.delta});
    out.kept = kept_; out.resolved = resolved_;
}
bool MultiKeyTable::restore(const uint8_t *entries, uint64_t n, uint64_t false_matches, uint64_t reseeds, const kang::WorkKeys &keys)
{
    if (keys.solved.size() != pubs_.size()) return false;
    for (size_t k = 0; k < pubs_.size(); k++) {
        if (!keys.solved[k] || known_[k]) continue;
        const Scalar o = hs::sc_sub(keys.key[k], a_);                  // a solved key of the file lies in the range and is the key of its point
        Scalar kv;
        if (o.l[2] || o.l[3] || !verify((uint32_t)k, (i128)(((u128)o.l[1] << 64) | o.l[0]), &kv)) return false;
        presolve((uint32_t)k, kv);
    }
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *e = entries + 32 * i;
        uint64_t k64; Entry en;
        memcpy(&k64, e, 8); memcpy(&en.d, e + 8, 16); memcpy(&en.kid, e + 24, 4); memcpy(&en.owner, e + 28, 4);
        if (en.owner > pubs_.size() || !map_.emplace(k64, en).second) return false;
    }
    for (const kang::WorkLink &l : keys.links) {
        if (l.j >= pubs_.size() || l.k >= pubs_.size() || l.j == l.k) return false;
        adj_[l.j].push_back((uint32_t)links_.size());
        adj_[l.k].push_back((uint32_t)links_.size());
        links_.push_back(Link{l.j, l.k, l.delta, true});
        live_links_++;
    }
    false_ = false_matches; reseeds_ = reseeds; kept_ = keys.kept; resolved_ = keys.resolved;
    return true;
}

// one scripted record into the table, its event lines printed; false: the record does not parse.  dpt (-selftest kangaroo-dpkeys): the record goes through
// DevDpTable::take as the device would hand it back -- paired: as the duplicate behind the stored half taken before it, never a dead record -- and is judged
// as take() names it
static bool multi_scripted_record(MultiKeyTable &tab, size_t n_keys, const std::string &rec, kang::DevDpTable *dpt = nullptr, bool paired = false)
{
    const std::vector<std::string> f = kang::split_commas(rec);
    if (f.size() != 4 || f[0].empty() || !strchr(paired ? "TW" : "TWD", f[0][0]) || (f[0][0] != 'W' && f[0].size() != 1)) return false;
    bsgs_kangaroo_record r;
    memset(&r, 0, sizeof r);
    r.flags = f[0][0] == 'D' ? BSGS_KANGAROO_DEAD : 0u;
    unsigned long k = 0;
    if (f[0][0] == 'W') {
        if (f[0].size() < 2) return false;
        k = strtoul(f[0].c_str() + 1, nullptr, 10);
        if (k >= n_keys) return false;
        r.flags = BSGS_KANGAROO_WILD | (uint32_t)k << BSGS_KANGAROO_KEY_SHIFT;
    }
    Scalar x, dd;
    if (!hs::fe_from_hex(x, f[1]) || !hs::fe_from_hex(dd, f[2]) || dd.l[2] || dd.l[3]) return false;
    hs::fe_to_le(x, r.x);
    memcpy(r.d, &dd.l[0], 16);
    r.kangaroo = (uint32_t)strtoul(f[3].c_str(), nullptr, 10);
    kang::DevDpTable off;
    const kang::DevDpTable::Taken t = (dpt ? dpt : &off)->take_scripted(r, (uint32_t)k, paired);
    const u128 d = ((u128)dd.l[1] << 64) | dd.l[0];
    std::vector<MultiKeyTable::Event> ev;
    if (t.kind == kang::DevDpTable::PAIR) {
        if (!tab.owner_fits(t.stored->flags)) { fprintf(stderr, "the table is damaged: an entry names owner %u, the list has %zu keys\n", t.stored->flags, n_keys); return false; }
        i128 ed;
        memcpy(&ed, t.stored->d, 16);
        tab.add_pair(ed, t.stored->kangaroo, t.stored->flags, d, r.kangaroo, r.flags, ev);
    } else if (t.kind == kang::DevDpTable::ALONE || t.kind == kang::DevDpTable::NOT_MINE) tab.add(r.x, d, r.kangaroo, r.flags, ev);
    else return false;
    for (const MultiKeyTable::Event &e : ev) switch (e.what) {
        case MultiKeyTable::NEW: printf("new\n"); break;
        case MultiKeyTable::REPEAT: printf("repeat\n"); break;
        case MultiKeyTable::RESEED: printf("reseed %u\n", e.a); break;
        case MultiKeyTable::FALSE_MATCH: printf("false\n"); break;
        case MultiKeyTable::LINK: printf("link %u %u\n", e.a, e.b); break;
        case MultiKeyTable::FOUND: printf("found %u %s\n", e.a, hs::fe_to_hex(e.key).c_str()); break;
    }
    return true;
}
// the keys equal to pk*G are solved up front: "presolved <k>"
static void presolve_scripted(MultiKeyTable &tab, const std::vector<Affine> &pubs, const Scalar &lo)
{
    const Affine aG = hs::point_mul(hs::G, lo);
    for (size_t k = 0; k < pubs.size(); k++)
        if (hs::fe_equal(pubs[k].x, aG.x) && hs::fe_equal(pubs[k].y, aG.y)) { tab.presolve((uint32_t)k, lo); printf("presolved %zu\n", k); }
}
static void print_summary(const MultiKeyTable &tab)
{
    printf("summary %zu %llu %llu %llu %llu %u\n", tab.size(), (unsigned long long)tab.false_matches(), (unsigned long long)tab.reseeds(),
           (unsigned long long)tab.links_kept(), (unsigned long long)tab.links_resolved(), tab.solved());
}

// -selftest kangaroo-multi <pk hex> <pke hex> <pubkey>[,<pubkey>...] <record>...   record = T|W<k>|D,<x hex>,<d hex: 128-bit two's complement>,<kangaroo>
// (W<k>: a wild kangaroo of the key at list position k, from 0; D: a dead record).  A key equal to pk*G is solved up front: "presolved <k>".  One line per
// event of a record: "new", "repeat", "reseed <kangaroo>", "false", "link <j> <k>", "found <k> <key hex>"; then
// "summary <stored> <false matches> <reseeds> <links kept> <links resolved> <keys solved>".
// -selftest kangaroo-dpkeys [sym] <pk hex> <pke hex> <pubkey>[,<pubkey>...] <item>...: the hand-back rule of -kdpkeys without a GPU, every item through
// DevDpTable::take.  An item is a scripted record as -selftest kangaroo-multi (sym: kangaroo-symlist) takes it -- what the device hands back alone: DEAD, tag
// 0, a full table -- and goes through the host's own map; or S,<tag hex>,<d hex>,<kangaroo>,<owner> followed by its record: a duplicate, judged against the
// stored entry it came with.  The same event and summary lines.
static int multi_selftest(const std::vector<std::string> &a, bool dpkeys)
{
    if (a.size() < 3) return 2;
    Scalar lo, hi; u128 W;
    std::vector<Affine> pubs;
    if (!kang::parse_range_pubs(a[0], a[1], a[2], lo, hi, W, pubs) || pubs.empty() || pubs.size() > BSGS_KANGAROO_MAX_KEYS) return 2;
    MultiKeyTable tab(lo, W, pubs);
    presolve_scripted(tab, pubs, lo);
    kang::DevDpTable dpt;
    dpt.on = dpt.keyed = dpkeys;
    if (!dpt.scripted_items(a, [&](const std::string &rec, bool paired) { return multi_scripted_record(tab, pubs.size(), rec, &dpt, paired); })) return 2;
    print_summary(tab);
    return 0;
}
int kangaroo_multi_selftest(const std::vector<std::string> &a) { return multi_selftest(a, false); }
int kangaroo_dpkeys_selftest(const std::vector<std::string> &a)
{
    return !a.empty() && a[0] == "sym" ? kangaroo_dpkeys_sym_selftest(std::vector<std::string>(a.begin() + 1, a.end())) : multi_selftest(a, true);
}

// -selftest kangaroo-dpkeys-plan <pk hex> <pke hex> <CUs> <min launch> <dp or -1> <kn or 0> <kdpn or 0> <L>: the plan of -kdpkeys for one engine and L open
// keys without a GPU -- -kdpdev's with sqrt(L W) in the place of sqrt(W) for the capacity and dp, through DevDpTable::plan --, one line:
// "plan <dp> <kn> <per thread> <S> <record buffer> <capacity>"
int kangaroo_dpkeys_plan_selftest(const std::vector<std::string> &a)
{
    if (a.size() != 8) return 2;
    kang::KangConfig c;
    c.pk = a[0]; c.pke = a[1]; c.dp = atoi(a[4].c_str()); c.kdpn = strtoull(a[6].c_str(), nullptr, 0);
    kang::Prologue p(c);
    const uint64_t L = strtoull(a[7].c_str(), nullptr, 0);
    if (!L || L > BSGS_KANGAROO_MAX_KEYS) return 2;
    kang::DevDpTable dpt;
    kang::Plan pl = kang::plan_herd(p.sqrtW, 1, atoi(a[2].c_str()), dpt.plan(c, std::sqrt((double)L * (double)p.W), 0), strtoull(a[5].c_str(), nullptr, 0));
    kang::plan_launch(pl, p.sqrtW, 0.0, atof(a[3].c_str()), true, c.dp < 0);
    printf("plan %u %llu %u %u %u %llu\n", pl.dp, (unsigned long long)pl.kn, pl.G, pl.S, pl.cap, (unsigned long long)dpt.capacity);
    return 0;
}

// -selftest kangaroo-multi-roundtrip <pk hex> <pke hex> <pubkeys> <split> <record>...: the first <split> records into a table, the table into a version-3
// work file without herds (a temporary file; BSGS_SELFTEST_WORK names a path to write and keep instead), the file into a fresh table, the other records into
// that one.  Prints what -selftest kangaroo-multi prints for the undivided stream.
int kangaroo_multi_roundtrip_selftest(const std::vector<std::string> &a)
{
    if (a.size() < 4) return 2;
    Scalar lo, hi; u128 W;
    std::vector<Affine> pubs;
    if (!kang::parse_range_pubs(a[0], a[1], a[2], lo, hi, W, pubs) || pubs.empty() || pubs.size() > BSGS_KANGAROO_MAX_KEYS) return 2;
    const size_t split = (size_t)strtoull(a[3].c_str(), nullptr, 10);
    if (split > a.size() - 4) return 2;
    bool keep;
    const std::string path = kang::selftest_work_path(keep);
    if (path.empty()) return 2;
    kang::WorkHeader h;
    h.version = kang::WORK_VERSION_KEYS;
    {
        MultiKeyTable first(lo, W, pubs);
        presolve_scripted(first, pubs, lo);
        for (size_t i = 0; i < split; i++) if (!multi_scripted_record(first, pubs.size(), a[4 + i])) return 2;
        std::vector<uint8_t> entries;
        kang::WorkKeys wk;
        first.write_entries(entries);
        first.write_keys(wk);
        h.table = first.size(); h.false_matches = first.false_matches(); h.reseeds = first.reseeds();
        for (size_t i = 0; i < split; i++) if (a[4 + i][0] != 'D') h.dps++;
        h.fingerprint = kang::keys_fingerprint(pubs, lo, hi, h);
        if (!kang::write_work(path, path + ".temp", h, entries, {}, {}, &wk)) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
    }
    kang::WorkFile wf;
    const std::string bad = kang::read_work(path, wf, true, kang::WORK_VERSION_KEYS);
    if (!keep) remove(path.c_str());
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    if (kang::keys_fingerprint(pubs, lo, hi, wf.h) != wf.h.fingerprint) { fprintf(stderr, "Recovery file was made with other settings\n"); return 1; }
    MultiKeyTable second(lo, W, pubs);
    if (!second.restore(wf.table.data(), wf.h.table, wf.h.false_matches, wf.h.reseeds, wf.keys)) { fprintf(stderr, "the table section does not load\n"); return 1; }
    for (size_t i = 4 + split; i < a.size(); i++) if (!multi_scripted_record(second, pubs.size(), a[i])) return 2;
    print_summary(second);
    return 0;
}

// ---- bsgs_mi355x -kangaroo -infile FILE with the plain walk: what ListSearch (host_kangaroo_list.h) leaves to the walk ---------------------------------
namespace {
using namespace kang;
struct ListMode : ListSearch<MultiKeyTable> {
    ListMode(const KangConfig &c, const std::vector<Affine> &P) : ListSearch(c, P)
    {
        version = WORK_VERSION_KEYS;
        wl_flag = "-kangaroo -infile -wl"; wl_kind = "a kangaroo.work file of a key list";
    }
    Scalar origin(const Prologue &p) const override { return p.lo; }              // Q_k = P_k - a*G; a wild start at infinity: k_key = a - u
    MultiKeyTable *new_table(const Prologue &p) const override { return new MultiKeyTable(p.lo, p.W, P); }
    bool restore_table(Prologue &p) override { return table->restore(p.wf.table.data(), p.wf.h.table, p.wf.h.false_matches, p.wf.h.reseeds, p.wf.keys); }
    i128 offset(uint64_t &rng, bool wild) const override { return herd_offset(rng, pro->W, wild); }
    // a wild kangaroo's flags carry its key
    uint32_t state_key(const bsgs_kangaroo_state &s) const override { return (s.flags >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu; }
    void put_key(bsgs_kangaroo_state &s, uint32_t key) const override { s.flags |= key << BSGS_KANGAROO_KEY_SHIFT; }
    void print_expectation(const Prologue &p) const override
    {
        printf("Expected steps for %u keys: between 2^%.2f (2 sqrt(L W)) and 2^%.2f (L 2 sqrt(W)), DP overhead included\n", open0, std::log2(exp_lo), std::log2(exp_hi));
        (void)p;
    }
    const char *setup(bsgs_dev *dev) override
    {
        const Plan &pl = pro->pl;
        if (bsgs_kangaroo_setup(dev, pro->jxy.data(), pro->js.data(), pl.dp, (uint32_t)pl.kn, pl.G, pl.cap) != BSGS_OK) return "bsgs_kangaroo_setup";
        if (bsgs_kangaroo_set_keys(dev, qxy.data(), L) != BSGS_OK) return "bsgs_kangaroo_set_keys";
        return dpt.begin(dev);
    }
    void add_record(const bsgs_kangaroo_record &r, uint32_t kid, std::vector<MultiKeyTable::Event> &ev) override
    {
        u128 d;
        memcpy(&d, r.d, 16);
        table->add(r.x, d, kid, r.flags, ev);
    }
    void add_pair_record(const bsgs_kangaroo_record &st, const bsgs_kangaroo_record &r, uint32_t kid, std::vector<MultiKeyTable::Event> &ev) override
    {
        u128 d; i128 ed;
        memcpy(&d, r.d, 16); memcpy(&ed, st.d, 16);
        table->add_pair(ed, st.kangaroo, st.flags, d, kid, r.flags, ev);
    }
    // (verify_q stays null: the engines hold the key list)  owner 0 tame, 1 + k a wild kangaroo of key k
    uint32_t entry_flags(uint32_t owner) const override { return owner ? BSGS_KANGAROO_WILD | (owner - 1u) << BSGS_KANGAROO_KEY_SHIFT : 0u; }
};
}  // namespace

int kangaroo_multi_main(const KangConfig &c) { return list_main<ListMode>(c); }
