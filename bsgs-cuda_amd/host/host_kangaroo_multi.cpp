// host_kangaroo_multi.cpp -- the table of distinguished points for a LIST of public keys in one range (include/bsgs_hip.h "Kangaroo, many keys" states the
// rule; tests/kangaroo_multi_model.py MultiTable restates it): an owner per entry, links between two unsolved keys, a solved key's entries acting as tame
// ones, -selftest kangaroo-multi / kangaroo-multi-roundtrip, which drive the table with a scripted record stream and no GPU, and ListMode, what
// bsgs_mi355x -kangaroo -infile puts behind the driver's seam (host_kangaroo_run.h): saved to kangaroo.work version 3 and continued with -wl.
#include "host_kangaroo_multi.h"
#include "host_kangaroo_run.h"

#include <map>

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
    const uint32_t owner = flags & BSGS_KANGAROO_WILD ? 1u + ((flags >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu) : 0u;
    auto it = map_.find(k64);
    if (it == map_.end()) { map_.emplace(k64, Entry{(i128)d, kid, owner}); ev.push_back(Event{NEW, 0, 0, Scalar()}); return; }
    const Entry &e = it->second;
    if (e.kid == kid) { ev.push_back(Event{REPEAT, 0, 0, Scalar()}); return; }
    // an owner whose key is solved counts as tame: d' = d + (k_k - a)
    i128 d1 = e.d, d2 = (i128)d;
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

// one scripted record into the table, its event lines printed; false: the record does not parse
static bool multi_scripted_record(MultiKeyTable &tab, size_t n_keys, const std::string &rec)
{
    const std::vector<std::string> f = kang::split_commas(rec);
    if (f.size() != 4 || f[0].empty() || !strchr("TWD", f[0][0]) || (f[0][0] != 'W' && f[0].size() != 1)) return false;
    uint32_t flags = f[0][0] == 'D' ? BSGS_KANGAROO_DEAD : 0u;
    if (f[0][0] == 'W') {
        if (f[0].size() < 2) return false;
        const unsigned long k = strtoul(f[0].c_str() + 1, nullptr, 10);
        if (k >= n_keys) return false;
        flags = BSGS_KANGAROO_WILD | (uint32_t)k << BSGS_KANGAROO_KEY_SHIFT;
    }
    Scalar x, dd;
    if (!hs::fe_from_hex(x, f[1]) || !hs::fe_from_hex(dd, f[2]) || dd.l[2] || dd.l[3]) return false;
    uint8_t xb[32];
    hs::fe_to_le(x, xb);
    std::vector<MultiKeyTable::Event> ev;
    tab.add(xb, ((u128)dd.l[1] << 64) | dd.l[0], (uint32_t)strtoul(f[3].c_str(), nullptr, 10), flags, ev);
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
int kangaroo_multi_selftest(const std::vector<std::string> &a)
{
    if (a.size() < 3) return 2;
    Scalar lo, hi; u128 W;
    std::vector<Affine> pubs;
    if (!kang::parse_range_pubs(a[0], a[1], a[2], lo, hi, W, pubs) || pubs.empty() || pubs.size() > BSGS_KANGAROO_MAX_KEYS) return 2;
    MultiKeyTable tab(lo, W, pubs);
    presolve_scripted(tab, pubs, lo);
    for (size_t i = 3; i < a.size(); i++) if (!multi_scripted_record(tab, pubs.size(), a[i])) return 2;
    print_summary(tab);
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

// ---- bsgs_mi355x -kangaroo -infile FILE: every key of the list in [pk, pke] with ONE herd per engine -----------------------------------------------
namespace {
using namespace kang;

// which key a wild kangaroo works on (include/bsgs_hip.h "Kangaroo, many keys", assignment; tests/kangaroo_multi_model.py Assigner)
class Assigner {
public:
    Assigner(uint32_t L, const std::vector<bool> &presolved, uint64_t n_wild) : count_(L, 0), key_(n_wild)
    {
        for (uint32_t k = 0; k < L; k++) if (!presolved[k]) open_.push_back(k);
        for (uint64_t w = 0; w < n_wild; w++) { key_[w] = open_[w % open_.size()]; count_[key_[w]]++; }
        for (uint32_t k : open_) by_count_.insert({count_[k], k});
    }
    uint32_t key(uint64_t w) const { return key_[w]; }
    void solved(uint32_t k) { by_count_.erase({count_[k], k}); }                   // k takes no kangaroo from now on
    // the key of wild kangaroo w from now on: its own while that is open, else the open key with the fewest kangaroos, lowest position first; false: none open
    bool reseed(uint64_t w, const MultiKeyTable &t, uint32_t *k)
    {
        const uint32_t old = key_[w];
        if (!t.known(old)) { *k = old; return true; }
        if (by_count_.empty()) return false;
        const uint32_t best = by_count_.begin()->second;
        by_count_.erase(by_count_.begin());
        count_[old]--; count_[best]++;
        by_count_.insert({count_[best], best});
        key_[w] = best; *k = best;
        return true;
    }
    const std::vector<uint32_t> &keys() const { return key_; }
    // -wl: every wild kangaroo's key as its saved state names it
    void restore(const std::vector<uint32_t> &keys, const MultiKeyTable &t)
    {
        key_ = keys;
        std::fill(count_.begin(), count_.end(), 0u);
        for (uint32_t k : key_) count_[k]++;
        by_count_.clear();
        for (uint32_t k : open_) if (!t.known(k)) by_count_.insert({count_[k], k});
    }
private:
    std::vector<uint32_t> open_, count_, key_;
    std::set<std::pair<uint32_t, uint32_t>> by_count_;                             // (kangaroos, list position) of the keys still open
};
}  // namespace

namespace {
struct ListMode : Mode {
    ListMode(const KangConfig &c, const std::vector<Affine> &P) : c(c), P(P), L((uint32_t)P.size())
    {
        version = WORK_VERSION_KEYS;
        wl_flag = "-kangaroo -infile -wl"; wl_kind = "a kangaroo.work file of a key list";
        if (c.cpuseed) herd_label = "herds (host), engine ";
    }
    std::string fingerprint(const Prologue &p, const WorkHeader &h) const override { return keys_fingerprint(P, p.lo, p.hi, h); }
    // a key is known: its KEY[n] block on the console and in win.txt at once, through key_lines as the BSGS path writes it
    void report(uint32_t k)
    {
        std::string console;
        const std::string win = key_lines((int)k + 1, table->key(k), P[k], console);
        fputs(console.c_str(), stdout);
        fflush(stdout);
        std::ofstream f(c.dir + "/win.txt", std::ios::app | std::ios::binary);
        f << win;
        found_n++;
    }
    bool before_devices(Prologue &p) override
    {
        pro = &p;
        if (p.resume && p.wf.keys.solved.size() != L) die("Recovery file was made with other settings");
        if (!p.resume) { Config rc; rc.dir = c.dir; read_recovery(rc); }         // (win.txt starts empty, as on the BSGS path; a resumed run appends to the one it has)
        p.t0 = Clock::now();
        table.reset(new MultiKeyTable(p.lo, p.W, P));
        for (uint32_t k = 0; k < L; k++) same[hs::compress_pubkey(P[k])].push_back(k);
        // keys solved before any device is opened: P_k == a*G has no affine Q_k; it keeps its slot (G stands in, no kangaroo is assigned)
        const Affine aG = hs::point_mul(hs::G, p.lo), naG = hs::affine_neg(aG);
        presolved.assign(L, false);
        qxy.resize(64 * (size_t)L);
        Q.resize(L);
        for (uint32_t k = 0; k < L; k++) {
            Q[k] = hs::point_add(P[k], naG);
            if (Q[k].inf) { presolved[k] = true; table->presolve(k, p.lo); if (p.resume) found_n++; else report(k); Q[k] = hs::G; }
            hs::affine_to_le(Q[k], &qxy[64 * (size_t)k], &qxy[64 * (size_t)k + 32]);
        }
        if (p.resume) {                                                            // the file's solved keys are in win.txt already: counted, not written again
            const uint32_t before = table->solved();
            if (!table->restore(p.wf.table.data(), p.wf.h.table, p.wf.h.false_matches, p.wf.h.reseeds, p.wf.keys)) die("-kangaroo -wl: the table section of " + p.wl_path + " does not load");
            std::vector<uint8_t>().swap(p.wf.table);
            found_n += (int)(table->solved() - before);
        }
        open0 = L - table->solved();
        if (!open0) printf("Found %d of %u\n", found_n, L);
        return open0 != 0;
    }
    // after the prologue: the expectation, the assignment of wild kangaroos to keys (-wl: as the saved states name it), the offsets of the initial herds in
    // engine order from the seeded stream (the points are computed in each engine's thread, by the GPU or with -kcpuseed by the host's comb)
    void prepare(Prologue &p, Shared &s)
    {
        sh = &s;
        const Plan &pl = p.pl;
        const uint64_t kn = pl.kn;
        half = kn / 2;                                                             // kangaroos [0, half) of an engine are tame, [half, kn) wild
        overhead = (double)kn * pl.engines * std::ldexp(1.0, (int)pl.dp);
        exp_lo = 2.0 * std::sqrt((double)open0 * (double)p.W) + overhead; exp_hi = (double)open0 * 2.0 * p.sqrtW + overhead;
        // (the give-up bound: 20 times L_open 2 sqrt(W) + overhead steps without a new key, L_open the keys open at that moment)
        printf("Expected steps for %u keys: between 2^%.2f (2 sqrt(L W)) and 2^%.2f (L 2 sqrt(W)), DP overhead included\n", open0, std::log2(exp_lo), std::log2(exp_hi));
        asg.reset(new Assigner(L, presolved, (kn - half) * pl.engines));
        if (p.resume) {
            std::vector<uint32_t> keys((kn - half) * pl.engines);
            for (uint32_t e = 0; e < pl.engines; e++) for (uint64_t i = half; i < kn; i++) {
                const uint32_t k = (p.herds[e][i].flags >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu;
                if (k >= L) die("-kangaroo -wl: a kangaroo of " + p.wl_path + " names key " + std::to_string(k));
                keys[(uint64_t)e * (kn - half) + (i - half)] = k;
            }
            asg->restore(keys, *table);
            printf("Resumed: %llu steps, %zu DPs, %u of %u keys solved\n", (unsigned long long)p.wf.h.steps, table->size(), table->solved(), L);
        }
        if (c.cpuseed) comb.reset(new Comb());
        steps_mark = s.steps.load();
        last_solved = table->solved();
        off0.resize(pl.engines);
        if (!p.resume) for (uint32_t e = 0; e < pl.engines; e++) { off0[e].resize(kn); for (uint64_t i = 0; i < kn; i++) off0[e][i] = herd_offset(s.rng, p.W, i >= half); }
    }
    // under sh->tab_m.  The consequences of FOUND events: the block is written, equal points of the list are solved with it, the key's kangaroos start afresh
    void on_events(const std::vector<MultiKeyTable::Event> &ev)
    {
        const uint64_t wild = pro->pl.kn - half;
        for (const MultiKeyTable::Event &x : ev) {
            if (x.what != MultiKeyTable::FOUND) continue;
            report(x.a);
            asg->solved(x.a);
            for (uint64_t w = 0; w < asg->keys().size(); w++) if (asg->keys()[w] == x.a) sh->push_reseed((uint32_t)(w / wild), (uint32_t)(half + w % wild));
            for (uint32_t o : same[hs::compress_pubkey(P[x.a])]) if (!table->known(o)) {
                std::vector<MultiKeyTable::Event> more;
                table->found(o, x.key, more);
                on_events(more);
            }
        }
        if (table->solved() == L) sh->stop = true;
    }
    const char *setup(bsgs_dev *dev) override
    {
        const Plan &pl = pro->pl;
        if (bsgs_kangaroo_setup(dev, pro->jxy.data(), pro->js.data(), pl.dp, (uint32_t)pl.kn, pl.G, pl.cap) != BSGS_OK) return "bsgs_kangaroo_setup";
        return bsgs_kangaroo_set_keys(dev, qxy.data(), L) == BSGS_OK ? nullptr : "bsgs_kangaroo_set_keys";
    }
    // one seed call: the whole herd (idx empty) or a list; a start at infinity solves its key and the kangaroo is seeded again next round
    const char *seed(bsgs_dev *dev, uint32_t e, const std::vector<uint32_t> &idx, Shared &s) override
    {
        const uint64_t kn = pro->pl.kn, wild0 = (uint64_t)e * (kn - half);
        std::vector<uint32_t> use, fl, key;
        std::vector<i128> d;
        if (idx.empty()) {
            fl.resize(kn); key.assign(kn, 0);
            for (uint64_t i = 0; i < kn; i++) { fl[i] = i >= half ? BSGS_KANGAROO_WILD : 0u; if (i >= half) key[i] = asg->key(wild0 + (i - half)); }
            d.swap(off0[e]);
        } else {                                                                   // offsets and keys: under the table's lock and then the stream's
            std::lock_guard<std::mutex> lt(s.tab_m);
            std::lock_guard<std::mutex> lk(s.rng_m);
            for (uint32_t i : idx) {
                const bool wild = i >= half;
                uint32_t k = 0;
                if (wild && !asg->reseed(wild0 + (i - half), *table, &k)) continue;                      // no key is open: the kangaroo rests
                use.push_back(i); fl.push_back(wild ? BSGS_KANGAROO_WILD : 0u); key.push_back(k);
                d.push_back(herd_offset(s.rng, pro->W, wild));
            }
            if (use.empty()) return nullptr;
        }
        uint32_t ninf = 0, first = 0;
        if (c.cpuseed) {                                                           // the same herd from the host's comb
            std::vector<uint32_t> word(d.size());
            std::vector<const Affine *> q(d.size());
            for (size_t k = 0; k < d.size(); k++) { word[k] = fl[k] | key[k] << BSGS_KANGAROO_KEY_SHIFT; q[k] = fl[k] ? &Q[key[k]] : nullptr; }
            std::vector<bsgs_kangaroo_state> st;
            const std::vector<size_t> inf = comb_states(*comb, d, word, q, st);
            for (size_t k : inf) st[k].flags |= BSGS_KANGAROO_DEAD;
            if ((use.empty() ? bsgs_kangaroo_upload(dev, 0, (uint32_t)st.size(), st.data()) : bsgs_kangaroo_upload_list(dev, use.data(), (uint32_t)use.size(), st.data())) != BSGS_OK) return "bsgs_kangaroo_upload";
            if (!inf.empty()) { ninf = 1; first = (uint32_t)inf[0]; }
        } else if (bsgs_kangaroo_seed_keys(dev, use.empty() ? nullptr : use.data(), 0, (uint32_t)d.size(), (const uint8_t *)d.data(), fl.data(), key.data(), &ninf, &first) != BSGS_OK) return "bsgs_kangaroo_seed_keys";
        if (ninf) {
            if (fl[first]) {                                                       // Q_key + u G = infinity: k_key = a - u
                std::lock_guard<std::mutex> lt(s.tab_m);
                if (!table->known(key[first])) {
                    std::vector<MultiKeyTable::Event> ev;
                    table->found(key[first], hs::sc_add(pro->lo, sc_from_i128(-d[first])), ev);
                    on_events(ev);
                }
            }
            s.push_reseed(e, use.empty() ? first : use[first]);
        }
        return nullptr;
    }
    bool record(uint32_t e, const bsgs_kangaroo_record &r, Shared &s) override
    {
        u128 d;
        memcpy(&d, r.d, 16);
        std::vector<MultiKeyTable::Event> ev;
        table->add(r.x, d, (uint32_t)(e * pro->pl.kn + r.kangaroo), r.flags, ev);
        for (const MultiKeyTable::Event &x : ev) if (x.what == MultiKeyTable::RESEED) s.push_reseed(e, r.kangaroo);
        on_events(ev);
        return true;
    }
    // (verify_q stays null: the engines hold the key list)  owner 0 tame, 1 + k a wild kangaroo of key k
    uint32_t entry_flags(uint32_t owner) const override { return owner ? BSGS_KANGAROO_WILD | (owner - 1u) << BSGS_KANGAROO_KEY_SHIFT : 0u; }
    bool done() const override { return table->solved() == L; }
    // give up: 20 times one key's expectation for every key still open, counted from the last key found
    bool give_up(uint64_t steps) override
    {
        const uint32_t solved_now = table->solved();
        if (solved_now != last_solved) { last_solved = solved_now; steps_mark = steps; }
        return (double)(steps - steps_mark) > 20.0 * ((double)(L - solved_now) * 2.0 * pro->sqrtW + overhead);
    }
    void status(double rate, uint64_t st, uint64_t dps) const override
    {
        printf("\r[%u] %.3e steps/s  steps 2^%.2f of expected 2^%.2f..2^%.2f  solved %u/%u  DPs %llu  %.0fs   ", pro->pl.engines, rate, st ? std::log2((double)st) : 0.0,
               std::log2(exp_lo), std::log2(exp_hi), table->solved(), L, (unsigned long long)dps, since(pro->t0));
    }
    const WorkKeys *save(WorkHeader &h, std::vector<uint8_t> &entries) override
    {
        h.false_matches = table->false_matches(); h.reseeds = table->reseeds(); h.table = table->size();
        entries.reserve(32 * table->size());
        table->write_entries(entries);
        table->write_keys(wk);
        return &wk;
    }

    const KangConfig &c;
    const std::vector<Affine> &P;
    const uint32_t L;
    const Prologue *pro = nullptr;
    Shared *sh = nullptr;
    std::unique_ptr<MultiKeyTable> table;
    std::unique_ptr<Assigner> asg;
    std::map<std::string, std::vector<uint32_t>> same;                            // list positions that hold the same point
    std::vector<bool> presolved;
    std::vector<Affine> Q;
    std::vector<uint8_t> qxy;
    std::unique_ptr<Comb> comb;
    std::vector<std::vector<i128>> off0;
    WorkKeys wk;
    int found_n = 0;
    uint32_t open0 = 0, last_solved = 0;
    uint64_t half = 0, steps_mark = 0;
    double overhead = 0.0, exp_lo = 0.0, exp_hi = 0.0;
};
}  // namespace

int kangaroo_multi_main(const KangConfig &c)
{
    Config fc; fc.infile = c.infile;
    const std::vector<std::string> pub_hex = read_pubs(fc);                       // the BSGS path's reader: same formats, same messages; a missing file ends the run here
    if (pub_hex.empty()) die("No public keys in " + c.infile);
    if (pub_hex.size() > BSGS_KANGAROO_MAX_KEYS) die("-kangaroo -infile: at most 65535 public keys, the file has " + std::to_string(pub_hex.size()));
    const uint32_t L = (uint32_t)pub_hex.size();
    std::vector<Affine> P(L);
    for (uint32_t k = 0; k < L; k++) if (!hs::parse_pubkey(P[k], pub_hex[k]) || !hs::on_curve(P[k])) die("Invalid Public Key (-infile, line " + std::to_string(k + 1) + ") length!!!");
    Prologue p(c);
    printf("Kangaroo range [%s, %s], width 2^%.2f, %u public keys\n", hs::fe_to_hex(p.lo).c_str(), hs::fe_to_hex(p.hi).c_str(), std::log2((double)p.W), L);
    ListMode mode(c, P);
    p.complete(c, mode);                                                           // dp, kn, the jump mean and the launch length from W, as for one key
    if (!p.go) return 0;
    Shared sh(p);
    mode.prepare(p, sh);
    const Outcome o = run(c, p, sh, mode);

    const MultiKeyTable &table = *mode.table;
    if (o == GAVE_UP) printf("\nKangaroo: %u of %u keys open after 20 times the expected steps (are the keys in the range?)\n", L - table.solved(), L);
    else if (o != DONE) printf("\nKangaroo: stopped after %llu steps (%s), %u of %u keys open\n", (unsigned long long)sh.steps.load(), o == BUDGET ? "-ksteps" : "signal",
                               L - table.solved(), L);
    printf("Job time %.2fs, %.3e kangaroo steps, %llu DPs (%zu in the table, %llu dropped), %llu false matches, %llu re-seeds, %llu links kept, %llu links resolved\n", p.elapsed_before + since(p.t0),
           (double)sh.steps.load(), (unsigned long long)sh.dps.load(), table.size(), (unsigned long long)sh.dropped.load(), (unsigned long long)table.false_matches(),
           (unsigned long long)table.reseeds(), (unsigned long long)table.links_kept(), (unsigned long long)table.links_resolved());
    for (uint32_t e = 0; e < p.pl.engines; e++) printf("Engine %u (GPU #%d): %llu records\n", e, p.gpus[e], (unsigned long long)sh.engine_records[e]);
    printf("Found %d of %u\n", mode.found_n, L);
    fflush(stdout);
    return o == DONE ? 0 : (o == BUDGET || o == INTERRUPTED) ? 3 : 1;
}
