// host_kangaroo_multi.cpp -- the table of distinguished points for a LIST of public keys in one range (include/bsgs_hip.h "Kangaroo, many keys" states the
// rule; tests/kangaroo_multi_model.py MultiTable restates it): an owner per entry, links between two unsolved keys, a solved key's entries acting as tame
// ones, -selftest kangaroo-multi / kangaroo-multi-roundtrip, which drive the table with a scripted record stream and no GPU, and the run itself:
// bsgs_mi355x -kangaroo -infile, saved to kangaroo.work version 3 and continued with -wl.
#include "host_kangaroo_multi.h"
#include "host_kangaroo.h"

#include <csignal>
#include <map>
#include <random>

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
    std::vector<std::string> f;
    std::stringstream ss(rec);
    std::string tok;
    while (std::getline(ss, tok, ',')) f.push_back(tok);
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

// -selftest kangaroo-multi <pk hex> <pke hex> <pubkey>[,<pubkey>...] <record>...   record = T|W<k>|D,<x hex>,<d hex: 128-bit two's complement>,<kangaroo>
// (W<k>: a wild kangaroo of the key at list position k, from 0; D: a dead record).  A key equal to pk*G is solved up front: "presolved <k>".  One line per
// event of a record: "new", "repeat", "reseed <kangaroo>", "false", "link <j> <k>", "found <k> <key hex>"; then
// "summary <stored> <false matches> <reseeds> <links kept> <links resolved> <keys solved>".
int kangaroo_multi_selftest(const std::vector<std::string> &a)
{
    if (a.size() < 3) return 2;
    Scalar lo, hi;
    if (!hs::fe_from_hex(lo, a[0]) || !hs::fe_from_hex(hi, a[1])) return 2;
    const Scalar w = hs::sc_sub(hi, lo);
    if (w.l[2] || w.l[3]) return 2;
    const u128 W = (((u128)w.l[1] << 64) | w.l[0]) + 1;
    std::vector<Affine> pubs;
    {
        std::stringstream ss(a[2]);
        std::string tok;
        while (std::getline(ss, tok, ',')) {
            Affine P;
            if (!hs::parse_pubkey(P, cut_hex(tok)) || !hs::on_curve(P)) return 2;
            pubs.push_back(P);
        }
    }
    if (pubs.empty() || pubs.size() > BSGS_KANGAROO_MAX_KEYS) return 2;
    MultiKeyTable tab(lo, W, pubs);
    const Affine aG = hs::point_mul(hs::G, lo);
    for (size_t k = 0; k < pubs.size(); k++)
        if (hs::fe_equal(pubs[k].x, aG.x) && hs::fe_equal(pubs[k].y, aG.y)) { tab.presolve((uint32_t)k, lo); printf("presolved %zu\n", k); }
    for (size_t i = 3; i < a.size(); i++) if (!multi_scripted_record(tab, pubs.size(), a[i])) return 2;
    printf("summary %zu %llu %llu %llu %llu %u\n", tab.size(), (unsigned long long)tab.false_matches(), (unsigned long long)tab.reseeds(),
           (unsigned long long)tab.links_kept(), (unsigned long long)tab.links_resolved(), tab.solved());
    return 0;
}

// -selftest kangaroo-multi-roundtrip <pk hex> <pke hex> <pubkeys> <split> <record>...: the first <split> records into a table, the table into a version-3
// work file without herds (a temporary file; BSGS_SELFTEST_WORK names a path to write and keep instead), the file into a fresh table, the other records into
// that one.  Prints what -selftest kangaroo-multi prints for the undivided stream.
int kangaroo_multi_roundtrip_selftest(const std::vector<std::string> &a)
{
    if (a.size() < 4) return 2;
    Scalar lo, hi;
    if (!hs::fe_from_hex(lo, a[0]) || !hs::fe_from_hex(hi, a[1])) return 2;
    const Scalar w = hs::sc_sub(hi, lo);
    if (w.l[2] || w.l[3]) return 2;
    const u128 W = (((u128)w.l[1] << 64) | w.l[0]) + 1;
    std::vector<Affine> pubs;
    {
        std::stringstream ss(a[2]);
        std::string tok;
        while (std::getline(ss, tok, ',')) { Affine P; if (!hs::parse_pubkey(P, cut_hex(tok)) || !hs::on_curve(P)) return 2; pubs.push_back(P); }
    }
    if (pubs.empty() || pubs.size() > BSGS_KANGAROO_MAX_KEYS) return 2;
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
    const Affine aG = hs::point_mul(hs::G, lo);
    kang::WorkHeader h;
    h.version = kang::WORK_VERSION_KEYS;
    {
        MultiKeyTable first(lo, W, pubs);
        for (size_t k = 0; k < pubs.size(); k++)
            if (hs::fe_equal(pubs[k].x, aG.x) && hs::fe_equal(pubs[k].y, aG.y)) { first.presolve((uint32_t)k, lo); printf("presolved %zu\n", k); }
        for (size_t i = 0; i < split; i++) if (!multi_scripted_record(first, pubs.size(), a[4 + i])) return 2;
        std::vector<uint8_t> entries;
        kang::WorkKeys wk;
        first.write_entries(entries);
        first.write_keys(wk);
        h.table = first.size(); h.false_matches = first.false_matches(); h.reseeds = first.reseeds();
        for (size_t i = 0; i < split; i++) if (a[4 + i][0] != 'D') h.dps++;
        h.fingerprint = kang::keys_fingerprint(pubs, lo, hi, h);
        if (!kang::write_work_file(path, path + ".temp", h, entries, {}, {}, &wk)) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
    }
    kang::WorkFile wf;
    const std::string bad = kang::read_work_file(path, wf, true, kang::WORK_VERSION_KEYS);
    if (!keep) remove(path.c_str());
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    if (kang::keys_fingerprint(pubs, lo, hi, wf.h) != wf.h.fingerprint) { fprintf(stderr, "Recovery file was made with other settings\n"); return 1; }
    MultiKeyTable second(lo, W, pubs);
    if (!second.restore(wf.table.data(), wf.h.table, wf.h.false_matches, wf.h.reseeds, wf.keys)) { fprintf(stderr, "the table section does not load\n"); return 1; }
    for (size_t i = 4 + split; i < a.size(); i++) if (!multi_scripted_record(second, pubs.size(), a[i])) return 2;
    printf("summary %zu %llu %llu %llu %llu %u\n", second.size(), (unsigned long long)second.false_matches(), (unsigned long long)second.reseeds(),
           (unsigned long long)second.links_kept(), (unsigned long long)second.links_resolved(), second.solved());
    return 0;
}

// ---- bsgs_mi355x -kangaroo -infile FILE: every key of the list in [pk, pke] with ONE herd per engine -----------------------------------------------
namespace {
using namespace kang;
volatile sig_atomic_t multi_signalled = 0;
void multi_on_signal(int) { multi_signalled = 1; }

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

int kangaroo_multi_main(const KangConfig &c)
{
    Config fc; fc.infile = c.infile;
    const std::vector<std::string> pub_hex = read_pubs(fc);                       // the BSGS path's reader: same formats, same messages; a missing file ends the run here
    if (pub_hex.empty()) die("No public keys in " + c.infile);
    if (pub_hex.size() > BSGS_KANGAROO_MAX_KEYS) die("-kangaroo -infile: at most 65535 public keys, the file has " + std::to_string(pub_hex.size()));
    const uint32_t L = (uint32_t)pub_hex.size();
    std::vector<Affine> P(L);
    for (uint32_t k = 0; k < L; k++) if (!hs::parse_pubkey(P[k], pub_hex[k]) || !hs::on_curve(P[k])) die("Invalid Public Key (-infile, line " + std::to_string(k + 1) + ") length!!!");
    Scalar lo, hi;
    if (!hs::fe_from_hex(lo, c.pk) || hs::fe_is_zero(lo)) die("Start range can`t be zero");
    if (!hs::fe_from_hex(hi, c.pke)) die("Invalid range (-pkend) length!!!");
    if (hs::fe_cmp(hi, lo) <= 0) die("End range must be more then start range");
    const Scalar wm1 = hs::sc_sub(hi, lo);
    if (wm1.l[2] || wm1.l[3] || (wm1.l[1] >> 61)) die("-kangaroo: the range width must be at most 2^125");
    const u128 W = (((u128)wm1.l[1] << 64) | wm1.l[0]) + 1;
    if (W < ((u128)1 << 20)) die("-kangaroo: the range width must be at least 2^20");
    const double Wd = (double)W, sqrtW = std::sqrt(Wd);
    printf("Kangaroo range [%s, %s], width 2^%.2f, %u public keys\n", hs::fe_to_hex(lo).c_str(), hs::fe_to_hex(hi).c_str(), std::log2(Wd), L);
    // -wl: the work file is read before any device is looked for; only a version-3 file of this list, range and plan can be continued
    const bool resume = !c.wl.empty();
    WorkFile wf;
    std::string wl_path = c.wl;
    if (resume) {
        struct stat sb;
        if (stat(wl_path.c_str(), &sb) != 0 && stat((c.dir + "/" + c.wl).c_str(), &sb) == 0) wl_path = c.dir + "/" + c.wl;
        const std::string bad = read_work_file(wl_path, wf, true, WORK_VERSION_KEYS);
        if (!bad.empty()) die("-kangaroo -infile -wl: " + bad + " (only a kangaroo.work file of a key list can be resumed here; a BSGS recovery file is not supported in kangaroo mode)");
        std::vector<std::string> dl;
        { std::stringstream ss(c.devices); std::string tok; while (std::getline(ss, tok, ',')) dl.push_back(tok); }
        if (keys_fingerprint(P, lo, hi, wf.h) != wf.h.fingerprint || wf.keys.solved.size() != L || (c.dp >= 0 && (uint32_t)c.dp != wf.h.dp) || (c.kn && c.kn != wf.h.herd) ||
            (c.seed_given && c.seed != wf.h.seed) || (!dl.empty() && dl.size() != wf.h.engines) || !wf.h.engines || !wf.h.herd || !wf.h.per_thread || wf.h.herd % (64ull * wf.h.per_thread))
            die("Recovery file was made with other settings");
    } else { Config rc; rc.dir = c.dir; read_recovery(rc); }                      // (win.txt starts empty, as on the BSGS path; a resumed run appends to the one it has)
    const auto t0 = Clock::now();

    MultiKeyTable table(lo, W, P);
    std::mutex tab_m;                                                              // table, assigner, win.txt
    int found_n = 0;
    std::map<std::string, std::vector<uint32_t>> same;                            // list positions that hold the same point
    for (uint32_t k = 0; k < L; k++) same[hs::compress_pubkey(P[k])].push_back(k);
    // a key is known: its KEY[n] block on the console and in win.txt at once, through key_lines as the BSGS path writes it
    auto report = [&](uint32_t k) {
        std::string console;
        const std::string win = key_lines((int)k + 1, table.key(k), P[k], console);
        fputs(console.c_str(), stdout);
        fflush(stdout);
        std::ofstream f(c.dir + "/win.txt", std::ios::app | std::ios::binary);
        f << win;
        found_n++;
    };
    // keys solved before any device is opened: P_k == a*G has no affine Q_k; it keeps its slot (G stands in, no kangaroo is assigned)
    const Affine aG = hs::point_mul(hs::G, lo), naG = hs::affine_neg(aG);
    std::vector<bool> presolved(L, false);
    std::vector<uint8_t> qxy(64 * (size_t)L);
    std::vector<Affine> Q(L);
    for (uint32_t k = 0; k < L; k++) {
        Q[k] = hs::point_add(P[k], naG);
        if (Q[k].inf) { presolved[k] = true; table.presolve(k, lo); if (resume) found_n++; else report(k); Q[k] = hs::G; }
        hs::affine_to_le(Q[k], &qxy[64 * (size_t)k], &qxy[64 * (size_t)k + 32]);
    }
    double elapsed_before = 0.0;
    if (resume) {                                                                  // the file's solved keys are in win.txt already: counted, not written again
        const uint32_t before = table.solved();
        if (!table.restore(wf.table.data(), wf.h.table, wf.h.false_matches, wf.h.reseeds, wf.keys)) die("-kangaroo -wl: the table section of " + wl_path + " does not load");
        std::vector<uint8_t>().swap(wf.table);
        found_n += (int)(table.solved() - before);
        elapsed_before = wf.h.elapsed;
    }
    const uint32_t open0 = L - table.solved();
    if (!open0) { printf("Found %d of %u\n", found_n, L); return 0; }

    std::vector<int> gpus;
    {
        int ngpu = 0;
        CK(bsgs_dev_count(&ngpu));
        if (ngpu <= 0) die("No GPU found");
        if (c.devices.empty()) for (int i = 0; i < ngpu; i++) gpus.push_back(i);
        else { std::stringstream ss(c.devices); std::string tok; while (std::getline(ss, tok, ',')) gpus.push_back(atoi(tok.c_str())); }
    }
    int cus = 256;
    { bsgs_dev *d = nullptr; CK(bsgs_dev_open(gpus[0], &d)); bsgs_dev_cu_count(d, &cus); bsgs_dev_close(d); }
    // dp, kn, the jump mean and the launch length from W, as for one key
    if (resume && gpus.size() != wf.h.engines) die("Recovery file was made with other settings");
    Plan pl = plan_herd(sqrtW, (uint32_t)gpus.size(), cus, resume ? (int)wf.h.dp : c.dp, c.kn);
    if (resume) { pl.kn = wf.h.herd; pl.G = wf.h.per_thread; }                      // the plan of the run that saved, not this GPU's
    const uint64_t kn = pl.kn;
    if (kn > (1ull << 26)) die("-kn: at most 2^26 kangaroos per engine");
    const double Nk = (double)kn * pl.engines, overhead = Nk * std::ldexp(1.0, (int)pl.dp);
    pl.expected = 2.0 * sqrtW + overhead;
    pl.S = (uint32_t)std::max(8.0, std::min(1024.0, pl.expected / Nk / 8.0));
    pl.cap = (uint32_t)std::min<double>(1u << 22, 2.0 * (double)kn * pl.S / std::ldexp(1.0, (int)pl.dp) + 65536.0);
    uint64_t seed = c.seed;
    if (resume) seed = wf.h.seed;
    else if (!c.seed_given) { std::random_device rd; seed = ((uint64_t)rd() << 32) ^ rd(); }
    printf("Kangaroo: %u engine(s) x %llu kangaroos (%u per thread), -dp %u, %u steps per launch, -kseed 0x%llx\n", pl.engines, (unsigned long long)kn, pl.G, pl.dp, pl.S,
           (unsigned long long)seed);
    const double exp_lo = 2.0 * std::sqrt((double)open0 * Wd) + overhead, exp_hi = (double)open0 * 2.0 * sqrtW + overhead;
    // (the give-up bound: 20 times L_open 2 sqrt(W) + overhead steps without a new key, L_open the keys open at that moment)
    printf("Expected steps for %u keys: between 2^%.2f (2 sqrt(L W)) and 2^%.2f (L 2 sqrt(W)), DP overhead included\n", open0, std::log2(exp_lo), std::log2(exp_hi));

    uint64_t rng = seed;
    std::mutex rng_m;
    const double mean = std::max(1.0, std::min(std::ldexp(1.0, 62), Nk * sqrtW / 4.0));
    std::vector<uint64_t> js(BSGS_KANGAROO_JUMPS);
    std::vector<uint8_t> jxy(64 * (size_t)BSGS_KANGAROO_JUMPS);
    for (int j = 0; j < BSGS_KANGAROO_JUMPS; j++) {
        const uint64_t span = (uint64_t)(2.0 * mean) > 1 ? (uint64_t)(2.0 * mean) - 1 : 1;
        js[j] = 1 + splitmix64(rng) % span;
        hs::affine_to_le(hs::point_mul(hs::G, hs::fe_from_u64(js[j])), &jxy[64 * j], &jxy[64 * j + 32]);
    }
    WorkHeader wh;                                                                 // what every save of this run shares
    wh.version = WORK_VERSION_KEYS; wh.engines = pl.engines; wh.dp = pl.dp; wh.per_thread = pl.G; wh.herd = kn; wh.seed = seed;
    wh.fingerprint = keys_fingerprint(P, lo, hi, wh);
    const std::string work_path = c.dir + "/kangaroo.work", work_tmp = c.dir + "/kangaroo.temp";
    const uint64_t half = kn / 2;                                                  // kangaroos [0, half) of an engine are tame, [half, kn) wild
    Assigner asg(L, presolved, (kn - half) * pl.engines);
    std::vector<std::vector<bsgs_kangaroo_state>> herds(pl.engines), saved(pl.engines);      // -wl: the file's herds; the herds as downloaded for a save
    if (resume) {
        std::vector<uint32_t> keys((kn - half) * pl.engines);
        for (uint32_t e = 0; e < pl.engines; e++) {
            herds[e].resize(kn);
            memcpy(herds[e].data(), wf.herds[e].data(), kn * sizeof(bsgs_kangaroo_state));
            std::vector<uint8_t>().swap(wf.herds[e]);
            for (uint64_t i = half; i < kn; i++) {
                const uint32_t k = (herds[e][i].flags >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu;
                if (k >= L) die("-kangaroo -wl: a kangaroo of " + wl_path + " names key " + std::to_string(k));
                keys[(uint64_t)e * (kn - half) + (i - half)] = k;
            }
        }
        asg.restore(keys, table);
    }
    std::unique_ptr<Comb> comb;
    if (c.cpuseed) comb.reset(new Comb());

    std::atomic<bool> stop{false};
    std::atomic<uint64_t> steps{0}, dps{0}, dropped{0};
    std::mutex q_m; std::condition_variable q_cv;
    std::deque<std::pair<uint32_t, std::vector<bsgs_kangaroo_record>>> queue;
    std::vector<std::unique_ptr<std::mutex>> reseed_m;
    std::vector<std::vector<uint32_t>> reseed(pl.engines);
    std::vector<uint64_t> engine_records(pl.engines, 0);
    for (uint32_t e = 0; e < pl.engines; e++) reseed_m.emplace_back(new std::mutex);
    std::mutex err_m; std::string err;
    if (resume) {
        rng = wf.h.rng; steps = wf.h.steps; dps = wf.h.dps; dropped = wf.h.dropped;
        for (uint32_t e = 0; e < pl.engines; e++) reseed[e] = wf.reseed[e];
        printf("Resumed: %llu steps, %zu DPs, %u of %u keys solved\n", (unsigned long long)wf.h.steps, table.size(), table.solved(), L);
    }
    // saving ("a save is a consistent cut"): engines park between two launches with their herd downloaded
    std::atomic<bool> save_req{false};
    std::mutex save_m; std::condition_variable save_cv;
    uint32_t parked = 0, running = 0;
    bool collector_busy = false;                                                   // (under q_m) a batch has left the queue and is not in the table yet

    // under tab_m.  The consequences of FOUND events: the block is written, equal points of the list are solved with it, the key's kangaroos start afresh
    std::function<void(const std::vector<MultiKeyTable::Event> &)> on_events = [&](const std::vector<MultiKeyTable::Event> &ev) {
        for (const MultiKeyTable::Event &x : ev) {
            if (x.what != MultiKeyTable::FOUND) continue;
            report(x.a);
            asg.solved(x.a);
            for (uint64_t w = 0; w < asg.keys().size(); w++) if (asg.keys()[w] == x.a) {
                const uint32_t e = (uint32_t)(w / (kn - half));
                std::lock_guard<std::mutex> lk(*reseed_m[e]);
                reseed[e].push_back((uint32_t)(half + w % (kn - half)));
            }
            for (uint32_t o : same[hs::compress_pubkey(P[x.a])]) if (!table.known(o)) {
                std::vector<MultiKeyTable::Event> more;
                table.found(o, x.key, more);
                on_events(more);
            }
        }
        if (table.solved() == L) stop = true;
    };
    // offsets and keys of the kangaroos idx (local indices of engine e): under the stream's lock and the table's
    auto draw = [&](uint32_t e, const std::vector<uint32_t> &idx, std::vector<uint32_t> &use, std::vector<i128> &d, std::vector<uint32_t> &fl, std::vector<uint32_t> &key) {
        std::lock_guard<std::mutex> lt(tab_m);
        std::lock_guard<std::mutex> lk(rng_m);
        for (uint32_t i : idx) {
            const bool wild = i >= half;
            uint32_t k = 0;
            if (wild && !asg.reseed((uint64_t)e * (kn - half) + (i - half), table, &k)) continue;      // no key is open: the kangaroo rests
            use.push_back(i); fl.push_back(wild ? BSGS_KANGAROO_WILD : 0u); key.push_back(k);
            d.push_back(herd_offset(rng, W, wild));
        }
    };
    // Q_key + u G = infinity: k_key = a - u
    auto infinite_start = [&](uint32_t k, i128 d) {
        std::lock_guard<std::mutex> lt(tab_m);
        if (table.known(k)) return;
        std::vector<MultiKeyTable::Event> ev;
        table.found(k, hs::sc_add(lo, sc_from_i128(-d)), ev);
        on_events(ev);
    };
    // -kcpuseed: the same herd from the host's comb
    auto host_states = [&](const std::vector<i128> &d, const std::vector<uint32_t> &fl, const std::vector<uint32_t> &key, std::vector<bsgs_kangaroo_state> &out, int64_t *first_inf) {
        std::vector<hs::Jac> j(d.size());
        for (size_t q = 0; q < d.size(); q++) {
            const bool neg = d[q] < 0;
            hs::Jac p = comb->mul(neg ? (u128)-d[q] : (u128)d[q]);
            if (neg && !p.inf) p.y = hs::fe_neg(p.y);
            if (fl[q]) p = hs::jac_add_affine(p, Q[key[q]]);
            j[q] = p;
        }
        const std::vector<Affine> pts = hs::batch_to_affine(j);
        out.resize(d.size());
        *first_inf = -1;
        for (size_t q = 0; q < d.size(); q++) {
            bsgs_kangaroo_state &s = out[q];
            memset(&s, 0, sizeof s);
            if (!pts[q].inf) hs::affine_to_le(pts[q], s.x, s.y);
            else if (*first_inf < 0) *first_inf = (int64_t)q;
            memcpy(s.d, &d[q], 16);
            s.flags = fl[q] | key[q] << BSGS_KANGAROO_KEY_SHIFT | (pts[q].inf ? BSGS_KANGAROO_DEAD : 0u);
        }
    };
    // initial herds: offsets in engine order from the seeded stream, whoever computes the points
    std::vector<std::vector<i128>> off0(pl.engines);
    if (!resume) for (uint32_t e = 0; e < pl.engines; e++) { off0[e].resize(kn); for (uint64_t i = 0; i < kn; i++) off0[e][i] = herd_offset(rng, W, i >= half); }

    auto engine = [&](uint32_t e) {
        bsgs_dev *dev = nullptr;
        auto bad = [&](const char *what) { std::lock_guard<std::mutex> lk(err_m); if (err.empty()) err = std::string(what) + ": " + bsgs_last_error(); stop = true; };
        // one seed call: by range (idx empty) or by list; a start at infinity solves its key and the kangaroo is seeded again next round
        auto seed_call = [&](const std::vector<uint32_t> &idx, const std::vector<i128> &d, const std::vector<uint32_t> &fl, const std::vector<uint32_t> &key) -> bool {
            uint32_t ninf = 0, first = 0;
            if (c.cpuseed) {
                std::vector<bsgs_kangaroo_state> st;
                int64_t fi;
                host_states(d, fl, key, st, &fi);
                if ((idx.empty() ? bsgs_kangaroo_upload(dev, 0, (uint32_t)st.size(), st.data()) : bsgs_kangaroo_upload_list(dev, idx.data(), (uint32_t)idx.size(), st.data())) != BSGS_OK) { bad("bsgs_kangaroo_upload"); return false; }
                if (fi >= 0) { ninf = 1; first = (uint32_t)fi; }
            } else if (bsgs_kangaroo_seed_keys(dev, idx.empty() ? nullptr : idx.data(), 0, (uint32_t)d.size(), (const uint8_t *)d.data(), fl.data(), key.data(), &ninf, &first) != BSGS_OK) { bad("bsgs_kangaroo_seed_keys"); return false; }
            if (ninf) {
                if (fl[first]) infinite_start(key[first], d[first]);
                std::lock_guard<std::mutex> lk(*reseed_m[e]);
                reseed[e].push_back(idx.empty() ? first : idx[first]);
            }
            return true;
        };
        if (bsgs_dev_open(gpus[e], &dev) != BSGS_OK) { bad("bsgs_dev_open"); return; }
        bool ok = bsgs_kangaroo_setup(dev, jxy.data(), js.data(), pl.dp, (uint32_t)kn, pl.G, pl.cap) == BSGS_OK;
        if (!ok) bad("bsgs_kangaroo_setup");
        if (ok && bsgs_kangaroo_set_keys(dev, qxy.data(), L) != BSGS_OK) { bad("bsgs_kangaroo_set_keys"); ok = false; }
        if (ok && resume) {
            if (bsgs_kangaroo_upload(dev, 0, (uint32_t)kn, herds[e].data()) != BSGS_OK) { bad("bsgs_kangaroo_upload"); ok = false; }
            std::vector<bsgs_kangaroo_state>().swap(herds[e]);
        } else if (ok) {
            const auto ts = Clock::now();
            std::vector<uint32_t> fl(kn), key(kn, 0);
            for (uint64_t i = 0; i < kn; i++) { fl[i] = i >= half ? BSGS_KANGAROO_WILD : 0u; if (i >= half) key[i] = asg.key((uint64_t)e * (kn - half) + (i - half)); }
            ok = seed_call({}, off0[e], fl, key);
            std::vector<i128>().swap(off0[e]);
            std::lock_guard<std::mutex> lk(err_m);
            printf("[startup] %-44s %.3fs\n", ((c.cpuseed ? "herds (host), engine " : "herds (GPU), engine ") + std::to_string(e)).c_str(), since(ts));
        }
        std::vector<bsgs_kangaroo_record> recs(pl.cap);
        while (ok && !stop.load()) {
            std::vector<uint32_t> rs;
            { std::lock_guard<std::mutex> lk(*reseed_m[e]); rs.swap(reseed[e]); }
            if (!rs.empty()) {
                std::sort(rs.begin(), rs.end());
                rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
                std::vector<uint32_t> use, fl, key;
                std::vector<i128> d;
                draw(e, rs, use, d, fl, key);
                if (!use.empty() && !seed_call(use, d, fl, key)) break;
                if (stop.load()) break;
            }
            uint32_t n = 0;
            uint64_t drop = 0;
            if (bsgs_kangaroo_run(dev, pl.S, recs.data(), pl.cap, &n, &drop, nullptr) != BSGS_OK) { bad("bsgs_kangaroo_run"); break; }
            const uint64_t total = (steps += kn * pl.S);
            dropped += drop;
            { std::lock_guard<std::mutex> lk(q_m); queue.emplace_back(e, std::vector<bsgs_kangaroo_record>(recs.begin(), recs.begin() + n)); }
            q_cv.notify_one();
            if (c.ksteps && total >= c.ksteps) stop = true;
            if (save_req.load() && !stop.load()) {                       // between two launches: the herd as it stands, then wait for the file
                saved[e].resize(kn);
                if (bsgs_kangaroo_download(dev, 0, (uint32_t)kn, saved[e].data()) != BSGS_OK) { bad("bsgs_kangaroo_download"); ok = false; break; }
                std::unique_lock<std::mutex> lk(save_m);
                parked++;
                save_cv.notify_all();
                while (save_req.load() && !stop.load()) save_cv.wait_for(lk, std::chrono::milliseconds(100));
                parked--;
            }
        }
        bool all_solved;
        { std::lock_guard<std::mutex> lt(tab_m); all_solved = table.solved() == L; }
        if (ok && dev && !all_solved) {                                  // the run stops with keys open: the herd goes into the last save
            saved[e].resize(kn);
            if (bsgs_kangaroo_download(dev, 0, (uint32_t)kn, saved[e].data()) != BSGS_OK) { bad("bsgs_kangaroo_download"); saved[e].clear(); }
        }
        if (dev) bsgs_dev_close(dev);
        std::lock_guard<std::mutex> lk(save_m);
        running--;
        save_cv.notify_all();
    };
    // the work file from the state as it stands: callers make sure that no engine walks and the collector's queue is empty
    auto write_state = [&]() {
        std::lock_guard<std::mutex> lt(tab_m);
        WorkHeader h = wh;
        h.rng = rng; h.steps = steps.load(); h.dps = dps.load(); h.dropped = dropped.load();
        h.false_matches = table.false_matches(); h.reseeds = table.reseeds(); h.table = table.size();
        h.elapsed = elapsed_before + since(t0);
        std::vector<uint8_t> entries;
        entries.reserve(32 * table.size());
        table.write_entries(entries);
        WorkKeys wk;
        table.write_keys(wk);
        std::vector<const std::vector<bsgs_kangaroo_state> *> hp;
        std::vector<std::vector<uint32_t>> rs(pl.engines);
        for (uint32_t e = 0; e < pl.engines; e++) { hp.push_back(&saved[e]); std::lock_guard<std::mutex> lk(*reseed_m[e]); rs[e] = reseed[e]; }
        if (!write_work_file(work_path, work_tmp, h, entries, hp, rs, &wk)) fprintf(stderr, "WARNING: cannot write %s\n", work_path.c_str());
    };
    std::atomic<bool> engines_done{false};
    std::thread collector([&]() {
        for (;;) {
            std::pair<uint32_t, std::vector<bsgs_kangaroo_record>> b;
            {
                std::unique_lock<std::mutex> lk(q_m);
                collector_busy = false;
                q_cv.wait_for(lk, std::chrono::milliseconds(100), [&] { return !queue.empty() || engines_done.load(); });
                if (queue.empty()) { if (engines_done.load()) return; continue; }
                b = std::move(queue.front());
                queue.pop_front();
                collector_busy = true;
            }
            std::lock_guard<std::mutex> lt(tab_m);
            if (table.solved() == L) continue;
            engine_records[b.first] += b.second.size();
            std::vector<MultiKeyTable::Event> ev;
            for (const bsgs_kangaroo_record &r : b.second) {
                u128 d;
                memcpy(&d, r.d, 16);
                ev.clear();
                table.add(r.x, d, (uint32_t)(b.first * kn + r.kangaroo), r.flags, ev);
                if (!(r.flags & BSGS_KANGAROO_DEAD)) dps++;
                for (const MultiKeyTable::Event &x : ev) if (x.what == MultiKeyTable::RESEED) { std::lock_guard<std::mutex> lk(*reseed_m[b.first]); reseed[b.first].push_back(r.kangaroo); }
                on_events(ev);
            }
        }
    });
    multi_signalled = 0;
    signal(SIGINT, multi_on_signal);
    signal(SIGTERM, multi_on_signal);
    std::vector<std::thread> th;
    running = pl.engines;
    for (uint32_t e = 0; e < pl.engines; e++) th.emplace_back(engine, e);
    auto last_t = Clock::now(), last_save = Clock::now();
    uint64_t last_steps = steps.load(), steps_mark = last_steps;
    uint32_t last_solved = table.solved();
    bool gave_up = false, interrupted = false;
    while (!stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        const auto now = Clock::now();
        if (multi_signalled) { interrupted = true; stop = true; save_cv.notify_all(); break; }
        if (std::chrono::duration<double>(now - last_t).count() >= 2.0) {
            const uint64_t st = steps.load();
            uint32_t solved;
            { std::lock_guard<std::mutex> lt(tab_m); solved = table.solved(); }
            printf("\r[%u] %.3e steps/s  steps 2^%.2f of expected 2^%.2f..2^%.2f  solved %u/%u  DPs %llu  %.0fs   ", pl.engines, (st - last_steps) / std::chrono::duration<double>(now - last_t).count(),
                   st ? std::log2((double)st) : 0.0, std::log2(exp_lo), std::log2(exp_hi), solved, L, (unsigned long long)dps.load(), since(t0));
            fflush(stdout);
            last_steps = st; last_t = now;
        }
        {                                                                // give up: 20 times one key's expectation for every key still open, counted from the last key found
            uint32_t solved_now;
            { std::lock_guard<std::mutex> lt(tab_m); solved_now = table.solved(); }
            if (solved_now != last_solved) { last_solved = solved_now; steps_mark = steps.load(); }
            if ((double)(steps.load() - steps_mark) > 20.0 * ((double)(L - solved_now) * 2.0 * sqrtW + overhead)) { gave_up = true; stop = true; }
        }
        if (!stop.load() && std::chrono::duration<double>(now - last_save).count() >= (double)c.wt) {
            // -wt: every engine parks between two launches with its herd downloaded; the collector empties the queue; then table, keys, links, stream, herds
            // and re-seed lists belong to one moment of the search
            const auto ts = Clock::now();
            save_req = true;
            {
                std::unique_lock<std::mutex> lk(save_m);
                while (parked != running && !stop.load() && !multi_signalled) save_cv.wait_for(lk, std::chrono::milliseconds(100));
            }
            for (;;) {
                { std::lock_guard<std::mutex> lk(q_m); if ((queue.empty() && !collector_busy) || stop.load()) break; }
                std::this_thread::sleep_for(std::chrono::milliseconds(1));
            }
            bool all_parked;
            { std::lock_guard<std::mutex> lk(save_m); all_parked = parked == pl.engines; }
            if (all_parked && !stop.load()) { write_state(); printf("\n[save] %s in %.2fs\n", work_path.c_str(), since(ts)); }
            { std::lock_guard<std::mutex> lk(save_m); save_req = false; }
            save_cv.notify_all();
            last_save = Clock::now();
        }
    }
    save_cv.notify_all();
    for (auto &t : th) t.join();
    engines_done = true;
    q_cv.notify_all();
    collector.join();
    signal(SIGINT, SIG_DFL);
    signal(SIGTERM, SIG_DFL);
    if (!err.empty()) die(err);
    const bool all = table.solved() == L;
    const bool budget = !all && !gave_up && !interrupted && c.ksteps && steps.load() >= c.ksteps;
    if (all) remove(work_path.c_str());                                            // a stale file never outlives its job
    else {
        bool have = true;
        for (uint32_t e = 0; e < pl.engines; e++) have = have && saved[e].size() == kn;
        if (have) write_state();                                                   // engines joined, queue drained: the state is final
    }
    if (!all) {
        if (gave_up) printf("\nKangaroo: %u of %u keys open after 20 times the expected steps (are the keys in the range?)\n", L - table.solved(), L);
        else printf("\nKangaroo: stopped after %llu steps (%s), %u of %u keys open\n", (unsigned long long)steps.load(), budget ? "-ksteps" : "signal",
                    L - table.solved(), L);
    }
    printf("Job time %.2fs, %.3e kangaroo steps, %llu DPs (%zu in the table, %llu dropped), %llu false matches, %llu re-seeds, %llu links kept, %llu links resolved\n", elapsed_before + since(t0),
           (double)steps.load(), (unsigned long long)dps.load(), table.size(), (unsigned long long)dropped.load(), (unsigned long long)table.false_matches(),
           (unsigned long long)table.reseeds(), (unsigned long long)table.links_kept(), (unsigned long long)table.links_resolved());
    for (uint32_t e = 0; e < pl.engines; e++) printf("Engine %u (GPU #%d): %llu records\n", e, gpus[e], (unsigned long long)engine_records[e]);
    printf("Found %d of %u\n", found_n, L);
    fflush(stdout);
    return all ? 0 : (budget || interrupted) ? 3 : 1;
}
