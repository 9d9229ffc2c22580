// host_kangaroo.cpp -- bsgs_mi355x -kangaroo: Pollard's kangaroo (lambda) search of ONE public key in [pk, pke] for ranges too wide for a baby table
// (include/bsgs_hip.h "Kangaroo" states the walk).  Here: the command line, the plan's defaults, the table of distinguished points and KeyMode,
// what the one-key search puts behind the driver's seam (host_kangaroo_run.h: the prologue, the engines, the collector, saving and -wl are there; the work
// file is host_kangaroo_work.cpp).  Start points come from the GPU (bsgs_kangaroo_seed; -kcpuseed: the host's comb); the key goes to win.txt through the
// JobList as the BSGS path writes it.  -selftest kangaroo drives the table with a scripted record stream and no GPU; -selftest kangaroo-table-roundtrip puts
// it through a work file.
// -ksym runs the symmetric walk (the negation map; include/bsgs_hip.h "Kangaroo, symmetric walk"): offsets counted from the middle of the range, R jump points
// (-kjumps) of mean -kjumpscale * N_k sqrt(W) / 4, the collision rule with signs, cycles counted, a version-2 work file; -selftest kangaroo-sym / kangaroo-sym-roundtrip.
// -kdpdev keeps the distinguished points in device memory (include/bsgs_hip.h "Kangaroo, distinguished-point table in device memory"): the launch inserts and
// pairs them there, the device table is read where the herd is downloaded for a save and loaded at -wl -- all of that is DevDpTable's
// (host_kangaroo_dptable.h), KeyMode's member dpt; KeyMode says which type words are legal and judges the handed-back pairs by the table's own rule; the plan is
// a low dp and the full herd; -selftest kangaroo-dpdev (through DevDpTable::take) / kangaroo-dpdev-plan.
#include "host_kangaroo_dptable.h"

#include <unordered_map>

using namespace kang;
namespace {

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

}  // namespace

// ---- the table of distinguished points: keyed on the low 64 bits of x, shared by all engines ---------------------------------------------------------
class KangarooTable {
    struct Entry { u128 d; uint32_t kid; bool wild, neg; };
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
        const bool wild = flags & BSGS_KANGAROO_WILD;
        auto it = map_.find(k64);                                      // look the tag up ...
        if (it == map_.end()) { map_.emplace(k64, Entry{d, kid, wild, sym_ && wild && (flags & BSGS_KANGAROO_NEG)}); return NEW; }
        return judge(it->second, d, kid, flags, key);                  // ... and judge the record against that entry
    }
    // -kdpdev: a record the device table handed back as a duplicate, against the stored entry it came with (d, kangaroo, type: 0 tame, 1 wild, 3 wild with
    // NEG); the host's map is not touched.  The verdicts of add() for the same pair, never NEW
    Verdict add_pair(u128 ed, uint32_t ekid, uint32_t etype, u128 d, uint32_t kid, uint32_t flags, Scalar *key)
    {
        if (flags & BSGS_KANGAROO_DEAD) { reseeds_++; if (flags & BSGS_KANGAROO_CYCLE) cycles_++; return RESEED; }
        return judge(Entry{ed, ekid, (etype & 1u) != 0, sym_ && etype == 3u}, d, kid, flags, key);
    }
    Verdict judge(const Entry &e, u128 d, uint32_t kid, uint32_t flags, Scalar *key)
    {
        if (sym_) return judge_sym(e, d, kid, flags, key);
        const bool wild = flags & BSGS_KANGAROO_WILD;
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
    // a record's point is sigma Q + d G, sigma = 0 tame, +1 wild, -1 wild with NEG; equal x: sigma1 Q + d1 G = +-(sigma2 Q + d2 G), so for each sign with
    // sigma1 -+ sigma2 != 0 the candidate is k'' = (+-d2 - d1) / (sigma1 -+ sigma2) mod n (the divisor is +-1 or +-2), the key a + W/2 + k''
    Verdict judge_sym(const Entry &e, u128 d, uint32_t kid, uint32_t flags, Scalar *key)
    {
        const bool wild = flags & BSGS_KANGAROO_WILD, neg = wild && (flags & BSGS_KANGAROO_NEG);
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
namespace {
bool parse_range_pub(const std::string &pk, const std::string &pke, const std::string &pub, Scalar &lo, Scalar &hi, Affine &P, u128 &W)
{
    std::vector<Affine> pubs;
    if (!parse_range_pubs(pk, pke, pub, lo, hi, W, pubs) || pubs.size() != 1) return false;
    P = pubs[0];
    return true;
}
// one scripted record (T|W|D,<x hex>,<d hex>,<kangaroo>; sym: also N, a wild kangaroo with NEG, and C, a cycle's dead record) into the table: prints the
// verdict line of -selftest kangaroo.  dpt (-selftest kangaroo-dpdev): the record goes through DevDpTable::take as the device would hand it back -- paired: as
// the duplicate behind the stored half taken before it, never a dead record -- and is judged as take() names it
// kn (-selftest kangaroo-dpshard): the kangaroo numbers are global, and a re-seed names the engine and the index there: "reseed <engine> <index>"
bool scripted_record(KangarooTable &tab, const std::string &rec, bool sym = false, DevDpTable *dpt = nullptr, bool paired = false, uint64_t kn = 0)
{
    const std::vector<std::string> f = split_commas(rec);
    if (f.size() != 4 || f[0].size() != 1 || !strchr(paired ? (sym ? "TWN" : "TW") : (sym ? "TWDNC" : "TWD"), f[0][0])) return false;
    Scalar x;
    u128 d;
    if (!hs::fe_from_hex(x, f[1]) || !parse_hex128(f[2], d)) return false;
    bsgs_kangaroo_record r;
    memset(&r, 0, sizeof r);
    hs::fe_to_le(x, r.x);
    memcpy(r.d, &d, 16);
    r.kangaroo = (uint32_t)strtoul(f[3].c_str(), nullptr, 10);
    r.flags = f[0] == "W" ? BSGS_KANGAROO_WILD : f[0] == "D" ? BSGS_KANGAROO_DEAD : f[0] == "N" ? BSGS_KANGAROO_WILD | BSGS_KANGAROO_NEG :
              f[0] == "C" ? BSGS_KANGAROO_DEAD | BSGS_KANGAROO_CYCLE : 0u;
    DevDpTable off;
    const DevDpTable::Taken t = (dpt ? dpt : &off)->take_scripted(r, 0, paired);
    Scalar key;
    KangarooTable::Verdict v;
    u128 ed;
    if (t.kind == DevDpTable::PAIR) { memcpy(&ed, t.stored->d, 16); v = tab.add_pair(ed, t.stored->kangaroo, t.stored->flags, d, r.kangaroo, r.flags, &key); }
    else if (t.kind == DevDpTable::ALONE || t.kind == DevDpTable::NOT_MINE) v = tab.add(r.x, d, r.kangaroo, r.flags, &key);
    else return false;
    switch (v) {
    case KangarooTable::NEW: printf("new\n"); break;
    case KangarooTable::FOUND: printf("found %s\n", hs::fe_to_hex(key).c_str()); break;
    case KangarooTable::RESEED:
        if (kn) printf("reseed %llu %llu\n", (unsigned long long)(r.kangaroo / kn), (unsigned long long)(r.kangaroo % kn));
        else printf("reseed %s\n", f[3].c_str());
        break;
    case KangarooTable::FALSE_MATCH: printf("false\n"); break;
    case KangarooTable::REPEAT: printf("repeat\n"); break;
    }
    return true;
}
}  // namespace

// -selftest kangaroo <pk hex> <pke hex> <pubkey> <record>...  record = T|W|D,<x hex>,<d hex: 128-bit two's complement>,<kangaroo> (D: a dead record).
// Prints one line per record: "new", "found <key hex>", "reseed <kangaroo>", "false", "repeat"; then "summary <stored> <false matches> <reseeds>".
// -selftest kangaroo-sym: the same through the symmetric table (record types T, W, N, D, C); the summary line is "summary <stored> <false matches> <reseeds> <cycles>".
// -selftest kangaroo-dpdev [sym] <pk hex> <pke hex> <pubkey> <item>...: the hand-back rule of -kdpdev without a GPU, every item through DevDpTable::take.  An
// item is a scripted record as above -- what the device hands back alone: DEAD, tag 0, a full table -- and goes through the host's own map; or
// S,<tag hex>,<d hex>,<kangaroo>,<type> followed by its record: a duplicate, judged against the stored entry it came with.  The same verdict and summary lines.
static int table_selftest(const std::vector<std::string> &a, bool sym, bool dpdev, uint64_t kn = 0)
{
    if (a.size() < 3) return 2;
    Scalar lo, hi; Affine P; u128 W;
    if (!parse_range_pub(a[0], a[1], a[2], lo, hi, P, W)) return 2;
    KangarooTable tab(lo, W, P, sym);
    DevDpTable dpt;
    dpt.on = dpdev;
    if (!dpt.scripted_items(a, [&](const std::string &rec, bool paired) {
            return !(paired && dpt.half.flags > 1u && !(sym && dpt.half.flags == 3u)) && scripted_record(tab, rec, sym, &dpt, paired, kn); })) return 2;
    if (sym) printf("summary %zu %llu %llu %llu\n", tab.size(), (unsigned long long)tab.false_matches(), (unsigned long long)tab.reseeds(), (unsigned long long)tab.cycles());
    else printf("summary %zu %llu %llu\n", tab.size(), (unsigned long long)tab.false_matches(), (unsigned long long)tab.reseeds());
    return 0;
}
int kangaroo_selftest(const std::vector<std::string> &a) { return table_selftest(a, false, false); }
int kangaroo_sym_selftest(const std::vector<std::string> &a) { return table_selftest(a, true, false); }
int kangaroo_dpdev_selftest(const std::vector<std::string> &a)
{
    const bool sym = !a.empty() && a[0] == "sym";
    return table_selftest(sym ? std::vector<std::string>(a.begin() + 1, a.end()) : a, sym, true);
}

// -selftest kangaroo-dpshard [sym] <engines> <kn> <pk hex> <pke hex> <pubkey> <item>...: the items of kangaroo-dpdev as the E tables of -kdpshard hand them back,
// every kangaroo number global (engine * kn + index); the same verdict lines, but a re-seed names its engine and the index there
int kangaroo_dpshard_selftest(const std::vector<std::string> &a)
{
    const bool sym = !a.empty() && a[0] == "sym";
    const std::vector<std::string> b(a.begin() + (sym ? 1 : 0), a.end());
    if (b.size() < 5) return 2;
    const uint64_t engines = strtoull(b[0].c_str(), nullptr, 10), kn = strtoull(b[1].c_str(), nullptr, 10);
    if (!engines || engines > BSGS_KANGAROO_DPT_MAX_SHARDS || !kn) return 2;
    for (size_t i = 5; i < b.size(); i++) {                            // every kangaroo an item names is one of the engines'
        const std::vector<std::string> f = split_commas(b[i]);
        if (f.size() >= 4 && strtoull(f[3].c_str(), nullptr, 10) >= engines * kn) return 2;
    }
    return table_selftest(std::vector<std::string>(b.begin() + 2, b.end()), sym, true, kn);
}
// -selftest kangaroo-barrier <event>...: the barrier in front of the last drain before a save (SaveBarrier, host_kangaroo_run.h) without threads or a GPU.
// Two engines, A and B; events: open (the saver opens a save round and asks), withdraw (it takes the request back), stop, A / B (the engine arrives: in the
// stop round when stop has been said, else in the save round), exitA / exitB (the engine's thread ends).  After every event one line: the state of each engine
// that waits, "A=<wait|all|given-up> B=...", "-" for one that does not; an engine that passes (all) or is let go (given-up) waits no longer and may arrive again
int kangaroo_barrier_selftest(const std::vector<std::string> &a)
{
    SaveBarrier b;
    bool save_req = false, stop = false, waits[2] = {false, false}, stopped[2] = {false, false};
    uint64_t round[2] = {0, 0};
    uint32_t living = 2;
    const char *names[] = {"wait", "all", "given-up"};
    for (const std::string &ev : a) {
        if (ev == "open") { b.open(); save_req = true; }
        else if (ev == "withdraw") save_req = false;
        else if (ev == "stop") stop = true;
        else if (ev == "A" || ev == "B") { const int e = ev == "B"; if (waits[e]) return 2; stopped[e] = stop; round[e] = b.arrive(stop); waits[e] = true; }
        else if (ev == "exitA" || ev == "exitB") { if (!living) return 2; living--; waits[ev == "exitB"] = false; }
        else return 2;
        std::string line;
        for (int e = 0; e < 2; e++) {
            const SaveBarrier::State st = b.state(stopped[e], round[e], living, save_req, stop);
            line += std::string(e ? " B=" : "A=") + (waits[e] ? names[st] : "-");
            if (waits[e] && st != SaveBarrier::WAIT) waits[e] = false;      // it passes, or it is let go
        }
        printf("%s\n", line.c_str());
    }
    return 0;
}

// -selftest kangaroo-dpshard-plan <pk hex> <pke hex> <CUs> <min launch> <dp or -1> <kn or 0> <kdpn or 0> <engines>: the plan of -kdpshard without a GPU, one
// line: "plan <dp> <kn> <per thread> <S> <record buffer> <capacity per engine> <engines>"; with 1 engine the numbers of kangaroo-dpdev-plan
int kangaroo_dpshard_plan_selftest(const std::vector<std::string> &a)
{
    if (a.size() != 8) return 2;
    KangConfig c;
    c.pk = a[0]; c.pke = a[1]; c.dp = atoi(a[4].c_str()); c.kdpn = strtoull(a[6].c_str(), nullptr, 0);
    Prologue p(c);
    const uint32_t engines = (uint32_t)strtoul(a[7].c_str(), nullptr, 10);
    if (!engines || engines > BSGS_KANGAROO_DPT_MAX_SHARDS) { fprintf(stderr, "kangaroo-dpshard-plan: %s engines, a table is divided over 1..16\n", a[7].c_str()); return 2; }
    DevDpTable dpt;
    Plan pl = plan_herd(p.sqrtW, engines, atoi(a[2].c_str()), dpt.plan(c, p.sqrtW, 0, engines), strtoull(a[5].c_str(), nullptr, 0));
    plan_launch(pl, p.sqrtW, 0.0, atof(a[3].c_str()), true, c.dp < 0);
    printf("plan %u %llu %u %u %u %llu %u\n", pl.dp, (unsigned long long)pl.kn, pl.G, pl.S, pl.cap, (unsigned long long)dpt.capacity, engines);
    return 0;
}

// -selftest kangaroo-dpdev-plan <pk hex> <pke hex> <CUs> <min launch> <dp or -1> <kn or 0> <kdpn or 0>: the plan of -kdpdev for one engine without a GPU, one line:
// "plan <dp> <kn> <per thread> <S> <record buffer> <capacity>" -- that of -kdpkeys (host_kangaroo_multi.cpp) for one open key
int kangaroo_dpdev_plan_selftest(const std::vector<std::string> &a)
{
    std::vector<std::string> b(a);
    b.push_back("1");
    return a.size() == 7 ? kangaroo_dpkeys_plan_selftest(b) : 2;
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
    bool keep;
    const std::string path = selftest_work_path(keep);
    if (path.empty()) return 2;
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
    bool ksym = false, kwalk_sym = false, wt_given = false, ktames_sym = false, ktames_plain = false;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        for (auto &ch : a) ch = (char)tolower(ch);
        auto next = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
        if (a == "-kangaroo") continue;
        else if (a == "-h") { usage(Config()); exit(0); }
        else if (a == "-pb") { c.pub = cut_hex(next()); c.pub_given = true; }
        else if (a == "-infile") c.infile = next();
        else if (a == "-pk") { c.pk = cut_hex(next()); c.range_given = true; }
        else if (a == "-pke") { c.pke = cut_hex(next()); c.range_given = true; }
        else if (a == "-d") c.devices = next();
        else if (a == "-dir") c.dir = next();
        else if (a == "-dp") { c.dp = atoi(next().c_str()); if (c.dp < 0 || c.dp > 32) die("-dp must be 0..32"); }
        else if (a == "-kn") c.kn = strtoull(next().c_str(), nullptr, 10);
        else if (a == "-kseed") { c.seed = strtoull(next().c_str(), nullptr, 0); c.seed_given = true; }
        else if (a == "-wl") c.wl = next();
        else if (a == "-wt") { c.wt = std::max(30, atoi(next().c_str())); wt_given = true; }
        else if (a == "-ktamesgen") c.ktamesgen = next();
        else if (a == "-ktames") { c.ktames = next(); ktames_plain = true; }
        else if (a == "-ktamessym") { c.ktames = next(); ktames_sym = true; }
        else if (a == "-ktamesdev") c.ktamesdev = true;
        else if (a == "-ktamesfrom") c.ktamesfrom = next();
        else if (a == "-ktamesmerge") c.ktamesmerge = next();
        else if (a == "-ktnplan") { c.ktnplan = strtoull(next().c_str(), nullptr, 0); if (!c.ktnplan || c.ktnplan > (1ull << 31)) die("-ktnplan must be 1..2^31"); }
        else if (a == "-ktn") { c.ktn = strtoull(next().c_str(), nullptr, 0); if (!c.ktn || c.ktn > (1ull << 31)) die("-ktn must be 1..2^31"); }
        else if (a == "-ksteps") { c.ksteps = strtoull(next().c_str(), nullptr, 10); if (!c.ksteps) die("-ksteps must be at least 1"); }
        else if (a == "-kcpuseed") c.cpuseed = true;
        else if (a == "-kdpdev") c.kdpdev = true;
        else if (a == "-kdpkeys") c.kdpkeys = true;
        else if (a == "-kdpshard") c.kdpshard = true;
        else if (a == "-kdpn") { c.kdpn = strtoull(next().c_str(), nullptr, 0); if (!c.kdpn || c.kdpn > (1ull << 31)) die("-kdpn must be 1..2^31"); }
        else if (a == "-ksym") ksym = true;
        else if (a == "-kwalk") { const std::string w = next(); if (w != "plain" && w != "sym") die("-kwalk must be plain or sym"); kwalk_sym = w == "sym"; }
        else if (a == "-noverify") c.verify = false;
        else if (a == "-kjumps") { c.jumps = (uint32_t)strtoul(next().c_str(), nullptr, 10); if (c.jumps < 64 || c.jumps > BSGS_KANGAROO_SYM_MAX_JUMPS || (c.jumps & (c.jumps - 1))) die("-kjumps must be a power of two, 64..4096"); }
        else if (a == "-kjumpscale") { c.jumpscale = atof(next().c_str()); if (!(c.jumpscale >= 1.0 / 64 && c.jumpscale <= 64.0)) die("-kjumpscale must be 1/64..64"); }
        else if (a == "-w" || a == "-htsz" || a == "-onlygen") die("-kangaroo cannot be combined with " + a + " (no baby table)");
        else die("Unknown parameter with -kangaroo: " + a);
    }
    // -kdpdev: the table of distinguished points of the one-key search, plain and -ksym, in device memory; every refusal before any device is looked for
    if (c.kdpn && !c.kdpdev && !c.kdpkeys && !c.kdpshard) die("-kdpn belongs to -kdpdev or -kdpkeys, or to -kdpshard (the capacity of the table in GPU memory)");
    // -kdpshard: that table divided over the engines of -d (without -d: every GPU, as plain -kangaroo), -kdpn entries on each
    if (c.kdpshard) {
        if (c.kdpdev) die("-kangaroo -kdpshard cannot be combined with -kdpdev (-kdpdev is one table on one engine, -kdpshard one table divided over the engines of -d)");
        if (c.kdpkeys) die("-kangaroo -kdpshard cannot be combined with -kdpkeys (the table of a key list stays on one engine)");
        if (!c.infile.empty()) die("-kangaroo -kdpshard cannot be combined with -infile (the divided table pairs the records of one key)");
        if (!c.ktames.empty() || !c.ktamesgen.empty() || !c.ktamesmerge.empty() || c.ktamesdev || !c.ktamesfrom.empty() || c.ktnplan || c.ktn)
            die("-kangaroo -kdpshard cannot be combined with -ktames, -ktamessym, -ktamesgen or their flags (a tame table is matched or grown by calls of its own)");
    }
    // one engine with one table: one -d entry; without -d a run takes every GPU of the machine, here it takes the first
    auto one_engine = [&c](const std::string &flag) {
        if (c.devices.find(',') != std::string::npos) die("-kangaroo " + flag + " takes one -d entry (several engines would need one table for all of them)");
        if (c.devices.empty()) {
            c.devices = "0";
            printf("Kangaroo %s: no -d given, one engine on GPU #0\n", flag.c_str());
        }
    };
    // -kdpkeys: the same for the list of -infile, plain and -kwalk sym, with an owner per entry
    if (c.kdpkeys) {
        if (c.kdpdev) die("-kangaroo -kdpkeys cannot be combined with -kdpdev (-kdpdev is the table of one key, -kdpkeys that of a key list)");
        if (c.pub_given) die("-kangaroo -kdpkeys cannot be combined with -pb (the table in GPU memory of one key is -kdpdev)");
        if (c.infile.empty()) die("-kangaroo -kdpkeys needs -infile (it keeps the table of a key list in GPU memory)");
        if (!c.ktames.empty() || !c.ktamesgen.empty() || !c.ktamesmerge.empty() || c.ktamesdev || !c.ktamesfrom.empty() || c.ktnplan || c.ktn)
            die("-kangaroo -kdpkeys cannot be combined with -ktames, -ktamessym, -ktamesgen or their flags (a tame table is matched or grown by calls of its own)");
        one_engine("-kdpkeys");
    }
    if (c.kdpdev) {
        if (!c.infile.empty()) die("-kangaroo -kdpdev cannot be combined with -infile (the table in GPU memory pairs the records of one key; -kdpkeys keeps the table of a key list there)");
        if (!c.ktames.empty() || !c.ktamesgen.empty() || !c.ktamesmerge.empty())
            die("-kangaroo -kdpdev cannot be combined with -ktames, -ktamessym, -ktamesgen or -ktamesmerge (a tame table is matched or grown by calls of its own)");
        one_engine("-kdpdev");
    }
    // a tame table (host_kangaroo_tames.cpp): made by the plain walk, or with -kwalk sym by the symmetric walk (file version 2); searched with -ktames,
    // a table of the symmetric walk with -ktamessym; never saved; every refusal before any device is looked for
    if (c.ktamesdev && c.ktamesgen.empty()) die("-ktamesdev belongs to -ktamesgen (the table that grows in GPU memory is the one being made)");
    if (c.ktamesdev && c.devices.find(',') != std::string::npos) die("-kangaroo -ktamesgen -ktamesdev takes one -d entry (a table grown on several GPUs would have to be merged)");
    // extending a table (-ktamesfrom), planning for its final size (-ktnplan), merging tables (-ktamesmerge): all three belong to -ktamesgen
    if (!c.ktamesfrom.empty() && (c.ktamesgen.empty() || !c.ktamesdev)) die("-ktamesfrom belongs to -ktamesgen -ktamesdev (a table is extended in GPU memory)");
    if (c.ktnplan && c.ktamesgen.empty()) die("-ktnplan belongs to -ktamesgen");
    if (c.ktnplan && !c.ktamesfrom.empty()) die("-ktnplan cannot be combined with -ktamesfrom (the walk comes from the table that is extended)");
    if (c.ktnplan && c.ktnplan < c.ktn) die("-ktnplan must not be below -ktn (it is the size the table is meant to reach)");
    if (!c.ktamesmerge.empty()) {
        if (c.ktamesgen.empty()) die("-ktamesmerge belongs to -ktamesgen (the file the merged table is written to)");
        if (c.ktamesdev || !c.ktamesfrom.empty() || c.ktnplan) die("-ktamesmerge cannot be combined with -ktamesdev, -ktamesfrom or -ktnplan (tables are merged on the host, nothing walks)");
    }
    if (!c.ktamesgen.empty() || !c.ktames.empty()) {
        const std::string flag = c.ktames.empty() ? "-ktamesgen" : ktames_sym ? "-ktamessym" : "-ktames";
        if (ktames_sym && ktames_plain) die("-ktames and -ktamessym exclude each other (one table, made by one walk)");
        if (!c.ktamesgen.empty() && !c.ktames.empty()) die("-ktamesgen and " + flag + " exclude each other (make the table first, then search with it)");
        if (ksym) die("-kangaroo " + flag + " cannot be combined with -ksym (-ksym is the search of one key without a table; a tame table of the symmetric walk is made with -ktamesgen -kwalk sym and searched with -ktamessym)");
        if (kwalk_sym && !c.ktames.empty()) die("-kangaroo " + flag + " cannot be combined with -kwalk sym (the table names its walk: -ktames searches a table of the plain walk, -ktamessym one of the symmetric walk)");
        c.tames_sym = c.ktames.empty() ? kwalk_sym : ktames_sym;
        if (ktames_sym && (c.jumps || c.jumpscale != 0.0)) die("-kangaroo -ktamessym takes no -kjumps or -kjumpscale (they belong to -ktamesgen -kwalk sym; the search takes them from the table)");
        if (!c.wl.empty()) die("-kangaroo " + flag + " cannot be combined with -wl (nothing is saved, so nothing is resumed)");
        if (c.ktames.empty()) {
            if (wt_given) die("-kangaroo -ktamesgen cannot be combined with -wt (nothing is saved but the table)");
            if (!c.ktn && c.ktamesmerge.empty()) die("-kangaroo -ktamesgen needs -ktn (the entries of the table)");
            if (c.pub_given || !c.infile.empty()) die("-kangaroo -ktamesgen takes no -pb or -infile (a tame table serves every key of its range)");
        } else {
            if (c.dp >= 0) die("-kangaroo " + flag + " cannot be combined with -dp (the table names its own)");
            if (c.ktn) die("-ktn belongs to -ktamesgen");
            if (c.pub_given && !c.infile.empty()) die("-kangaroo: -pb and -infile exclude each other (the keys come from the file)");
            if (!c.pub_given && c.infile.empty()) die("-kangaroo " + flag + " needs -pb or -infile");
        }
        return c;
    }
    if (c.ktn) die("-ktn belongs to -ktamesgen");
    // -kwalk sym: the symmetric walk of whatever is searched -- one key (-pb; the same as -ksym) or the list of -infile
    c.symlist = kwalk_sym && !c.infile.empty();
    c.sym = ksym || (kwalk_sym && c.infile.empty());
    if (!c.sym && !c.symlist && (c.jumps || c.jumpscale != 0.0)) die("-kjumps and -kjumpscale belong to -ksym");
    if (!c.infile.empty()) {
        if (c.pub_given) die("-kangaroo: -pb and -infile exclude each other (the keys come from the file)");
        if (ksym) die("-kangaroo -ksym cannot be combined with -infile: -ksym is the symmetric walk for one key (-kwalk sym searches a list with the symmetric walk)");
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

uint64_t kang::dpdev_capacity(double sqrtW, uint64_t kdpn)
{
    if (kdpn) return kdpn;
    uint64_t cap = 1ull << 16;
    while (cap < (1ull << 27) && (double)cap < 4.0 * sqrtW) cap *= 2;
    return cap;
}
uint32_t kang::dpdev_dp(double sqrtW, uint64_t capacity)
{
    return (uint32_t)std::min(32.0, std::max(0.0, std::ceil(std::log2(4.0 * sqrtW / (double)capacity))));
}

// ---- KeyMode: what the search of one key, plain or -ksym, puts behind the driver's seam ---------------------------------------------------------------
namespace {
struct KeyMode : Mode {
    KeyMode(const KangConfig &c, const Affine &P) : c(c), P(P)
    {
        if (c.sym) { version = WORK_VERSION_SYM; min_launch = 2.0 * BSGS_KANGAROO_CYCLE_WINDOW; }      // -ksym: a launch longer than the cycle window
        dpt.enable(c, *this);
    }
    std::string fingerprint(const Prologue &p, const WorkHeader &h) const override { return kangaroo_fingerprint(P, p.lo, p.hi, h); }
    bool before_devices(Prologue &p) override
    {
        pro = &p;
        const WorkHeader &f = p.wf.h;
        if (p.resume && ((c.jumps && c.jumps != f.jumps) || (c.jumpscale != 0.0 && c.jumpscale != f.jumpscale))) die("Recovery file was made with other settings");
        if (c.sym) {
            jumps = p.wh.jumps = p.resume ? f.jumps : c.jumps ? c.jumps : 1024u;
            jumpscale = p.wh.jumpscale = p.resume ? f.jumpscale : c.jumpscale != 0.0 ? c.jumpscale : KSYM_JUMPSCALE;
        }
        printf("Kangaroo range [%s, %s], width 2^%.2f\n", hs::fe_to_hex(p.lo).c_str(), hs::fe_to_hex(p.hi).c_str(), std::log2((double)p.W));
        if (c.kdpdev && p.resume && f.engines != 1) die("Recovery file was made with other settings");      // (-kdpdev is one engine with one table)
        if (c.kdpdev) dp_fixed = dpt.plan(c, p.sqrtW, p.resume ? f.table : 0);
        if (c.kdpshard && p.resume && f.engines > BSGS_KANGAROO_DPT_MAX_SHARDS) die("Recovery file was made with other settings");
        // -ksym: offsets are counted from the middle of the range, k'' = k - (a + W/2) (include/bsgs_hip.h "Kangaroo, symmetric walk")
        base = c.sym ? hs::sc_add(p.lo, hs::sc_from_u128(p.W / 2)) : p.lo;
        Q = hs::point_add(P, hs::affine_neg(hs::point_mul(hs::G, base)));
        hs::affine_to_le(Q, qxy, qxy + 32);
        verify_q = qxy;
        if (Q.inf) verify_skip = "the key is -pk itself, there is no affine Q to check a herd against";
        jobs.reset(new JobList({c.pub}, Recovery(), c.dir, [](int, const std::string &, const Scalar &) {}));      // win.txt as the BSGS path writes it
        { Config rc; rc.dir = c.dir; read_recovery(rc); }                                                  // (win.txt starts empty, as there: the key was not found yet)
        jobs->open_lanes(1);
        jobs->claim(0, cl);
        printf("\nFindpubkey  : %s\n", hs::compress_pubkey(P).c_str());
        return true;
    }
    // -kdpshard: the engines are known, so is each one's share of the table, and with it dp
    void engines_known(Prologue &p) override
    {
        if (!c.kdpshard) return;
        if (p.gpus.size() > BSGS_KANGAROO_DPT_MAX_SHARDS) die("-kangaroo -kdpshard takes at most 16 engines");
        dp_fixed = dpt.plan(c, p.sqrtW, p.resume ? p.wf.h.table : 0, (uint32_t)p.gpus.size());
    }
    // after the prologue: the table (-wl: the file's), the offsets of the initial herds in engine order from the seeded stream, whoever computes the points,
    // and with the host's comb the herds themselves, on up to 16 threads, before any engine starts
    void prepare(Prologue &p, Shared &sh)
    {
        table.reset(new KangarooTable(p.lo, p.W, P, c.sym));
        if (p.resume) {
            const bool sym = c.sym;                                    // the type words of a table entry: 0 tame, 1 wild, -ksym: 3 wild with NEG
            if (dpt.on && !dpt.split(p.wf.table, [sym](uint32_t type) { return type <= 1u || (sym && type == 3u); })) die("-kangaroo -wl: the table section of " + p.wl_path + " does not load");
            if (!table->restore(p.wf.table.data(), p.wf.table.size() / 32, p.wf.h.false_matches, p.wf.h.reseeds)) die("-kangaroo -wl: the table section of " + p.wl_path + " does not load");
            std::vector<uint8_t>().swap(p.wf.table);
            table->set_cycles(p.wf.h.cycles);
            printf("Resumed: %llu steps, %zu DPs\n", (unsigned long long)p.wf.h.steps, table_size());
        }
        p.t0 = Clock::now();
        // the host's comb: -kcpuseed, and Q at infinity (the key is -pk itself: no affine Q to hand to the kernel; the host's additions take it as it is)
        cpuseed = c.cpuseed || Q.inf;
        if (cpuseed) comb.reset(new Comb());
        if (p.resume) return;
        const uint64_t kn = p.pl.kn;
        off0.resize(p.pl.engines);
        for (uint32_t e = 0; e < p.pl.engines; e++) {
            off0[e].resize(kn);
            for (uint64_t i = 0; i < kn; i++) off0[e][i] = offset(sh.rng, i >= kn / 2);
        }
        if (!cpuseed) return;
        for (uint32_t e = 0; e < p.pl.engines; e++) {
            p.herds[e].resize(kn);
            const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
            std::vector<std::thread> tt;
            for (unsigned q = 0; q < nt; q++) tt.emplace_back([&, q]() {
                const uint64_t b0 = kn * q / nt, b1 = kn * (q + 1) / nt;
                std::vector<i128> dd(off0[e].begin() + (long)b0, off0[e].begin() + (long)b1);
                std::vector<uint32_t> ff(b1 - b0);
                for (uint64_t i = b0; i < b1; i++) ff[i - b0] = i >= kn / 2 ? BSGS_KANGAROO_WILD : 0u;
                std::vector<bsgs_kangaroo_state> st;
                host_states(dd, ff, st, sh);
                std::copy(st.begin(), st.end(), p.herds[e].begin() + (long)b0);
            });
            for (auto &t : tt) t.join();
            std::vector<i128>().swap(off0[e]);
        }
        printf("[startup] %-44s %.3fs\n", "herds (host)", since(p.t0));
    }
    i128 offset(uint64_t &rng, bool wild) const { return c.sym ? herd_offset_sym(rng, pro->W, wild) : herd_offset(rng, pro->W, wild); }
    // Q + u G = infinity: k' = -u; a start at infinity IS the key
    void infinite_start(i128 d, Shared &sh)
    {
        std::lock_guard<std::mutex> lk(sh.rng_m);
        key = hs::sc_add(base, sc_from_i128(-d));
        found = true; sh.stop = true;
    }
    // the points from the host's comb, on the calling thread
    void host_states(const std::vector<i128> &d, const std::vector<uint32_t> &fl, std::vector<bsgs_kangaroo_state> &out, Shared &sh)
    {
        std::vector<const Affine *> q(d.size());
        for (size_t k = 0; k < d.size(); k++) q[k] = fl[k] ? &Q : nullptr;
        for (size_t k : comb_states(*comb, d, fl, q, out)) infinite_start(d[k], sh);
    }
    const char *setup(bsgs_dev *dev) override
    {
        const Plan &pl = pro->pl;
        if ((c.sym ? bsgs_kangaroo_setup_sym(dev, pro->jxy.data(), pro->js.data(), jumps, pl.dp, (uint32_t)pl.kn, pl.G, pl.cap)
                   : bsgs_kangaroo_setup(dev, pro->jxy.data(), pro->js.data(), pl.dp, (uint32_t)pl.kn, pl.G, pl.cap)) != BSGS_OK) return "bsgs_kangaroo_setup";
        return dpt.sharded ? nullptr : dpt.begin(dev);
    }
    const char *setup_engine(bsgs_dev *dev, uint32_t e) override      // -kdpshard: engine e's share of the table
    {
        const char *failed = setup(dev);
        return failed || !dpt.sharded ? failed : dpt.begin(dev, e);
    }
    std::string drain(bsgs_dev *dev, uint32_t e, Shared &sh) override { return dpt.drain(dev, e, sh); }
    // -kdpdev: the launch, the load at -wl and the read for a save are the device table's
    int launch(bsgs_dev *dev, uint32_t e, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t cap, uint32_t *n, uint64_t *dropped, Shared &sh) override
    {
        return dpt.on ? dpt.launch(dev, steps, recs, cap, n, dropped, sh, e) : Mode::launch(dev, e, steps, recs, cap, n, dropped, sh);
    }
    std::string resumed(bsgs_dev *dev, uint32_t e, Shared &) override { return dpt.resumed(dev, pro->wl_path, e); }
    std::string fetch(bsgs_dev *dev, uint32_t e, Shared &) override { return dpt.fetch(dev, e); }
    size_t table_size() const { return table->size() + (size_t)dpt.entries.load(); }      // "in the table": the host's entries and the device's
    // (a whole herd from the host's comb was computed in prepare() and is uploaded by the driver: the comb is asked for lists only)
    const char *seed(bsgs_dev *dev, uint32_t e, const std::vector<uint32_t> &idx, Shared &sh) override
    {
        const uint64_t kn = pro->pl.kn;
        std::vector<i128> d;
        std::vector<uint32_t> fl(idx.empty() ? kn : idx.size());
        if (idx.empty()) {
            d.swap(off0[e]);
            for (uint64_t i = 0; i < kn; i++) fl[i] = i >= kn / 2 ? BSGS_KANGAROO_WILD : 0u;
        } else {                                                       // offsets from the shared stream (under its lock), in the order of idx
            d.resize(idx.size());
            std::lock_guard<std::mutex> lk(sh.rng_m);
            for (size_t k = 0; k < idx.size(); k++) { fl[k] = idx[k] >= kn / 2 ? BSGS_KANGAROO_WILD : 0u; d[k] = offset(sh.rng, fl[k] != 0u); }
        }
        if (cpuseed && !idx.empty()) {
            std::vector<bsgs_kangaroo_state> st;
            host_states(d, fl, st, sh);
            return bsgs_kangaroo_upload_list(dev, idx.data(), (uint32_t)idx.size(), st.data()) == BSGS_OK ? nullptr : "bsgs_kangaroo_upload_list";
        }
        uint32_t ninf = 0, first = 0;
        if (bsgs_kangaroo_seed(dev, qxy, idx.empty() ? nullptr : idx.data(), 0, (uint32_t)d.size(), (const uint8_t *)d.data(), fl.data(), &ninf, &first) != BSGS_OK) return "bsgs_kangaroo_seed";
        if (ninf) infinite_start(d[first], sh);
        return nullptr;
    }
    bool record(uint32_t e, const bsgs_kangaroo_record &r, Shared &sh) override
    {
        u128 d;
        memcpy(&d, r.d, 16);
        Scalar k;
        const uint32_t kid = dpt.sharded ? r.kangaroo : (uint32_t)(e * pro->pl.kn + r.kangaroo);      // -kdpshard: the device's ids are global already
        KangarooTable::Verdict v;
        const DevDpTable::Taken t = dpt.take(r);
        u128 ed;
        switch (t.kind) {
        case DevDpTable::STORED_HALF: case DevDpTable::ORPHAN: return true;
        case DevDpTable::PAIR: memcpy(&ed, t.stored->d, 16); v = table->add_pair(ed, t.stored->kangaroo, t.stored->flags, d, kid, r.flags, &k); break;
        default: v = table->add(r.x, d, kid, r.flags, &k);             // no -kdpdev, or what the device hands back alone: the host's own map
        }
        if (v == KangarooTable::FOUND) { key = k; found = true; sh.stop = true; return false; }
        if (v == KangarooTable::RESEED) {
            if (dpt.sharded) sh.push_reseed((uint32_t)(kid / pro->pl.kn), (uint32_t)(kid % pro->pl.kn));      // (an inbox record belongs to the engine it came from)
            else sh.push_reseed(e, r.kangaroo);
        }
        return true;
    }
    uint32_t entry_flags(uint32_t type) const override { return (type & 1u ? BSGS_KANGAROO_WILD : 0u) | (type & 2u ? BSGS_KANGAROO_NEG : 0u); }      // 0 tame, 1 wild, 3 wild with NEG
    bool done() const override { return found.load(); }
    bool give_up(uint64_t steps) override { return (double)steps > 20.0 * pro->pl.expected; }
    void status(double rate, uint64_t st, uint64_t dps) const override
    {
        printf("\r[%u] %.3e steps/s  steps 2^%.2f of expected 2^%.2f  DPs %llu  %.0fs   ", pro->pl.engines, rate, st ? std::log2((double)st) : 0.0, std::log2(pro->pl.expected),
               (unsigned long long)dps, pro->elapsed_before + since(pro->t0));
    }
    const WorkKeys *save(WorkHeader &h, std::vector<uint8_t> &entries) override
    {
        h.false_matches = table->false_matches(); h.reseeds = table->reseeds(); h.cycles = table->cycles();
        dpt.save(h, entries, table->size());                           // -kdpdev: the device's entries first
        table->write_entries(entries);
        return nullptr;
    }

    const KangConfig &c;
    const Affine P;
    const Prologue *pro = nullptr;
    Scalar base, key;
    Affine Q;
    uint8_t qxy[64];
    std::unique_ptr<JobList> jobs;
    JobList::Claim cl;
    std::unique_ptr<KangarooTable> table;
    std::atomic<bool> found{false};
    bool cpuseed = false;
    std::unique_ptr<Comb> comb;
    std::vector<std::vector<i128>> off0;
    DevDpTable dpt;                                // -kdpdev
};
}  // namespace

int kangaroo_main(int argc, char **argv)
{
    printf("BSGS MI355X kangaroo mode on %s\n", bsgs_version());
    const KangConfig c = parse_kangaroo_args(argc, argv);
    if (!c.ktamesgen.empty() || !c.ktames.empty()) return kangaroo_tames_main(c);
    if (!c.infile.empty()) return c.symlist ? kangaroo_symlist_main(c) : kangaroo_multi_main(c);
    Affine P;
    if (!hs::parse_pubkey(P, c.pub) || !hs::on_curve(P)) die("Invalid Public Key (-pb) length!!!");
    Prologue p(c);
    KeyMode mode(c, P);
    p.complete(c, mode);
    const Plan &pl = p.pl;
    printf("Expected steps: 2^%.2f (2 sqrt(W) + DP overhead), expected DPs 2^%.2f\n", std::log2(pl.expected), std::log2(2.0 * p.sqrtW / std::ldexp(1.0, (int)pl.dp) + 1.0));
    if (c.kdpshard) mode.dpt.shards(pl.engines, pl.kn, pl.cap);
    if (c.kdpdev || c.kdpshard) mode.dpt.banner(pl.cap);
    else if (c.dp < 0 && 2.0 * p.sqrtW / std::ldexp(1.0, (int)pl.dp) > 67108864.0) printf("WARNING: the expected DP count exceeds 2^26 host entries even at -dp 32\n");
    if (c.sym) printf("Kangaroo: symmetric walk (negation map), %u jump points, jump scale %g\n", p.wh.jumps, p.wh.jumpscale);
    Shared sh(p);
    mode.prepare(p, sh);
    const Outcome o = run(c, p, sh, mode);

    const KangarooTable &table = *mode.table;
    const double secs = p.elapsed_before + std::chrono::duration<double>(sh.ended - p.t0).count();      // (the last save is not job time here)
    std::string text, win;
    if (o == DONE) {
        std::string console;
        win = key_lines(mode.cl.listpos, mode.key, P, console);
        text = console;
    } else {
        char line[160];
        snprintf(line, sizeof line, "\nKangaroo: stopped after %llu steps (%s)\n", (unsigned long long)sh.steps.load(), o == BUDGET ? "-ksteps" : "signal");
        text = o == GAVE_UP ? "\nKangaroo: no key after 20 times the expected steps (is the key in the range?)\n" : o == ENDED ? "\nReached end of space\n" : line;
    }
    char tail[512];
    snprintf(tail, sizeof tail, "Job time %.2fs, %.3e kangaroo steps, %llu DPs (%zu in the table, %llu dropped), %llu false matches, %llu re-seeds\n", secs,
             (double)sh.steps.load(), (unsigned long long)sh.dps.load(), mode.table_size(), (unsigned long long)sh.dropped.load(), (unsigned long long)table.false_matches(),
             (unsigned long long)table.reseeds());
    text += tail;
    if (c.sym) text += "Symmetric walk: " + std::to_string(table.cycles()) + " cycles retired\n";
    for (uint32_t e = 0; e < pl.engines; e++)
        text += "Engine " + std::to_string(e) + " (GPU #" + std::to_string(p.gpus[e]) + "): " + std::to_string(sh.engine_records[e]) + " records" +
                (c.kdpshard ? ", " + std::to_string(sh.routed[e].load()) + " routed to other engines" : std::string()) + "\n";
    fputs(text.c_str(), stdout);                                       // one lane: the JobList leaves the console to the job (it appends win.txt)
    mode.jobs->finish(0, text, o == DONE, win);
    printf("Found %d of %zu\n", mode.jobs->found(), mode.jobs->size());
    fflush(stdout);
    return o == DONE ? 0 : (o == BUDGET || o == INTERRUPTED) ? 3 : 1;
}
