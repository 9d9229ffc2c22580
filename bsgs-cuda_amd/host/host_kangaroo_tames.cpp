// host_kangaroo_tames.cpp -- the tame half of the kangaroo search done once and kept (include/bsgs_hip.h "Kangaroo, tame table" states the rule;
// tests/kangaroo_tames_model.py restates it): the table file, the plan, and the two modes behind the driver's seam (host_kangaroo_run.h):
//   bsgs_mi355x -kangaroo -ktamesgen FILE -ktn T   an all-tame herd walks until the host's map holds T distinguished points, which are written sorted
//   bsgs_mi355x -kangaroo -ktames FILE             an all-wild herd, shared over the keys, walks with the file's jumps; each launch's records are matched
//                                                 against the table on the device (bsgs_kangaroo_run_tames) and only the matches come back
//   bsgs_mi355x -kangaroo -ktamesgen FILE -ktn T -ktamesdev   the same herd, the growing table in device memory (include/bsgs_hip.h "Kangaroo, tame table grown
//                                                 on the device"): each launch's records are inserted there (bsgs_kangaroo_run_tames_gen) and only merges, dead
//                                                 kangaroos and cycles come back; GenRule is what they mean, without a device (-selftest kangaroo-tames-gen)
//   ... -ktamesgen OUT -ktamesdev -ktamesfrom IN -ktn T   IN's entries are loaded into the growing table (bsgs_kangaroo_tames_gen_load) and a new herd walks with
//                                                 IN's walk until T entries are there; -ktnplan N plans a table's walk for the size it is meant to reach
//   bsgs_mi355x -kangaroo -ktamesmerge A,B -ktamesgen OUT   tables of one walk merged by tag on the host (tests/kangaroo_tames_extend_model.py restates both rules)
// Neither writes kangaroo.work.  TamesRule is the search rule without a device: -selftest kangaroo-tames-search drives it with scripted records.
// -ktamesgen -kwalk sym and -ktamessym FILE run the symmetric walk (include/bsgs_hip.h "Kangaroo, tame table for the symmetric walk"; tests/kangaroo_tames_sym_model.py): the
// file is version 2 (R, the jump scale and R scalars), offsets are counted from the middle of the range and are those of representatives, the search's herd is
// that of bsgs_kangaroo_setup_sym_keys and its records come back through bsgs_kangaroo_run_tames_keys, the entry numbers beside them.
#include "host_kangaroo_list.h"

#include <functional>
#include <iostream>
#include <queue>
#include <random>

namespace {
using namespace kang;

const char TAMES_MAGIC[9] = "KANGTAME";
const uint32_t TAMES_VERSION = 1, TAMES_VERSION_SYM = 2;      // 1: the plain walk's table; 2: the symmetric walk's (-kwalk sym): R and the jump scale, R scalars
const size_t TAMES_FIXED = 112, TAMES_FIXED_SYM = 128, TAMES_ENTRY = 24;

struct TamesFile {
    uint32_t version = TAMES_VERSION, dp = 0;
    Scalar lo, hi;
    uint64_t steps = 0, seed = 0, m = 0;
    uint32_t R = BSGS_KANGAROO_JUMPS;              // version 2: the jump points of the symmetric walk and the scale its mean jump was made with
    double jumpscale = 1.0;
    std::vector<uint64_t> js, x;                   // the R jump scalars; the entries' low 64 bits of x, strictly ascending
    std::vector<i128> d;                           // and their offsets (version 2: of the representative, signed)
    bool sym() const { return version == TAMES_VERSION_SYM; }
};

bool write_tames(const std::string &path, const TamesFile &f)
{
    const size_t head = (f.sym() ? TAMES_FIXED_SYM : TAMES_FIXED) + 8 * (size_t)f.R;
    std::vector<uint8_t> b(head + TAMES_ENTRY * f.x.size(), 0);
    const uint64_t T = f.x.size();
    memcpy(&b[0], TAMES_MAGIC, 8); memcpy(&b[8], &f.version, 4); memcpy(&b[12], &f.dp, 4);
    hs::fe_to_le(f.lo, &b[16]); hs::fe_to_le(f.hi, &b[48]);
    memcpy(&b[80], &T, 8); memcpy(&b[88], &f.steps, 8); memcpy(&b[96], &f.seed, 8); memcpy(&b[104], &f.m, 8);
    if (f.sym()) { memcpy(&b[112], &f.R, 4); memcpy(&b[120], &f.jumpscale, 8); }
    memcpy(&b[head - 8 * (size_t)f.R], f.js.data(), 8 * (size_t)f.R);
    for (uint64_t i = 0; i < T; i++) { memcpy(&b[head + TAMES_ENTRY * i], &f.x[i], 8); memcpy(&b[head + TAMES_ENTRY * i + 8], &f.d[i], 16); }
    const std::string tmp = path + ".temp";
    { std::ofstream o(tmp, std::ios::binary); o.write((const char *)b.data(), (std::streamsize)b.size()); if (!o) return false; }
    return rename(tmp.c_str(), path.c_str()) == 0;
}

// "" when the file is a complete tame table of version `want`, else what is wrong with it; the file is only read.  Each reader refuses the other's
// version with one line that says which walk the file belongs to.
std::string read_tames(const std::string &path, TamesFile &f, uint32_t want = TAMES_VERSION)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) return "cannot open " + path;
    std::vector<uint8_t> b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (b.size() < 8 || memcmp(b.data(), TAMES_MAGIC, 8) != 0) return path + " is not a tame table (magic)";
    uint32_t version = 0;
    if (b.size() >= 12) memcpy(&version, &b[8], 4);
    if (b.size() < 12 || version != want)
        return path + ": tame table version " + std::to_string(version) + ", this program reads version " + std::to_string(want) +
               (version == TAMES_VERSION_SYM && want == TAMES_VERSION ? " (version 2 is a table of the symmetric walk: -ktamessym)" :
                version == TAMES_VERSION && want == TAMES_VERSION_SYM ? " with -ktamessym (version 1 is a table of the plain walk: -ktames)" : "");
    f.version = version;
    const bool sym = f.sym();
    const std::string wrong_length = path + ": wrong length for a tame table (" + std::to_string(b.size()) + " bytes)";
    f.R = BSGS_KANGAROO_JUMPS; f.jumpscale = 1.0;
    if (sym) {
        if (b.size() < TAMES_FIXED_SYM) return wrong_length;
        memcpy(&f.R, &b[112], 4); memcpy(&f.jumpscale, &b[120], 8);
        if (f.R < 64 || f.R > BSGS_KANGAROO_SYM_MAX_JUMPS || (f.R & (f.R - 1))) return path + ": -kjumps " + std::to_string(f.R) + " (a power of two, 64..4096)";
    }
    const size_t head = (sym ? TAMES_FIXED_SYM : TAMES_FIXED) + 8 * (size_t)f.R;
    uint64_t T = 0;
    if (b.size() >= head) memcpy(&T, &b[80], 8);
    if (b.size() < head || !T || T > (1ull << 31) || b.size() != head + TAMES_ENTRY * T) return wrong_length;
    memcpy(&f.dp, &b[12], 4);
    if (f.dp > 32) return path + ": -dp " + std::to_string(f.dp);
    f.lo = hs::fe_from_le(&b[16]); f.hi = hs::fe_from_le(&b[48]);
    memcpy(&f.steps, &b[88], 8); memcpy(&f.seed, &b[96], 8); memcpy(&f.m, &b[104], 8);
    f.js.resize(f.R);
    memcpy(f.js.data(), &b[head - 8 * (size_t)f.R], 8 * (size_t)f.R);
    for (uint32_t j = 0; j < f.R; j++) if (!f.js[j]) return path + ": jump scalar " + std::to_string(j) + " is zero";
    f.x.resize(T); f.d.resize(T);
    for (uint64_t i = 0; i < T; i++) {
        memcpy(&f.x[i], &b[head + TAMES_ENTRY * i], 8); memcpy(&f.d[i], &b[head + TAMES_ENTRY * i + 8], 16);
        if (i && f.x[i] <= f.x[i - 1]) return path + ": entries are not strictly ascending (entry " + std::to_string(i) + ")";
    }
    return "";
}

// the planning defaults ("tame table"): K = T 2^dp trail points stand for the table; m = W / 2K keeps the tame trails from saturating the
// range; tame starts reach E = max(4 m W / K, W / 8) past the range; wild starts are spread over U = min(2^32, W / 4, E); a wild kangaroo older than A steps starts afresh
struct TamesPlan { uint64_t m, A; u128 E, U; double per_key; };
TamesPlan tames_plan(u128 W, uint64_t T, uint32_t dp)
{
    TamesPlan t;
    const long double K = (long double)T * std::ldexp(1.0L, (int)dp), w = (long double)W;
    const long double m = std::min(std::ldexp(1.0L, 62) - 1.0L, std::max(2.0L, w / (2.0L * K)));
    t.m = (uint64_t)m;
    t.E = std::max((u128)std::min(std::ldexp(1.0L, 126), std::max(1.0L, 4.0L * m * w / K)), W / 8);
    t.U = std::min(std::min<u128>((u128)1 << 32, std::max<u128>(W / 4, 1)), t.E);   // (within E: a wild start beyond the tame starts meets no trail)
    t.per_key = (double)(w / K);
    t.A = (uint64_t)std::min(std::ldexp(1.0L, 62), 8.0L * (w / K + std::ldexp(1.0L, (int)dp)));
    return t;
}

// the symmetric walk's defaults (tests/kangaroo_tames_sym_model.py plan): tame starts in [1, ceil(W/2) + E) with E = W / 16.  The walk on classes
// diffuses: after n steps a kangaroo is about m sqrt(n) from its start with n points within that distance, so it meets its own trail with probability about
// n^1.5 / m.  m is the largest that keeps the herd inside the covered region, m sqrt(n) = E / 2 with n = K / kn the steps of a generating kangaroo (kn: the
// generating herd, all engines), never below the plain table's W / 2K; wild starts are spread over [-U, U), U = min(2^32, E / 4); the age limit is the plain table's
uint64_t isqrt64(uint64_t v)
{
    uint64_t r = (uint64_t)std::sqrt((long double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}
TamesPlan tames_plan_sym(u128 W, uint64_t T, uint32_t dp, uint64_t kn)
{
    TamesPlan t = tames_plan(W, T, dp);
    const uint64_t K = T << dp, n = std::max<uint64_t>(1, K / std::max<uint64_t>(kn, 1));
    t.E = std::max<u128>(W / 16, 1);
    t.m = std::max<uint64_t>(t.m, (uint64_t)std::min<u128>(((u128)1 << 62) - 1, t.E / (2 * isqrt64(n))));
    t.U = std::max<u128>(1, std::min<u128>((u128)1 << 32, t.E / 4));
    t.per_key = (double)(((long double)(W / 2) + (long double)t.E) / (long double)K);
    return t;
}

std::string u128_hex(u128 v) { return hs::fe_to_hex(hs::sc_from_u128(v)); }

// ---- the search rule without a device -------------------------------------------------------------------------------------------------------------------
class TamesRule {
public:
    enum What { FOUND, FALSE_MATCH, STALE, RESEED };
    struct Event { What what; uint32_t a; Scalar key; };
    TamesRule(const TamesFile &f, u128 W, const std::vector<Affine> &P, const std::vector<bool> &presolved, uint64_t n_wild, uint64_t age_launches)
        : f_(f), W_(W), base_(f.sym() ? hs::sc_add(f.lo, hs::sc_from_u128(W / 2)) : f.lo), P_(P), known_(presolved), key_(P.size()),
          asg_((uint32_t)P.size(), presolved, n_wild), age_(n_wild, 0), limit_(age_launches)
    {
        for (size_t k = 0; k < P.size(); k++) { if (presolved[k]) { key_[k] = base_; solved_++; } same_[hs::compress_pubkey(P[k])].push_back((uint32_t)k); }
    }
    // what offsets are counted from: a, or with a table of the symmetric walk a + floor(W/2); a key equal to base*G is solved up front
    const Scalar &base() const { return base_; }
    uint64_t cycles() const { return cycles_; }
    // key k is base + off when off lies in the range as counted from base and that multiple of G is P_k: every equal point of the list is solved with it
    bool accept(uint32_t k, i128 off, std::vector<Event> &ev)
    {
        const i128 lowest = f_.sym() ? -(i128)(W_ / 2) : 0;
        if (off < lowest || off >= lowest + (i128)W_) return false;
        const Scalar cand = hs::sc_add(base_, sc_from_i128(off));
        const Affine q = hs::point_mul(hs::G, cand);
        if (q.inf || !hs::fe_equal(q.x, P_[k].x) || !hs::fe_equal(q.y, P_[k].y)) return false;
        for (uint32_t o : same_[hs::compress_pubkey(P_[k])]) if (!known_[o]) {
            known_[o] = true; key_[o] = cand; solved_++; asg_.solved(o);
            ev.push_back(Event{FOUND, o, cand});
        }
        return true;
    }
    bool known(uint32_t k) const { return known_[k]; }
    const Scalar &key(uint32_t k) const { return key_[k]; }
    uint32_t solved() const { return solved_; }
    uint32_t key_of(uint64_t w) const { return asg_.key(w); }
    const std::vector<uint32_t> &keys() const { return asg_.keys(); }
    uint64_t matches() const { return matches_; }
    uint64_t false_matches() const { return false_; }
    uint64_t reseeds() const { return reseeds_; }
    // one record the device handed back: flags and offset of the kangaroo, reserved = entry number + 1 or 0
    void record(uint32_t flags, uint32_t reserved, i128 d, std::vector<Event> &ev)
    {
        if (flags & BSGS_KANGAROO_DEAD) { reseeds_++; if (flags & BSGS_KANGAROO_CYCLE) cycles_++; ev.push_back(Event{RESEED, 0, Scalar()}); return; }
        if (!reserved || reserved > f_.x.size()) return;               // (the device hands back nothing else)
        matches_++;
        const uint32_t k = (flags >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu;
        if (k >= P_.size() || known_[k]) { ev.push_back(Event{STALE, k, Scalar()}); return; }
        const i128 dT = f_.d[reserved - 1];
        if (f_.sym()) {                                                // sigma Q_k + d_W G = eps d_T G: k'' = sigma (eps d_T - d_W), eps = +1 first
            const i128 sg = flags & BSGS_KANGAROO_NEG ? -1 : 1;
            if (accept(k, sg * (dT - d), ev) || accept(k, sg * (-dT - d), ev)) return;
        } else if (accept(k, dT - d, ev)) return;                      // k' = d_T - d_W
        false_++;
        ev.push_back(Event{FALSE_MATCH, k, Scalar()});
    }
    // a wild kangaroo of key k seeded with the offset u stands at infinity: Q_k = -u G, the candidate is -u (the symmetric walk's range holds such keys)
    void start_at_infinity(uint32_t k, i128 u, std::vector<Event> &ev) { if (k < P_.size() && !known_[k]) accept(k, -u, ev); }
    // a launch of wild kangaroos [first, first + n) ended: those that have walked more than the limit since their start are named
    void launch_done(uint64_t first, uint64_t n, std::vector<uint64_t> &aged)
    {
        for (uint64_t w = first; w < first + n; w++) if (++age_[w] > limit_) { aged.push_back(w); reseeds_++; }
    }
    // wild kangaroo w starts afresh: its key from now on (false: no key is open, it rests)
    bool reseed(uint64_t w, uint32_t *k) { age_[w] = 0; return asg_.reseed(w, *this, k); }
private:
    const TamesFile &f_;
    const u128 W_;
    const Scalar base_;
    const std::vector<Affine> &P_;
    std::vector<bool> known_;
    std::vector<Scalar> key_;
    Assigner asg_;
    std::vector<uint32_t> age_;
    const uint64_t limit_;
    std::map<std::string, std::vector<uint32_t>> same_;
    uint64_t matches_ = 0, false_ = 0, reseeds_ = 0, cycles_ = 0;
    uint32_t solved_ = 0;
};

u128 range_width(const Scalar &lo, const Scalar &hi)
{
    const Scalar wm1 = hs::sc_sub(hi, lo);
    return (((u128)wm1.l[1] << 64) | wm1.l[0]) + 1;
}

// ---- -ktamesgen -ktamesdev: what a handed-back record means, without a device ----------------------------------------------------------------------------
class GenRule {
public:
    enum What { RESEED, MERGE, HELD, DROPPED, IGNORED };
    explicit GenRule(uint64_t T) : T_(T) {}
    void entries(uint64_t n) { dev_ = n; }                            // entries in the device's table after a launch
    void hold(uint64_t x, i128 d) { held_.emplace(x, d); }            // -ktamesfrom: the loaded table's entry with the tag the device cannot hold
    uint64_t total() const { return dev_ + held_.size(); }
    bool done() const { return total() >= T_; }
    // one record the device handed back, `reason` its reserved word (BSGS_KANGAROO_GEN_*): a dead kangaroo starts afresh; a duplicate has merged into a
    // known trail and starts afresh; the one tag the device cannot hold is kept here, where a second one is a merge; FULL is counted (the sizing makes
    // it unreachable).  Once the table is done nothing is looked at
    What record(uint32_t reason, uint64_t x, i128 d)
    {
        if (done()) return IGNORED;
        switch (reason) {
            case BSGS_KANGAROO_GEN_DEAD: reseeds_++; return RESEED;
            case BSGS_KANGAROO_GEN_DUPLICATE: merges_++; reseeds_++; return MERGE;
            case BSGS_KANGAROO_GEN_TAG_ZERO:
                if (!held_.emplace(x, d).second) { merges_++; reseeds_++; return MERGE; }
                return HELD;
            default: dropped_++; return DROPPED;
        }
    }
    const std::map<uint64_t, i128> &held() const { return held_; }
    uint64_t merges() const { return merges_; }
    uint64_t reseeds() const { return reseeds_; }
    uint64_t dropped() const { return dropped_; }
private:
    const uint64_t T_;
    uint64_t dev_ = 0, merges_ = 0, reseeds_ = 0, dropped_ = 0;
    std::map<uint64_t, i128> held_;
};

// T entries (tag x, offset d) of a tame table against d*G on an open device that has a herd (bsgs_kangaroo_verify_points, tame flags), 2^20 at a time:
// *bad = the first entry that does not match its offset, T when every one does.  The code of the call that failed, else BSGS_OK
int verify_tame_entries(bsgs_dev *dev, const uint64_t *x, const i128 *d, uint64_t T, uint64_t *bad)
{
    uint8_t g[64];
    hs::affine_to_le(hs::G, g, g + 32);
    const uint64_t step = 1u << 20;
    std::vector<uint32_t> fl((size_t)std::min(T, step), 0u);
    *bad = T;
    for (uint64_t pos = 0; pos < T; pos += step) {
        uint32_t n_bad = 0, first = 0;
        const int rc = bsgs_kangaroo_verify_points(dev, g, (uint32_t)std::min(T - pos, step), (const uint8_t *)&d[pos], fl.data(), &x[pos], &n_bad, &first, 1);
        if (rc != BSGS_OK) return rc;
        if (n_bad) { *bad = pos + first; break; }
    }
    return BSGS_OK;
}

// ---- -ktamesgen ---------------------------------------------------------------------------------------------------------------------------------------
struct GenMode : Mode {
    GenMode(const KangConfig &c, const Prologue &p, TamesFile *from = nullptr) : c(c), T(c.ktn), Tplan(c.ktnplan ? c.ktnplan : c.ktn), from(from), rule(c.ktn)
    {
        saves = false;
        // dp: the command line's, else about (log2(W / T)) / 2 - 4: the trails stay a small part of the range while a wild walk to the next DP stays short
        // (-ktnplan: T is the size the table is meant to reach; -ktamesfrom: the walk is the loaded table's, the plan only says where tame kangaroos start)
        dp_fixed = from ? (int)from->dp : c.dp >= 0 ? c.dp : (int)std::max(0.0, std::min(14.0, std::floor(std::log2((double)p.W / (double)Tplan) / 2.0) - 4.0));
        plan = tames_plan(p.W, Tplan, (uint32_t)dp_fixed);             // (-kwalk sym: planned() replaces it once the herd is known)
        if (from) { plan.m = from->m; jump_scalars = from->js.data(); }
        mean_jump = (double)plan.m;
        expected = 2.0 * (double)T * std::ldexp(1.0, dp_fixed);
        herd_label = "herd (GPU, all tame), engine ";
        span = p.W + plan.E - 1;
        if (c.tames_sym) {                                             // -kwalk sym: R jump points, a launch longer than the cycle window
            jumps = from ? from->R : c.jumps ? c.jumps : 1024u;
            jumpscale = from ? from->jumpscale : c.jumpscale != 0.0 ? c.jumpscale : 1.0;
            min_launch = 2.0 * BSGS_KANGAROO_CYCLE_WINDOW;
        }
        if (!c.ktamesdev) map.reserve((size_t)T * 2);
    }
    // -kwalk sym: the mean jump depends on the steps a kangaroo of this herd walks; mean -kjumpscale * m, starts in [1, ceil(W/2) + E)
    void planned(const Prologue &p) override
    {
        if (!c.tames_sym) return;
        plan = tames_plan_sym(p.W, Tplan, p.pl.dp, p.pl.kn * p.pl.engines);
        mean_jump = from ? (double)from->m : std::max(1.0, std::min(std::ldexp(1.0, 62), jumpscale * (double)plan.m));
        span = (p.W + 1) / 2 + plan.E - 1;
    }
    std::string fingerprint(const Prologue &, const WorkHeader &) const override { return ""; }
    bool before_devices(Prologue &p) override { pro = &p; p.t0 = Clock::now(); return true; }
    const char *setup(bsgs_dev *dev) override
    {
        const Plan &pl = pro->pl;
        if (c.tames_sym) { if (bsgs_kangaroo_setup_sym(dev, pro->jxy.data(), pro->js.data(), jumps, pl.dp, (uint32_t)pl.kn, pl.G, pl.cap) != BSGS_OK) return "bsgs_kangaroo_setup_sym"; }
        else if (bsgs_kangaroo_setup(dev, pro->jxy.data(), pro->js.data(), pl.dp, (uint32_t)pl.kn, pl.G, pl.cap) != BSGS_OK) return "bsgs_kangaroo_setup";
        if (c.ktamesdev && bsgs_kangaroo_tames_gen_begin(dev, T) != BSGS_OK) return "bsgs_kangaroo_tames_gen_begin";
        return from ? load(dev) : nullptr;
    }
    // -ktamesfrom: the table begins with the capacity of the final table and takes the file's entries in, 24 bytes each; the one tag the device cannot hold
    // (it can only be the first entry) is kept here, as a record with that tag is
    const char *load(bsgs_dev *dev)
    {
        const auto ts = Clock::now();
        const size_t skip = !from->x.empty() && from->x[0] == 0 ? 1 : 0;
        uint64_t stored = 0, dup = 0, zero = 0, full = 0, n_entries = 0;
        if (bsgs_kangaroo_tames_gen_load(dev, from->x.data() + skip, (const uint8_t *)(from->d.data() + skip), from->x.size() - skip, &stored, &dup, &zero, &full, &n_entries) != BSGS_OK)
            return "bsgs_kangaroo_tames_gen_load";
        if (skip) rule.hold(0, from->d[0]);
        rule.entries(n_entries);
        loaded = stored + skip;
        printf("Loaded %llu entries of the table into GPU memory, %llu duplicates%s, %.3fs\n", (unsigned long long)loaded, (unsigned long long)dup,
               full || zero ? " (entries were lost: the file is not a sound table)" : "", since(ts));
        std::vector<uint64_t>().swap(from->x);
        std::vector<i128>().swap(from->d);
        return full || zero ? "bsgs_kangaroo_tames_gen_load (the table did not take every entry)" : nullptr;
    }
    // every kangaroo is tame: t uniform in [1, W + E), with -kwalk sym in [1, ceil(W/2) + E), d = t
    const char *seed(bsgs_dev *dev, uint32_t e, const std::vector<uint32_t> &idx, Shared &sh) override
    {
        const size_t n = idx.empty() ? (size_t)pro->pl.kn : idx.size();
        std::vector<i128> d(n);
        std::vector<uint32_t> fl(n, 0u);
        { std::lock_guard<std::mutex> lk(sh.rng_m); for (size_t k = 0; k < n; k++) d[k] = (i128)(1 + draw128(sh.rng) % span); }
        uint32_t ninf = 0, first = 0;
        if (bsgs_kangaroo_seed(dev, nullptr, idx.empty() ? nullptr : idx.data(), 0, (uint32_t)n, (const uint8_t *)d.data(), fl.data(), &ninf, &first) != BSGS_OK) return "bsgs_kangaroo_seed";
        if (ninf) sh.push_reseed(e, idx.empty() ? first : idx[first]);
        return nullptr;
    }
    // -ktamesdev: the launch, the insert on the device, the handed-back records alone; the entry count decides when the table is done
    int launch(bsgs_dev *dev, uint32_t e, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t cap, uint32_t *n, uint64_t *dropped, Shared &sh) override
    {
        if (!c.ktamesdev) return Mode::launch(dev, e, steps, recs, cap, n, dropped, sh);
        uint64_t n_seen = 0, n_entries = 0;
        const int rc = bsgs_kangaroo_run_tames_gen(dev, steps, recs, cap, n, &n_seen, &n_entries, dropped, nullptr);
        if (rc != BSGS_OK) return rc;
        seen += n_seen;
        std::lock_guard<std::mutex> lt(sh.tab_m);
        rule.entries(n_entries);
        if (rule.done()) sh.stop = true;
        return rc;
    }
    // -ktamesdev, in the engine's thread before its device is closed: the finished table leaves the device sorted and cut to the T lowest tags
    // (bsgs_kangaroo_tames_gen_read_sorted), the host's entries go in front, and every entry that will be written is checked against d*G on this engine
    std::string ending(bsgs_dev *dev, uint32_t, Shared &sh) override
    {
        if (!c.ktamesdev) return "";
        std::lock_guard<std::mutex> lt(sh.tab_m);
        if (!rule.done()) return "";
        walked = since(pro->t0);
        // the device sorts and cuts: the host's entries have the tag 0 and sort first, so the T - (held) lowest tags of the device complete the table
        const auto tr = Clock::now();
        const uint64_t held = std::min<uint64_t>(T, rule.held().size()), want = T - held;
        uint64_t n = 0, h = 0;
        tx.resize((size_t)T); td.resize((size_t)T);                    // the file's two columns, filled in place
        for (const auto &kv : rule.held()) if (h < held) { tx[h] = kv.first; td[h] = kv.second; h++; }
        const int rc = bsgs_kangaroo_tames_gen_read_sorted(dev, tx.data() + held, (uint8_t *)(td.data() + held), want, &n);
        if (rc != BSGS_OK || n < want) {
            tx.clear(); td.clear();
            return rc != BSGS_OK ? std::string("bsgs_kangaroo_tames_gen_read_sorted: ") + bsgs_last_error() :
                                   "growing tame table: " + std::to_string(n + held) + " entries read, " + std::to_string(T) + " counted";
        }
        (void)bsgs_kangaroo_tames_gen_end(dev);
        read_secs = since(tr);
        if (!c.verify) return "";
        const auto ts = Clock::now();
        uint64_t bad = 0;
        if (verify_tame_entries(dev, tx.data(), td.data(), T, &bad) != BSGS_OK) return std::string("bsgs_kangaroo_verify_points: ") + bsgs_last_error();
        if (bad < T) { tx.clear(); td.clear(); return "Tame table is damaged: entry " + std::to_string(bad) + " does not match its offset"; }
        printf("\n[verify] tame table: %llu entries %.3fs\n", (unsigned long long)T, since(ts));
        return "";
    }
    bool record_dev(uint32_t e, const bsgs_kangaroo_record &r, Shared &sh)
    {
        uint64_t x; i128 d;
        memcpy(&x, r.x, 8); memcpy(&d, r.d, 16);
        handed_back++;
        switch (rule.record(r.reserved, x, d)) {
            case GenRule::IGNORED: return false;
            case GenRule::RESEED: case GenRule::MERGE: sh.push_reseed(e, r.kangaroo); break;
            case GenRule::HELD: if (rule.done()) { sh.stop = true; return false; } break;
            case GenRule::DROPPED: sh.dropped++; break;
        }
        return true;
    }
    bool record(uint32_t e, const bsgs_kangaroo_record &r, Shared &sh) override
    {
        if (c.ktamesdev) return record_dev(e, r, sh);
        if (map.size() >= T) return false;
        if (r.flags & BSGS_KANGAROO_DEAD) { sh.push_reseed(e, r.kangaroo); return true; }
        uint64_t x; i128 d;
        memcpy(&x, r.x, 8); memcpy(&d, r.d, 16);
        if (!map.emplace(x, d).second) { merges++; sh.push_reseed(e, r.kangaroo); return true; }     // it has merged into a known trail
        if (map.size() >= T) { sh.stop = true; return false; }
        return true;
    }
    uint32_t entry_flags(uint32_t) const override { return 0u; }
    size_t size() const { return c.ktamesdev ? (size_t)rule.total() : map.size(); }
    uint64_t n_merges() const { return c.ktamesdev ? rule.merges() : merges; }
    bool done() const override { return size() >= T; }
    bool give_up(uint64_t steps) override { return (double)steps > 50.0 * pro->pl.expected; }
    void status(double rate, uint64_t st, uint64_t dps) const override
    {
        if (c.ktamesdev) {
            printf("\r[%u] %.3e steps/s  steps 2^%.2f  entries %zu of %llu  DPs %llu  handed back %llu  merges %llu  %.0fs   ", pro->pl.engines, rate, st ? std::log2((double)st) : 0.0, size(),
                   (unsigned long long)T, (unsigned long long)seen.load(), (unsigned long long)handed_back, (unsigned long long)rule.merges(), since(pro->t0));
            return;
        }
        printf("\r[%u] %.3e steps/s  steps 2^%.2f  entries %zu of %llu  DPs %llu  merges %llu  %.0fs   ", pro->pl.engines, rate, st ? std::log2((double)st) : 0.0, map.size(),
               (unsigned long long)T, (unsigned long long)dps, (unsigned long long)merges, since(pro->t0));
    }
    const WorkKeys *save(WorkHeader &, std::vector<uint8_t> &) override { return nullptr; }

    const KangConfig &c;
    const uint64_t T, Tplan;                                           // the entries to make; the entries the walk is planned for (-ktnplan)
    TamesFile *const from;                                             // -ktamesfrom: the table that is extended (its entries until they are loaded)
    uint64_t loaded = 0;
    const Prologue *pro = nullptr;
    TamesPlan plan;
    u128 span;
    std::unordered_map<uint64_t, i128> map;
    uint64_t merges = 0;
    // -ktamesdev: the rule of the handed-back records (under sh.tab_m), the records the walk produced, the records that crossed the bus, and the
    // finished table: the T lowest tags, sorted (ending())
    GenRule rule;
    std::atomic<uint64_t> seen{0};
    uint64_t handed_back = 0;
    std::vector<uint64_t> tx;
    std::vector<i128> td;
    double walked = 0.0, read_secs = 0.0;                              // seconds from the start to the launch that completed the table; of the sorted read
};

void tames_verify(const TamesFile &f, int gpu);

std::string find_tames(const KangConfig &c, std::string path)
{
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0 && stat((c.dir + "/" + path).c_str(), &sb) == 0) path = c.dir + "/" + path;
    return path;
}

int tames_generate(const KangConfig &c_in)
{
    KangConfig c = c_in;
    // -ktamesfrom: the table is read and every refusal is made before any device is looked for; the walk is the file's, and what the command line names of it
    // must be what the file says
    TamesFile in;
    const bool extend = !c.ktamesfrom.empty();
    if (extend) {
        const std::string bad = read_tames(find_tames(c, c.ktamesfrom), in, c.tames_sym ? TAMES_VERSION_SYM : TAMES_VERSION);
        if (!bad.empty()) die("-ktamesfrom: " + bad);
        if (c.ktn <= in.x.size()) die("-ktamesfrom: -ktn " + std::to_string(c.ktn) + " must be above the " + std::to_string(in.x.size()) + " entries of the table that is extended");
        if (c.seed_given && c.seed == in.seed) die("-ktamesfrom: -kseed is the seed the table was made with (the new herd would retrace its starts): give another");
        if (c.dp >= 0 && (uint32_t)c.dp != in.dp) die("-ktamesfrom: -dp " + std::to_string(c.dp) + " differs from the table's -dp " + std::to_string(in.dp));
        if (c.jumps && c.jumps != in.R) die("-ktamesfrom: -kjumps " + std::to_string(c.jumps) + " differs from the table's " + std::to_string(in.R));
        if (c.jumpscale != 0.0 && c.jumpscale != in.jumpscale) die("-ktamesfrom: -kjumpscale differs from the table's");
        if (!c.range_given) { c.pk = hs::fe_to_hex(in.lo); c.pke = hs::fe_to_hex(in.hi); }
    }
    Prologue p(c);
    if (extend && (hs::fe_cmp(p.lo, in.lo) != 0 || hs::fe_cmp(p.hi, in.hi) != 0)) die("-ktamesfrom: Tame table was made for another range");
    if (extend && !c.seed_given) {                                     // no -kseed: drawn here, so that it is not the file's by chance
        std::random_device rd;
        do c.seed = ((uint64_t)rd() << 32) ^ rd(); while (c.seed == in.seed);
        c.seed_given = true;
    }
    printf("Kangaroo range [%s, %s], width 2^%.2f: a tame table of %llu entries\n", hs::fe_to_hex(p.lo).c_str(), hs::fe_to_hex(p.hi).c_str(), std::log2((double)p.W),
           (unsigned long long)c.ktn);
    if (extend) printf("Extending a table of %zu entries made with %.3e steps: its walk is taken over\n", in.x.size(), (double)in.steps);
    const uint64_t in_steps = in.steps, in_T = in.x.size();
    GenMode mode(c, p, extend ? &in : nullptr);
    p.complete(c, mode);
    if (extend && c.verify) tames_verify(in, p.gpus[0]);
    if (c.tames_sym) printf("Plan: symmetric walk, %u jump points, jump scale %g, mean jump m = %llu, tame starts reach E = 0x%s past the half range, -dp %u\n", mode.jumps, mode.jumpscale,
                            (unsigned long long)mode.mean_jump, u128_hex(mode.plan.E).c_str(), p.pl.dp);
    else printf("Plan: mean jump m = %llu, tame starts reach E = 0x%s past the range, -dp %u\n", (unsigned long long)mode.plan.m, u128_hex(mode.plan.E).c_str(), p.pl.dp);
    Shared sh(p);
    const Outcome o = run(c, p, sh, mode);
    const double secs = since(p.t0);
    if (o != DONE) {
        printf("\nKangaroo: tame table not finished after %llu steps (%s), %zu of %llu entries; nothing written\n", (unsigned long long)sh.steps.load(),
               o == GAVE_UP ? "the trails have saturated the range: a smaller -ktn or -dp" : o == BUDGET ? "-ksteps" : "signal", mode.size(), (unsigned long long)c.ktn);
        return o == GAVE_UP ? 1 : 3;
    }
    TamesFile f;
    f.dp = p.pl.dp; f.lo = p.lo; f.hi = p.hi; f.steps = in_steps + sh.steps.load(); f.seed = p.wh.seed; f.m = mode.plan.m; f.js = p.js;
    if (c.tames_sym) { f.version = TAMES_VERSION_SYM; f.R = mode.jumps; f.jumpscale = mode.jumpscale; f.m = extend ? in.m : (uint64_t)mode.mean_jump; }
    if (c.ktamesdev) { f.x.swap(mode.tx); f.d.swap(mode.td); }         // read sorted and cut, completed and verified in the engine's thread (GenMode::ending)
    else {
        std::vector<std::pair<uint64_t, i128>> en(mode.map.begin(), mode.map.end());
        std::sort(en.begin(), en.end());
        en.resize((size_t)c.ktn);
        for (const auto &kv : en) { f.x.push_back(kv.first); f.d.push_back(kv.second); }
    }
    if (f.x.size() != c.ktn || f.d.size() != c.ktn) die("tame table: " + std::to_string(f.x.size()) + " entries of " + std::to_string(c.ktn));
    std::string path = c.ktamesgen;
    if (path.find('/') == std::string::npos) path = c.dir + "/" + path;
    if (!write_tames(path, f)) die("cannot write " + path);
    printf("\nTame table %s: %llu entries, %.3e steps, %llu DPs, %llu merges, %.2fs\n", path.c_str(), (unsigned long long)c.ktn, (double)f.steps,
           (unsigned long long)(c.ktamesdev ? mode.seen.load() : sh.dps.load()), (unsigned long long)mode.n_merges(), secs);
    if (c.ktamesdev) printf("Table grown on the GPU: %llu records inserted there, %llu handed back over the bus (%llu dropped), %.2fs of walking\n", (unsigned long long)mode.seen.load(),
                            (unsigned long long)mode.handed_back, (unsigned long long)sh.dropped.load(), mode.walked);
    if (c.ktamesdev) printf("Table sorted and cut on the GPU: %.3fs for the sorted read, %.2fs from the last launch to the file\n", mode.read_secs, since(p.t0) - mode.walked);
    if (extend) printf("Extended from %llu to %llu entries: %llu loaded, %.3e steps of this run, %.3e in all\n", (unsigned long long)in_T, (unsigned long long)c.ktn,
                       (unsigned long long)mode.loaded, (double)sh.steps.load(), (double)f.steps);
    fflush(stdout);
    return 0;
}

// ---- -ktames --------------------------------------------------------------------------------------------------------------------------------------------
struct SearchMode : Mode {
    SearchMode(const KangConfig &c, const std::vector<Affine> &P, const TamesFile &f, const Prologue &p) : c(c), P(P), L((uint32_t)P.size()), f(f)
    {
        saves = false;
        dp_fixed = (int)f.dp;
        mean_jump = (double)f.m;
        jump_scalars = f.js.data();                                    // the search walks with exactly the generator's jumps
        plan = f.sym() ? tames_plan_sym(p.W, f.x.size(), f.dp, 1) : tames_plan(p.W, f.x.size(), f.dp);      // (E, U, A: they do not depend on the herd; m is the file's)
        if (f.sym()) { jumps = f.R; jumpscale = f.jumpscale; min_launch = 2.0 * BSGS_KANGAROO_CYCLE_WINDOW; }      // a launch longer than the cycle window
        herd_label = "herd (GPU, all wild), engine ";
    }
    std::string fingerprint(const Prologue &, const WorkHeader &) const override { return ""; }
    void report(uint32_t k, const Scalar &key) { report_key(c.dir, (int)k + 1, key, P[k]); found_n++; }
    bool before_devices(Prologue &p) override
    {
        pro = &p;
        { Config rc; rc.dir = c.dir; read_recovery(rc); }             // (win.txt starts empty, as on the BSGS path)
        p.t0 = Clock::now();
        base = f.sym() ? hs::sc_add(p.lo, hs::sc_from_u128(p.W / 2)) : p.lo;      // -kwalk sym: offsets are counted from the middle of the range
        const Affine naG = hs::affine_neg(hs::point_mul(hs::G, base));
        presolved.assign(L, false);
        qxy.resize(64 * (size_t)L);
        for (uint32_t k = 0; k < L; k++) {                             // Q_k = P_k - a*G; a key equal to a*G is solved here and keeps its slot
            Affine Q = hs::point_add(P[k], naG);
            if (Q.inf) { presolved[k] = true; report(k, base); Q = hs::G; }
            hs::affine_to_le(Q, &qxy[64 * (size_t)k], &qxy[64 * (size_t)k + 32]);
        }
        open0 = L - (uint32_t)found_n;
        expected = (double)open0 * plan.per_key;
        if (!open0) printf("Found %d of %u\n", found_n, L);
        return open0 != 0;
    }
    void prepare(Prologue &p, Shared &s)
    {
        const Plan &pl = p.pl;
        // (the give-up bound's allowance per kangaroo: the way to the next DP, and W / K steps before it meets a trail at all -- the trails of a small
        // generating herd leave gaps that long)
        overhead = (double)pl.kn * pl.engines * (plan.per_key + std::ldexp(1.0, (int)pl.dp));
        const uint64_t launches = std::max<uint64_t>(1, (plan.A + pl.S - 1) / pl.S);
        rule.reset(new TamesRule(f, p.W, P, presolved, pl.kn * pl.engines, launches));
        printf("Tame table: %zu entries at -dp %u, mean jump %llu; about 2^%.2f steps per key; a wild kangaroo starts afresh after %llu launches\n", f.x.size(), f.dp,
               (unsigned long long)f.m, std::log2(plan.per_key + std::ldexp(1.0, (int)f.dp)), (unsigned long long)launches);
        off0.resize(pl.engines);
        for (uint32_t e = 0; e < pl.engines; e++) { off0[e].resize(pl.kn); for (uint64_t i = 0; i < pl.kn; i++) off0[e][i] = wild_offset(s.rng); }
        if (f.sym()) entries.assign(pl.engines, std::vector<uint32_t>(pl.cap));
        last_solved = rule->solved();
    }
    // u uniform in [0, U); with a table of the symmetric walk in [-U, U)
    i128 wild_offset(uint64_t &rng) const { return f.sym() ? (i128)(draw128(rng) % (2 * plan.U)) - (i128)plan.U : (i128)(draw128(rng) % plan.U); }
    const char *setup(bsgs_dev *dev) override
    {
        const Plan &pl = pro->pl;
        if (f.sym()) {                                                 // the symmetric herd whose records name their key beside the flags
            if (bsgs_kangaroo_setup_sym_keys(dev, pro->jxy.data(), pro->js.data(), jumps, pl.dp, (uint32_t)pl.kn, pl.G, pl.cap) != BSGS_OK) return "bsgs_kangaroo_setup_sym_keys";
            if (bsgs_kangaroo_set_keys(dev, qxy.data(), L) != BSGS_OK) return "bsgs_kangaroo_set_keys";
            return bsgs_kangaroo_tames_install_keys(dev, f.x.data(), f.x.size()) == BSGS_OK ? nullptr : "bsgs_kangaroo_tames_install_keys";
        }
        if (bsgs_kangaroo_setup(dev, pro->jxy.data(), pro->js.data(), pl.dp, (uint32_t)pl.kn, pl.G, pl.cap) != BSGS_OK) return "bsgs_kangaroo_setup";
        if (bsgs_kangaroo_set_keys(dev, qxy.data(), L) != BSGS_OK) return "bsgs_kangaroo_set_keys";
        return bsgs_kangaroo_tames_install(dev, f.x.data(), f.x.size()) == BSGS_OK ? nullptr : "bsgs_kangaroo_tames_install";
    }
    // every kangaroo is wild: kangaroo of key k at Q_k + u*G, u uniform in [0, U), flags WILD | k << 8 (the symmetric herd: the key beside the flags)
    const char *seed(bsgs_dev *dev, uint32_t e, const std::vector<uint32_t> &idx, Shared &s) override
    {
        const uint64_t kn = pro->pl.kn, w0 = (uint64_t)e * kn;
        std::vector<uint32_t> use, fl, key;
        std::vector<i128> d;
        if (idx.empty()) {
            fl.assign(kn, BSGS_KANGAROO_WILD); key.resize(kn);
            for (uint64_t i = 0; i < kn; i++) key[i] = rule->key_of(w0 + i);
            d.swap(off0[e]);
        } else {
            std::lock_guard<std::mutex> lt(s.tab_m);
            std::lock_guard<std::mutex> lk(s.rng_m);
            for (uint32_t i : idx) {
                uint32_t k = 0;
                if (!rule->reseed(w0 + i, &k)) continue;               // no key is open: the kangaroo rests
                use.push_back(i); fl.push_back(BSGS_KANGAROO_WILD); key.push_back(k);
                d.push_back(wild_offset(s.rng));
            }
            if (use.empty()) return nullptr;
        }
        uint32_t ninf = 0, first = 0;
        if (bsgs_kangaroo_seed_keys(dev, use.empty() ? nullptr : use.data(), 0, (uint32_t)d.size(), (const uint8_t *)d.data(), fl.data(), key.data(), &ninf, &first) != BSGS_OK)
            return "bsgs_kangaroo_seed_keys";
        if (ninf) {
            // Q_k + u*G at infinity names the key base - u: below the plain walk's range, but maybe in the symmetric walk's.  Either way the kangaroo starts again
            if (f.sym()) {
                std::lock_guard<std::mutex> lt(s.tab_m);
                std::vector<TamesRule::Event> ev;
                rule->start_at_infinity(key[first], d[first], ev);
                found_events(ev, s);
            }
            s.push_reseed(e, use.empty() ? first : use[first]);
        }
        return nullptr;
    }
    // under s.tab_m: the keys an event list names as found go to win.txt, and their kangaroos start afresh
    void found_events(const std::vector<TamesRule::Event> &ev, Shared &s)
    {
        const uint64_t kn = pro->pl.kn;
        for (const TamesRule::Event &x : ev) {
            if (x.what != TamesRule::FOUND) continue;
            report(x.a, x.key);
            for (uint64_t w = 0; w < rule->keys().size(); w++) if (rule->keys()[w] == x.a) s.push_reseed((uint32_t)(w / kn), (uint32_t)(w % kn));
        }
        if (rule->solved() == L) s.stop = true;
    }
    // the launch, the match on the device, the matched and DEAD records alone; then the kangaroos that have walked too long
    int launch(bsgs_dev *dev, uint32_t e, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t cap, uint32_t *n, uint64_t *dropped, Shared &s) override
    {
        uint64_t n_seen = 0;
        int rc;
        if (f.sym()) {
            // the records as the walk wrote them, the entry numbers beside them: brought into the form of the plain herd's -- the key into the flags'
            // key bits (where the walk keeps its last jump index, which means nothing here), entry number + 1 into `reserved`
            rc = bsgs_kangaroo_run_tames_keys(dev, steps, recs, entries[e].data(), std::min<uint32_t>(cap, (uint32_t)entries[e].size()), n, &n_seen, dropped, nullptr);
            if (rc == BSGS_OK) for (uint32_t i = 0; i < *n; i++) {
                const uint32_t type = recs[i].flags & (BSGS_KANGAROO_WILD | BSGS_KANGAROO_NEG | BSGS_KANGAROO_CYCLE | BSGS_KANGAROO_DEAD);
                recs[i].flags = type | (recs[i].reserved & 0xFFFFu) << BSGS_KANGAROO_KEY_SHIFT;
                recs[i].reserved = entries[e][i];
            }
        } else rc = bsgs_kangaroo_run_tames(dev, steps, recs, cap, n, &n_seen, dropped, nullptr);
        if (rc != BSGS_OK) return rc;
        seen += n_seen;
        std::vector<uint64_t> aged;
        const uint64_t kn = pro->pl.kn;
        { std::lock_guard<std::mutex> lt(s.tab_m); rule->launch_done((uint64_t)e * kn, kn, aged); }
        for (uint64_t w : aged) s.push_reseed(e, (uint32_t)(w - (uint64_t)e * kn));
        return rc;
    }
    bool record(uint32_t e, const bsgs_kangaroo_record &r, Shared &s) override
    {
        std::vector<TamesRule::Event> ev;
        i128 d;
        memcpy(&d, r.d, 16);
        rule->record(r.flags, r.reserved, d, ev);
        for (const TamesRule::Event &x : ev) if (x.what == TamesRule::RESEED) s.push_reseed(e, r.kangaroo);
        found_events(ev, s);
        return true;
    }
    uint32_t entry_flags(uint32_t) const override { return 0u; }
    bool done() const override { return rule && rule->solved() == L; }
    bool give_up(uint64_t steps) override
    {
        const uint32_t now = rule->solved();
        if (now != last_solved) { last_solved = now; steps_mark = steps; }
        return (double)(steps - steps_mark) > 20.0 * ((double)(L - now) * plan.per_key + overhead);
    }
    void status(double rate, uint64_t st, uint64_t) const override
    {
        printf("\r[%u] %.3e steps/s  steps 2^%.2f  solved %u/%u  records seen %llu  matches %llu  %.0fs   ", pro->pl.engines, rate, st ? std::log2((double)st) : 0.0, rule->solved(), L,
               (unsigned long long)seen.load(), (unsigned long long)rule->matches(), since(pro->t0));
    }
    const WorkKeys *save(WorkHeader &, std::vector<uint8_t> &) override { return nullptr; }

    const KangConfig &c;
    const std::vector<Affine> &P;
    const uint32_t L;
    const TamesFile &f;
    const Prologue *pro = nullptr;
    TamesPlan plan;
    std::unique_ptr<TamesRule> rule;
    std::vector<bool> presolved;
    std::vector<uint8_t> qxy;
    std::vector<std::vector<i128>> off0;
    Scalar base;                                                       // what offsets are counted from: a, or a + floor(W/2) with a table of the symmetric walk
    std::vector<std::vector<uint32_t>> entries;                        // per engine, the symmetric herd: entry number + 1 of each record of a launch
    std::atomic<uint64_t> seen{0};
    int found_n = 0;
    uint32_t open0 = 0, last_solved = 0;
    uint64_t steps_mark = 0;
    double overhead = 0.0;
};

// every entry of the table against d*G on the first engine's device, before anything walks
void tames_verify(const TamesFile &f, int gpu)
{
    const auto ts = Clock::now();
    bsgs_dev *dev = nullptr;
    CK(bsgs_dev_open(gpu, &dev));
    std::vector<uint8_t> jxy(64 * (size_t)BSGS_KANGAROO_JUMPS);
    for (uint32_t j = 0; j < BSGS_KANGAROO_JUMPS; j++) hs::affine_to_le(hs::G, &jxy[64 * (size_t)j], &jxy[64 * (size_t)j + 32]);
    CK(bsgs_kangaroo_setup(dev, jxy.data(), f.js.data(), f.dp, 64, 1, 64));      // the smallest herd: the verification's comb hangs on one
    const uint64_t T = f.x.size();
    uint64_t bad = 0;
    CK(verify_tame_entries(dev, f.x.data(), f.d.data(), T, &bad));
    bsgs_dev_close(dev);
    if (bad < T) die("Tame table is damaged: entry " + std::to_string(bad) + " does not match its offset");
    printf("[verify] tame table: %llu entries %.3fs\n", (unsigned long long)T, since(ts));
}

int tames_search(const KangConfig &c)
{
    // the table is read before any device is looked for
    TamesFile f;
    const std::string path = find_tames(c, c.ktames);
    const std::string bad = read_tames(path, f, c.tames_sym ? TAMES_VERSION_SYM : TAMES_VERSION);
    if (!bad.empty()) die(std::string(c.tames_sym ? "-ktamessym: " : "-ktames: ") + bad);
    std::vector<std::string> pub_hex;
    if (!c.infile.empty()) { Config fc; fc.infile = c.infile; pub_hex = read_pubs(fc); if (pub_hex.empty()) die("No public keys in " + c.infile); }
    else pub_hex.push_back(c.pub);
    if (pub_hex.size() > BSGS_KANGAROO_MAX_KEYS) die("-kangaroo -ktames: at most 65535 public keys, the file has " + std::to_string(pub_hex.size()));
    const uint32_t L = (uint32_t)pub_hex.size();
    std::vector<Affine> P(L);
    for (uint32_t k = 0; k < L; k++) if (!hs::parse_pubkey(P[k], pub_hex[k]) || !hs::on_curve(P[k])) die("Invalid Public Key (line " + std::to_string(k + 1) + ") length!!!");
    Prologue p(c);
    if (hs::fe_cmp(p.lo, f.lo) != 0 || hs::fe_cmp(p.hi, f.hi) != 0) die("Tame table was made for another range");
    printf("Kangaroo range [%s, %s], width 2^%.2f, %u public key(s), tame table %s\n", hs::fe_to_hex(p.lo).c_str(), hs::fe_to_hex(p.hi).c_str(), std::log2((double)p.W), L, path.c_str());
    SearchMode mode(c, P, f, p);
    p.complete(c, mode);
    if (!p.go) return 0;
    if (f.sym()) printf("Kangaroo: symmetric walk (negation map), %u jump points, jump scale %g, from the table\n", f.R, f.jumpscale);
    if (c.verify) tames_verify(f, p.gpus[0]);
    Shared sh(p);
    mode.prepare(p, sh);
    const Outcome o = run(c, p, sh, mode);
    const TamesRule &r = *mode.rule;
    if (o == GAVE_UP) printf("\nKangaroo: %u of %u keys open after 20 times the expected steps (are the keys in the range?)\n", L - r.solved(), L);
    else if (o != DONE) printf("\nKangaroo: stopped after %llu steps (%s), %u of %u keys open\n", (unsigned long long)sh.steps.load(), o == BUDGET ? "-ksteps" : "signal", L - r.solved(), L);
    printf("Job time %.2fs, %.3e kangaroo steps, %llu records seen (%llu dropped), %llu matches, %llu false matches, %llu re-seeds\n", since(p.t0), (double)sh.steps.load(),
           (unsigned long long)mode.seen.load(), (unsigned long long)sh.dropped.load(), (unsigned long long)r.matches(), (unsigned long long)r.false_matches(), (unsigned long long)r.reseeds());
    if (f.sym()) printf("Symmetric walk: %llu cycles retired\n", (unsigned long long)r.cycles());
    for (uint32_t e = 0; e < p.pl.engines; e++) printf("Engine %u (GPU #%d): %llu records\n", e, p.gpus[e], (unsigned long long)sh.engine_records[e]);
    printf("Found %d of %u\n", mode.found_n, L);
    fflush(stdout);
    return o == DONE ? 0 : (o == BUDGET || o == INTERRUPTED) ? 3 : 1;
}
// ---- -ktamesmerge ---------------------------------------------------------------------------------------------------------------------------------------
// "" when b was made by the walk of a, else the first field that differs, in the header's order
std::string walk_differs(const TamesFile &a, const TamesFile &b)
{
    if (a.dp != b.dp) return "-dp " + std::to_string(b.dp) + " against " + std::to_string(a.dp);
    if (hs::fe_cmp(a.lo, b.lo) != 0 || hs::fe_cmp(a.hi, b.hi) != 0) return "the range [" + hs::fe_to_hex(b.lo) + ", " + hs::fe_to_hex(b.hi) + "] is another";
    if (a.m != b.m) return "mean jump " + std::to_string(b.m) + " against " + std::to_string(a.m);
    if (a.R != b.R) return "-kjumps " + std::to_string(b.R) + " against " + std::to_string(a.R);
    if (memcmp(&a.jumpscale, &b.jumpscale, 8) != 0) return "the jump scale differs";
    for (uint32_t j = 0; j < a.R; j++) if (a.js[j] != b.js[j]) return "jump scalar " + std::to_string(j) + " differs";
    return "";
}

// a k-way merge by tag of tables that are strictly ascending each: one entry per tag, the first table that has it wins; the T lowest tags are written
int tames_merge(const KangConfig &c)
{
    std::vector<std::string> paths;
    for (const std::string &s : split_commas(c.ktamesmerge)) if (!s.empty()) paths.push_back(find_tames(c, s));
    if (paths.size() < 2) die("-ktamesmerge needs at least two tables: A,B[,C...]");
    std::vector<TamesFile> in(paths.size());
    for (size_t i = 0; i < paths.size(); i++) {
        const std::string bad = read_tames(paths[i], in[i], c.tames_sym ? TAMES_VERSION_SYM : TAMES_VERSION);
        if (!bad.empty()) die("-ktamesmerge: " + bad);
        const std::string differs = i ? walk_differs(in[0], in[i]) : "";
        if (!differs.empty()) die("-ktamesmerge: " + paths[i] + " was not made by the walk of " + paths[0] + ": " + differs);
    }
    TamesFile f;
    f.version = in[0].version; f.dp = in[0].dp; f.lo = in[0].lo; f.hi = in[0].hi; f.seed = in[0].seed; f.m = in[0].m; f.R = in[0].R; f.jumpscale = in[0].jumpscale; f.js = in[0].js;
    uint64_t total = 0, dropped = 0;
    for (const TamesFile &t : in) { f.steps += t.steps; total += t.x.size(); }
    typedef std::pair<uint64_t, size_t> Head;                          // (tag, table): the lowest tag first, of equal tags the earlier table
    std::priority_queue<Head, std::vector<Head>, std::greater<Head>> heads;
    std::vector<size_t> at(in.size(), 0);
    for (size_t i = 0; i < in.size(); i++) heads.push(Head(in[i].x[0], i));
    const uint64_t keep = c.ktn ? c.ktn : ~0ull;
    uint64_t tags = 0, last = 0;
    while (!heads.empty()) {
        const Head h = heads.top();
        heads.pop();
        const size_t i = h.second;
        if (tags && h.first == last) dropped++;                        // an earlier table had the tag
        else {
            tags++;
            last = h.first;
            if (f.x.size() < keep) { f.x.push_back(h.first); f.d.push_back(in[i].d[at[i]]); }
        }
        if (++at[i] < in[i].x.size()) heads.push(Head(in[i].x[at[i]], i));
    }
    printf("Merged %zu tame tables: %llu entries in all, %llu distinct tags, %llu dropped because an earlier table had their tag\n", in.size(), (unsigned long long)total,
           (unsigned long long)tags, (unsigned long long)dropped);
    if (c.ktn > tags) die("-ktamesmerge: -ktn " + std::to_string(c.ktn) + " is above the " + std::to_string(tags) + " tags of the union; nothing written");
    if (tags > (1ull << 31) && !c.ktn) die("-ktamesmerge: the union has " + std::to_string(tags) + " tags, a table holds at most 2^31: cut it with -ktn");
    if (c.verify) {                                                    // every entry written, on the first -d device; -noverify opens no device at all
        int ngpu = 0;
        CK(bsgs_dev_count(&ngpu));
        if (ngpu <= 0) die("No GPU found");
        tames_verify(f, c.devices.empty() ? 0 : atoi(c.devices.c_str()));
    }
    std::string path = c.ktamesgen;
    if (path.find('/') == std::string::npos) path = c.dir + "/" + path;
    if (!write_tames(path, f)) die("cannot write " + path);
    printf("Tame table %s: %zu entries, %.3e steps\n", path.c_str(), f.x.size(), (double)f.steps);
    fflush(stdout);
    return 0;
}
}  // namespace

int kangaroo_tames_main(const KangConfig &c) { return !c.ktamesmerge.empty() ? tames_merge(c) : c.ktamesgen.empty() ? tames_search(c) : tames_generate(c); }

// -selftest kangaroo-tames [sym] FILE [pk pke]: the header fields of a tame table, its ordering, and with a range whether it is the table's.  sym: the reader
// of -ktamessym (version 2; two more lines, "jumps <R>" and "jump scale <s>"), else the reader of -ktames (version 1)
int kangaroo_tames_selftest(const std::vector<std::string> &args)
{
    const bool sym = !args.empty() && args[0] == "sym";
    const std::vector<std::string> a(args.begin() + (sym ? 1 : 0), args.end());
    if (a.size() != 1 && a.size() != 3) return 2;
    TamesFile f;
    const std::string bad = read_tames(a[0], f, sym ? TAMES_VERSION_SYM : TAMES_VERSION);
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    printf("version %u\ndp %u\npk %s\npke %s\nentries %zu\nsteps %llu\nseed 0x%llx\nmean jump %llu\n", f.version, f.dp, hs::fe_to_hex(f.lo).c_str(), hs::fe_to_hex(f.hi).c_str(), f.x.size(),
           (unsigned long long)f.steps, (unsigned long long)f.seed, (unsigned long long)f.m);
    if (sym) printf("jumps %u\njump scale %g\n", f.R, f.jumpscale);
    if (a.size() == 3) {
        Scalar lo, hi;
        if (!hs::fe_from_hex(lo, cut_hex(a[1])) || !hs::fe_from_hex(hi, cut_hex(a[2]))) return 2;
        if (hs::fe_cmp(lo, f.lo) != 0 || hs::fe_cmp(hi, f.hi) != 0) { fprintf(stderr, "Tame table was made for another range\n"); return 1; }
    }
    printf("ok\n");
    return 0;
}

// -selftest kangaroo-tames-gen <T> <item>...: the rule of -ktamesgen -ktamesdev on scripted hand-backs, no GPU.
//   D|U|Z|F,<x hex>,<d hex: 128-bit two's complement>,<kangaroo>   a record the device handed back as DEAD, DUPLICATE, TAG_ZERO or FULL
//   E,<n>                                                          the device's table holds n entries after this launch
// One line per item: "reseed <kangaroo>", "merge <kangaroo>" (it starts afresh too), "held <kangaroo>" (the host keeps the entry), "dropped", "ignored" (the
// table was done), "entries <device + host>"; "done" once after the item that completes the table; then "summary <re-seeds> <merges> <held> <dropped> <done>".
int kangaroo_tames_gen_selftest(const std::vector<std::string> &a)
{
    if (a.empty()) return 2;
    const uint64_t T = strtoull(a[0].c_str(), nullptr, 0);
    if (!T || T > (1ull << 31)) return 2;
    GenRule rule(T);
    bool said = false;
    for (size_t i = 1; i < a.size(); i++) {
        const std::vector<std::string> t = split_commas(a[i]);
        if (t.size() == 2 && t[0] == "E") {
            rule.entries(strtoull(t[1].c_str(), nullptr, 0));
            printf("entries %llu\n", (unsigned long long)rule.total());
        } else if (t.size() == 4 && t[0].size() == 1 && strchr("DUZF", t[0][0])) {
            Scalar x, dd;
            if (!hs::fe_from_hex(x, t[1]) || !hs::fe_from_hex(dd, t[2]) || dd.l[2] || dd.l[3]) return 2;
            const unsigned long long kid = strtoull(t[3].c_str(), nullptr, 10);
            const uint32_t reason = t[0] == "D" ? BSGS_KANGAROO_GEN_DEAD : t[0] == "U" ? BSGS_KANGAROO_GEN_DUPLICATE : t[0] == "Z" ? BSGS_KANGAROO_GEN_TAG_ZERO : BSGS_KANGAROO_GEN_FULL;
            switch (rule.record(reason, x.l[0], (i128)(((u128)dd.l[1] << 64) | dd.l[0]))) {
                case GenRule::RESEED: printf("reseed %llu\n", kid); break;
                case GenRule::MERGE: printf("merge %llu\n", kid); break;
                case GenRule::HELD: printf("held %llu\n", kid); break;
                case GenRule::DROPPED: printf("dropped\n"); break;
                case GenRule::IGNORED: printf("ignored\n"); break;
            }
        } else return 2;
        if (rule.done() && !said) { printf("done\n"); said = true; }
    }
    printf("summary %llu %llu %zu %llu %d\n", (unsigned long long)rule.reseeds(), (unsigned long long)rule.merges(), rule.held().size(), (unsigned long long)rule.dropped(), rule.done() ? 1 : 0);
    return 0;
}

// -selftest kangaroo-tames-image: tags (decimal or 0x..., white space between them) from stdin -> "lines <n>" and the SHA-1 of the image
int kangaroo_tames_image_selftest(const std::vector<std::string> &)
{
    std::vector<uint64_t> tags;
    std::string tok;
    while (std::cin >> tok) tags.push_back(strtoull(tok.c_str(), nullptr, 0));
    uint64_t lines = 0;
    if (bsgs_kangaroo_tames_image(tags.data(), tags.size(), nullptr, 0, &lines) != BSGS_OK) { fprintf(stderr, "%s\n", bsgs_last_error()); return 1; }
    std::string image((size_t)lines * 64, '\0');
    if (bsgs_kangaroo_tames_image(tags.data(), tags.size(), &image[0], image.size(), &lines) != BSGS_OK) { fprintf(stderr, "%s\n", bsgs_last_error()); return 1; }
    printf("lines %llu\ndigest %s\n", (unsigned long long)lines, sha1_hex(image).c_str());
    return 0;
}

// -selftest kangaroo-tames-search FILE <pubkey>[,<pubkey>...] <wild kangaroos> <launches before a kangaroo is aged> <item>...: the search rule on a script.
//   R,<x hex>,<d hex: 128-bit two's complement>,<kangaroo>   a record of wild kangaroo <kangaroo>; the table is looked up as the device does, by the low 64 bits
//   D,<kangaroo>                                             its DEAD record
//   L                                                        a launch of every kangaroo has ended
// One line per event: "miss", "found <k> <key hex>", "false", "stale", "reseed <kangaroo> <key>", "aged <kangaroo> <key>", and after a found key, for each of
// its kangaroos in ascending order, "reassign <kangaroo> <key>" ("rest <kangaroo>" when no key is open); then "summary <matches> <false matches> <re-seeds> <solved>".
// -selftest kangaroo-tames-search sym FILE ...: the rule of a table of the symmetric walk (version 2).  Record types W and N (a wild kangaroo, N: with NEG) in
// the place of R, D and C,<kangaroo> (C: the cycle check's DEAD | CYCLE record); a key equal to (pk + W/2)*G is presolved; the summary line ends with the
// cycles retired.
int kangaroo_tames_search_selftest(const std::vector<std::string> &args)
{
    const bool sym = !args.empty() && args[0] == "sym";
    const std::vector<std::string> a(args.begin() + (sym ? 1 : 0), args.end());
    if (a.size() < 4) return 2;
    TamesFile f;
    const std::string bad = read_tames(a[0], f, sym ? TAMES_VERSION_SYM : TAMES_VERSION);
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
    std::vector<Affine> P;
    if (!parse_pubs(a[1], P) || P.empty() || P.size() > BSGS_KANGAROO_MAX_KEYS) return 2;
    const uint64_t n_wild = strtoull(a[2].c_str(), nullptr, 10), limit = strtoull(a[3].c_str(), nullptr, 10);
    if (!n_wild || n_wild > (1u << 20)) return 2;
    const Affine aG = hs::point_mul(hs::G, sym ? hs::sc_add(f.lo, hs::sc_from_u128(range_width(f.lo, f.hi) / 2)) : f.lo);
    std::vector<bool> presolved(P.size(), false);
    bool open = false;
    for (size_t k = 0; k < P.size(); k++) {
        presolved[k] = hs::fe_equal(P[k].x, aG.x) && hs::fe_equal(P[k].y, aG.y);
        if (presolved[k]) printf("presolved %zu\n", k); else open = true;
    }
    if (!open) { printf(sym ? "summary 0 0 0 %zu 0\n" : "summary 0 0 0 %zu\n", P.size()); return 0; }
    TamesRule rule(f, range_width(f.lo, f.hi), P, presolved, n_wild, limit);
    auto start_afresh = [&](const char *word, uint64_t w) {
        uint32_t k = 0;
        if (rule.reseed(w, &k)) printf("%s %llu %u\n", word, (unsigned long long)w, k); else printf("rest %llu\n", (unsigned long long)w);
    };
    for (size_t i = 4; i < a.size(); i++) {
        const std::vector<std::string> t = split_commas(a[i]);
        std::vector<TamesRule::Event> ev;
        uint64_t w = 0;
        if (t.size() == 1 && t[0] == "L") {
            std::vector<uint64_t> aged;
            rule.launch_done(0, n_wild, aged);
            for (uint64_t v : aged) start_afresh("aged", v);
            continue;
        } else if (t.size() == 2 && (t[0] == "D" || (sym && t[0] == "C"))) {
            w = strtoull(t[1].c_str(), nullptr, 10);
            if (w >= n_wild) return 2;
            rule.record(BSGS_KANGAROO_WILD | BSGS_KANGAROO_DEAD | (t[0] == "C" ? BSGS_KANGAROO_CYCLE : 0u) | rule.key_of(w) << BSGS_KANGAROO_KEY_SHIFT, 0, 0, ev);
        } else if (t.size() == 4 && (sym ? t[0] == "W" || t[0] == "N" : t[0] == "R")) {
            Scalar x, dd;
            if (!hs::fe_from_hex(x, t[1]) || !hs::fe_from_hex(dd, t[2]) || dd.l[2] || dd.l[3]) return 2;
            w = strtoull(t[3].c_str(), nullptr, 10);
            if (w >= n_wild) return 2;
            const auto it = std::lower_bound(f.x.begin(), f.x.end(), x.l[0]);
            if (it == f.x.end() || *it != x.l[0]) { printf("miss\n"); continue; }
            rule.record(BSGS_KANGAROO_WILD | (t[0] == "N" ? BSGS_KANGAROO_NEG : 0u) | rule.key_of(w) << BSGS_KANGAROO_KEY_SHIFT, (uint32_t)(it - f.x.begin()) + 1u, (i128)(((u128)dd.l[1] << 64) | dd.l[0]), ev);
        } else return 2;
        for (const TamesRule::Event &e : ev) switch (e.what) {
            case TamesRule::FALSE_MATCH: printf("false\n"); break;
            case TamesRule::STALE: printf("stale\n"); break;
            case TamesRule::RESEED: start_afresh("reseed", w); break;
            case TamesRule::FOUND: {
                printf("found %u %s\n", e.a, hs::fe_to_hex(e.key).c_str());
                const std::vector<uint32_t> before = rule.keys();
                for (uint64_t v = 0; v < before.size(); v++) if (before[v] == e.a) start_afresh("reassign", v);
                break;
            }
        }
    }
    printf("summary %llu %llu %llu %u", (unsigned long long)rule.matches(), (unsigned long long)rule.false_matches(), (unsigned long long)rule.reseeds(), rule.solved());
    if (sym) printf(" %llu", (unsigned long long)rule.cycles());
    printf("\n");
    return 0;
}
