// host_kangaroo.cpp -- bsgs_mi355x -kangaroo: Pollard's kangaroo (lambda) search of ONE public key in [pk, pke] for ranges too wide for a baby table
// (include/bsgs_hip.h "Kangaroo" states the walk).  Herds of tame and wild kangaroos on every engine (-d, one engine per listed device), one
// host table of distinguished points shared by all engines and fed by a collector thread, the key written to win.txt through the JobList as the BSGS path
// writes it.  -selftest kangaroo drives the same table with a scripted record stream and no GPU.
#include "host.h"

#include <random>
#include <unordered_map>

namespace {
using Clock = std::chrono::steady_clock;
typedef unsigned __int128 u128;
typedef __int128 i128;
double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

uint64_t splitmix64(uint64_t &state)
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
u128 draw128(uint64_t &state) { const uint64_t lo = splitmix64(state), hi = splitmix64(state); return ((u128)hi << 64) | lo; }
// start offsets (tests/kangaroo_model.py herd_offset): tame t uniform in [1, W), wild u uniform in [-W/2, W/2), both from the seeded stream
i128 herd_offset(uint64_t &state, u128 W, bool wild)
{
    const u128 r = draw128(state);
    return wild ? (i128)(r % W) - (i128)(W / 2) : (i128)(1 + r % (W - 1));
}
Scalar sc_from_i128(i128 v) { return v >= 0 ? hs::sc_from_u128((u128)v) : hs::sc_neg(hs::sc_from_u128((u128)-v)); }
bool parse_hex128(const std::string &s, u128 &v)
{
    Scalar t;
    if (!hs::fe_from_hex(t, s) || t.l[2] || t.l[3]) return false;
    v = ((u128)t.l[1] << 64) | t.l[0];
    return true;
}

// fixed-base comb for 128-bit scalars: table[k][v] = v * 2^(8k) * G, sixteen mixed additions per point
struct Comb {
    std::vector<std::vector<Affine>> tab;
    Comb()
    {
        Affine base = hs::G;
        for (int k = 0; k < 16; k++) {
            std::vector<Affine> m = hs::multiples(base, 256);              // base, 2 base, ..., 256 base
            tab.push_back(std::vector<Affine>(m.begin(), m.end() - 1));
            base = m.back();
        }
    }
    hs::Jac mul(u128 s) const
    {
        hs::Jac r; r.inf = true;
        for (int k = 0; k < 16; k++) { const unsigned v = (unsigned)(s >> (8 * k)) & 255u; if (v) r = hs::jac_add_affine(r, tab[k][v - 1]); }
        return r;
    }
};

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
    KangarooTable(const Scalar &a, u128 W, const Affine &P) : a_(a), W_(W), P_(P) { map_.reserve(1u << 20); }
    // one record: FOUND (*key = k), RESEED (the record's kangaroo follows another of its type, or died), FALSE_MATCH (tame and wild x agree in the key but the
    // difference does not solve: counted, ignored), REPEAT (the same kangaroo's own point again), NEW (stored)
    Verdict add(const uint8_t x[32], u128 d, uint32_t kid, uint32_t flags, Scalar *key)
    {
        if (flags & BSGS_KANGAROO_DEAD) { reseeds_++; return RESEED; }
        uint64_t k64;
        memcpy(&k64, x, 8);
        const bool wild = flags & BSGS_KANGAROO_WILD;
        auto it = map_.find(k64);
        if (it == map_.end()) { map_.emplace(k64, Entry{d, kid, wild}); return NEW; }
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
private:
    struct Entry { u128 d; uint32_t kid; bool wild; };
    const Scalar a_;
    const u128 W_;
    const Affine P_;
    std::unordered_map<uint64_t, Entry> map_;
    uint64_t false_ = 0, reseeds_ = 0;
};

// -selftest kangaroo <pk hex> <pke hex> <pubkey> <record>...  record = T|W|D,<x hex>,<d hex: 128-bit two's complement>,<kangaroo> (D: a dead record).
// Prints one line per record: "new", "found <key hex>", "reseed <kangaroo>", "false", "repeat"; then "summary <stored> <false matches> <reseeds>".
int kangaroo_selftest(const std::vector<std::string> &a)
{
    if (a.size() < 3) return 2;
    Scalar lo, hi;
    Affine P;
    if (!hs::fe_from_hex(lo, a[0]) || !hs::fe_from_hex(hi, a[1]) || !hs::parse_pubkey(P, cut_hex(a[2])) || !hs::on_curve(P)) return 2;
    const Scalar w = hs::sc_sub(hi, lo);
    if (w.l[2] || w.l[3]) return 2;
    KangarooTable tab(lo, (((u128)w.l[1] << 64) | w.l[0]) + 1, P);
    for (size_t i = 3; i < a.size(); i++) {
        std::vector<std::string> f;
        std::stringstream ss(a[i]);
        std::string tok;
        while (std::getline(ss, tok, ',')) f.push_back(tok);
        if (f.size() != 4 || f[0].size() != 1 || !strchr("TWD", f[0][0])) return 2;
        Scalar x;
        u128 d;
        if (!hs::fe_from_hex(x, f[1]) || !parse_hex128(f[2], d)) return 2;
        uint8_t xb[32];
        hs::fe_to_le(x, xb);
        const uint32_t flags = f[0] == "W" ? BSGS_KANGAROO_WILD : f[0] == "D" ? BSGS_KANGAROO_DEAD : 0u;
        Scalar key;
        switch (tab.add(xb, d, (uint32_t)strtoul(f[3].c_str(), nullptr, 10), flags, &key)) {
        case KangarooTable::NEW: printf("new\n"); break;
        case KangarooTable::FOUND: printf("found %s\n", hs::fe_to_hex(key).c_str()); break;
        case KangarooTable::RESEED: printf("reseed %s\n", f[3].c_str()); break;
        case KangarooTable::FALSE_MATCH: printf("false\n"); break;
        case KangarooTable::REPEAT: printf("repeat\n"); break;
        }
    }
    printf("summary %zu %llu %llu\n", tab.size(), (unsigned long long)tab.false_matches(), (unsigned long long)tab.reseeds());
    return 0;
}

namespace {
struct KangConfig {
    std::string devices, pub = Config().pub, pk = Config().pk, pke = Config().pke, dir = ".";
    int dp = -1;                                   // -dp (default: from W)
    uint64_t kn = 0;                               // -kn: kangaroos per engine (default: from W)
    uint64_t seed = 0;
    bool seed_given = false;
};

KangConfig parse_kangaroo_args(int argc, char **argv)
{
    KangConfig c;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        for (auto &ch : a) ch = (char)tolower(ch);
        auto next = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
        if (a == "-kangaroo") continue;
        else if (a == "-h") { usage(Config()); exit(0); }
        else if (a == "-pb") c.pub = cut_hex(next());
        else if (a == "-pk") c.pk = cut_hex(next());
        else if (a == "-pke") c.pke = cut_hex(next());
        else if (a == "-d") c.devices = next();
        else if (a == "-dir") c.dir = next();
        else if (a == "-dp") { c.dp = atoi(next().c_str()); if (c.dp < 0 || c.dp > 32) die("-dp must be 0..32"); }
        else if (a == "-kn") c.kn = strtoull(next().c_str(), nullptr, 10);
        else if (a == "-kseed") { c.seed = strtoull(next().c_str(), nullptr, 0); c.seed_given = true; }
        else if (a == "-wl") die("-kangaroo: checkpoint / resume (-wl) is not supported in kangaroo mode");
        else if (a == "-w" || a == "-htsz" || a == "-infile" || a == "-onlygen") die("-kangaroo cannot be combined with " + a + " (no baby table, one public key)");
        else die("Unknown parameter with -kangaroo: " + a);
    }
    return c;
}

// what the engines and the collector share
struct Shared {
    std::atomic<bool> stop{false}, found{false};
    std::atomic<uint64_t> steps{0}, dps{0}, dropped{0};
    std::mutex rng_m;
    uint64_t rng = 0;                              // the seeded stream: initial herds in engine order, then every re-seed
    std::mutex q_m; std::condition_variable q_cv;
    std::deque<std::pair<uint32_t, std::vector<bsgs_kangaroo_record>>> queue;     // (engine, records of one launch)
    std::vector<std::unique_ptr<std::mutex>> reseed_m;
    std::vector<std::vector<uint32_t>> reseed;     // per engine: kangaroos (local index) to start afresh
    std::vector<uint64_t> engine_records;
    std::mutex err_m; std::string err;
    Scalar key;
};

struct Plan { uint32_t engines, dp, G, S, cap; uint64_t kn; double expected; };
}  // namespace

int kangaroo_main(int argc, char **argv)
{
    printf("BSGS MI355X kangaroo mode on %s\n", bsgs_version());
    const KangConfig c = parse_kangaroo_args(argc, argv);
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
    printf("Kangaroo range [%s, %s], width 2^%.2f\n", hs::fe_to_hex(lo).c_str(), hs::fe_to_hex(hi).c_str(), std::log2(Wd));
    const Affine Q = hs::point_add(P, hs::affine_neg(hs::point_mul(hs::G, lo)));
    JobList jobs({c.pub}, Recovery(), c.dir, [](int, const std::string &, const Scalar &) {});      // win.txt as the BSGS path writes it
    { Config rc; rc.dir = c.dir; read_recovery(rc); }                                                  // (a fresh run: win.txt starts empty, as there)
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
    int cus = 256;
    { bsgs_dev *d = nullptr; CK(bsgs_dev_open(gpus[0], &d)); bsgs_dev_cu_count(d, &cus); bsgs_dev_close(d); }
    // defaults from W: expected DPs (2 sqrt(W) / 2^dp) within 2^25 host entries, DP overhead N_k 2^dp at most sqrt(W) / 8, a full herd is 16 kangaroos
    // per thread at four waves per SIMD (one batch inversion per block costs about 70 multiplications per thread: 16 kangaroos share it)
    Plan pl;
    pl.engines = (uint32_t)gpus.size();
    pl.dp = c.dp >= 0 ? (uint32_t)c.dp : (uint32_t)std::min(32.0, std::max(0.0, std::ceil(std::log2(2.0 * sqrtW / 33554432.0))));
    const uint64_t full = (uint64_t)cus * 1024 * 16;
    uint64_t kn = c.kn ? c.kn : (uint64_t)std::min((double)full, sqrtW / 8.0 / std::ldexp(1.0, (int)pl.dp) / pl.engines);
    kn = std::max<uint64_t>(kn, 64);
    pl.G = 16;                                                        // fewer kangaroos per thread only while the GPU would have less than two waves per SIMD
    while (pl.G > 1 && kn / pl.G < (uint64_t)cus * 512) pl.G /= 2;
    kn = std::max<uint64_t>(64ull * pl.G, kn / (64ull * pl.G) * (64ull * pl.G));
    if (kn > (1ull << 26)) die("-kn: at most 2^26 kangaroos per engine");
    pl.kn = kn;
    const double Nk = (double)kn * pl.engines;
    pl.expected = 2.0 * sqrtW + Nk * std::ldexp(1.0, (int)pl.dp);
    pl.S = (uint32_t)std::max(8.0, std::min(1024.0, pl.expected / Nk / 8.0));
    const double per_launch = Nk / pl.engines * pl.S / std::ldexp(1.0, (int)pl.dp);
    pl.cap = (uint32_t)std::min<double>(1u << 22, 2.0 * per_launch + 65536.0);
    uint64_t seed = c.seed;
    if (!c.seed_given) { std::random_device rd; seed = ((uint64_t)rd() << 32) ^ rd(); }
    printf("Kangaroo: %u engine(s) x %llu kangaroos (%u per thread), -dp %u, %u steps per launch, -kseed 0x%llx\n", pl.engines, (unsigned long long)kn, pl.G, pl.dp, pl.S,
           (unsigned long long)seed);
    printf("Expected steps: 2^%.2f (2 sqrt(W) + DP overhead), expected DPs 2^%.2f\n", std::log2(pl.expected), std::log2(2.0 * sqrtW / std::ldexp(1.0, (int)pl.dp) + 1.0));
    if (c.dp < 0 && 2.0 * sqrtW / std::ldexp(1.0, (int)pl.dp) > 67108864.0) printf("WARNING: the expected DP count exceeds 2^26 host entries even at -dp 32\n");

    // jump table: s_j uniform in [1, 2m), mean m = N_k sqrt(W) / 4 (at most 2^62)
    Shared sh;
    sh.rng = seed;
    const double mean = std::max(1.0, std::min(std::ldexp(1.0, 62), Nk * sqrtW / 4.0));
    std::vector<uint64_t> js(BSGS_KANGAROO_JUMPS);
    std::vector<uint8_t> jxy(64 * BSGS_KANGAROO_JUMPS);
    for (int j = 0; j < BSGS_KANGAROO_JUMPS; j++) {
        const uint64_t span = (uint64_t)(2.0 * mean) > 1 ? (uint64_t)(2.0 * mean) - 1 : 1;
        js[j] = 1 + splitmix64(sh.rng) % span;
        const Affine J = hs::point_mul(hs::G, hs::fe_from_u64(js[j]));
        hs::affine_to_le(J, &jxy[64 * j], &jxy[64 * j + 32]);
    }
    const Comb comb;
    sh.reseed.resize(pl.engines);
    sh.engine_records.assign(pl.engines, 0);
    for (uint32_t e = 0; e < pl.engines; e++) sh.reseed_m.emplace_back(new std::mutex);
    const auto t0 = Clock::now();

    // a kangaroo's start: offsets from the shared stream (under its lock), points on the calling thread; a wild start at infinity IS the key
    auto starts = [&](const std::vector<uint32_t> &idx, std::vector<bsgs_kangaroo_state> &out) {
        std::vector<i128> d(idx.size());
        std::vector<bool> wild(idx.size());
        {
            std::lock_guard<std::mutex> lk(sh.rng_m);
            for (size_t k = 0; k < idx.size(); k++) { wild[k] = idx[k] >= kn / 2; d[k] = herd_offset(sh.rng, W, wild[k]); }
        }
        const std::vector<Affine> pts = herd_points(comb, Q, d, wild);
        out.resize(idx.size());
        for (size_t k = 0; k < idx.size(); k++) {
            if (pts[k].inf) {                                            // Q + u G = infinity: k' = -u
                sh.key = hs::sc_add(lo, sc_from_i128(-d[k]));
                sh.found = true; sh.stop = true;
            }
            out[k] = to_state(pts[k], d[k], wild[k]);
        }
    };
    // initial herds, in engine order from the seeded stream (several threads for the points)
    std::vector<std::vector<bsgs_kangaroo_state>> herds(pl.engines);
    for (uint32_t e = 0; e < pl.engines; e++) {
        herds[e].resize(kn);
        const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<i128> off(kn);
        for (uint64_t i = 0; i < kn; i++) off[i] = herd_offset(sh.rng, W, i >= kn / 2);
        std::vector<std::thread> tt;
        for (unsigned q = 0; q < nt; q++) tt.emplace_back([&, q]() {
            const uint64_t b0 = kn * q / nt, b1 = kn * (q + 1) / nt;
            std::vector<i128> dd(off.begin() + (long)b0, off.begin() + (long)b1);
            std::vector<bool> ww(b1 - b0);
            for (uint64_t i = b0; i < b1; i++) ww[i - b0] = i >= kn / 2;
            const std::vector<Affine> pts = herd_points(comb, Q, dd, ww);
            for (uint64_t i = b0; i < b1; i++) {
                if (pts[i - b0].inf) { std::lock_guard<std::mutex> lk(sh.rng_m); sh.key = hs::sc_add(lo, sc_from_i128(-dd[i - b0])); sh.found = true; sh.stop = true; }
                herds[e][i] = to_state(pts[i - b0], dd[i - b0], ww[i - b0]);
            }
        });
        for (auto &t : tt) t.join();
    }
    printf("[startup] %-44s %.3fs\n", "herds (host)", since(t0));

    // engines: one thread each, all calls for a device from the thread that opened it
    auto engine = [&](uint32_t e) {
        bsgs_dev *dev = nullptr;
        auto bad = [&](const char *what) { std::lock_guard<std::mutex> lk(sh.err_m); if (sh.err.empty()) sh.err = std::string(what) + ": " + bsgs_last_error(); sh.stop = true; };
        if (bsgs_dev_open(gpus[e], &dev) != BSGS_OK) { bad("bsgs_dev_open"); return; }
        if (bsgs_kangaroo_setup(dev, jxy.data(), js.data(), pl.dp, (uint32_t)kn, pl.G, pl.cap) != BSGS_OK) { bad("bsgs_kangaroo_setup"); bsgs_dev_close(dev); return; }
        if (bsgs_kangaroo_upload(dev, 0, (uint32_t)kn, herds[e].data()) != BSGS_OK) { bad("bsgs_kangaroo_upload"); bsgs_dev_close(dev); return; }
        std::vector<bsgs_kangaroo_state>().swap(herds[e]);
        std::vector<bsgs_kangaroo_record> recs(pl.cap);
        while (!sh.stop.load()) {
            std::vector<uint32_t> rs;
            { std::lock_guard<std::mutex> lk(*sh.reseed_m[e]); rs.swap(sh.reseed[e]); }
            if (!rs.empty()) {
                std::sort(rs.begin(), rs.end());
                rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
                std::vector<bsgs_kangaroo_state> st;
                starts(rs, st);
                if (bsgs_kangaroo_upload_list(dev, rs.data(), (uint32_t)rs.size(), st.data()) != BSGS_OK) { bad("bsgs_kangaroo_upload_list"); break; }
            }
            uint32_t n = 0;
            uint64_t dropped = 0;
            if (bsgs_kangaroo_run(dev, pl.S, recs.data(), pl.cap, &n, &dropped, nullptr) != BSGS_OK) { bad("bsgs_kangaroo_run"); break; }
            sh.steps += kn * pl.S;
            sh.dropped += dropped;
            { std::lock_guard<std::mutex> lk(sh.q_m); sh.queue.emplace_back(e, std::vector<bsgs_kangaroo_record>(recs.begin(), recs.begin() + n)); }
            sh.q_cv.notify_one();
        }
        bsgs_dev_close(dev);
    };
    // the collector: every engine's records into the one table
    KangarooTable table(lo, W, P);
    std::atomic<bool> engines_done{false};
    std::thread collector([&]() {
        for (;;) {
            std::pair<uint32_t, std::vector<bsgs_kangaroo_record>> b;
            {
                std::unique_lock<std::mutex> lk(sh.q_m);
                sh.q_cv.wait_for(lk, std::chrono::milliseconds(100), [&] { return !sh.queue.empty() || engines_done.load(); });
                if (sh.queue.empty()) { if (engines_done.load()) return; continue; }
                b = std::move(sh.queue.front());
                sh.queue.pop_front();
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
    std::vector<std::thread> th;
    if (!sh.stop.load()) for (uint32_t e = 0; e < pl.engines; e++) th.emplace_back(engine, e);
    auto last_t = Clock::now();
    uint64_t last_steps = 0;
    bool gave_up = false;
    while (!sh.stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        const auto now = Clock::now();
        if (std::chrono::duration<double>(now - last_t).count() >= 2.0) {
            const uint64_t st = sh.steps.load();
            const double rate = (st - last_steps) / std::chrono::duration<double>(now - last_t).count();
            printf("\r[%u] %.3e steps/s  steps 2^%.2f of expected 2^%.2f  DPs %llu  %.0fs   ", pl.engines, rate, st ? std::log2((double)st) : 0.0, std::log2(pl.expected),
                   (unsigned long long)sh.dps.load(), since(t0));
            fflush(stdout);
            last_steps = st; last_t = now;
        }
        if ((double)sh.steps.load() > 20.0 * pl.expected) { gave_up = true; sh.stop = true; }
    }
    for (auto &t : th) t.join();
    engines_done = true;
    sh.q_cv.notify_all();
    collector.join();
    if (!sh.err.empty()) die(sh.err);
    const double secs = since(t0);
    std::string text, win;
    if (sh.found.load()) {
        std::string console;
        win = key_lines(cl.listpos, sh.key, P, console);
        text = console;
    } else text = gave_up ? "\nKangaroo: no key after 20 times the expected steps (is the key in the range?)\n" : "\nReached end of space\n";
    char tail[512];
    snprintf(tail, sizeof tail, "Job time %.2fs, %.3e kangaroo steps, %llu DPs (%zu in the table, %llu dropped), %llu false matches, %llu re-seeds\n", secs,
             (double)sh.steps.load(), (unsigned long long)sh.dps.load(), table.size(), (unsigned long long)sh.dropped.load(), (unsigned long long)table.false_matches(),
             (unsigned long long)table.reseeds());
    text += tail;
    for (uint32_t e = 0; e < pl.engines; e++) text += "Engine " + std::to_string(e) + " (GPU #" + std::to_string(gpus[e]) + "): " + std::to_string(sh.engine_records[e]) + " records\n";
    fputs(text.c_str(), stdout);                                       // one lane: the JobList leaves the console to the job (it appends win.txt)
    jobs.finish(0, text, sh.found.load(), win);
    printf("Found %d of %zu\n", jobs.found(), jobs.size());
    fflush(stdout);
    return sh.found.load() ? 0 : 1;
}
