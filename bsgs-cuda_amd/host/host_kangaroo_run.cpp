// host_kangaroo_run.cpp -- what every mode of bsgs_mi355x -kangaroo runs through (host_kangaroo_run.h): the prologue (range, -wl, devices,
// plan, seed, jump table) and the driver: one thread per engine, the collector that feeds the mode's table, the monitor with the -wt save handshake and the
// signals, the shutdown and the last save.  The host's comb start points, which both modes use with -kcpuseed, are here too.
#include "host_kangaroo_run.h"

#include <csignal>
#include <random>

using namespace kang;

std::vector<size_t> kang::comb_states(const Comb &C, const std::vector<i128> &d, const std::vector<uint32_t> &fl, const std::vector<const Affine *> &Q, std::vector<bsgs_kangaroo_state> &out)
{
    std::vector<hs::Jac> j(d.size());
    for (size_t k = 0; k < d.size(); k++) {
        const bool neg = d[k] < 0;
        hs::Jac p = C.mul(neg ? (u128)-d[k] : (u128)d[k]);
        if (neg && !p.inf) p.y = hs::fe_neg(p.y);
        if (Q[k]) p = hs::jac_add_affine(p, *Q[k]);
        j[k] = p;
    }
    const std::vector<Affine> pts = hs::batch_to_affine(j);
    std::vector<size_t> inf;
    out.resize(d.size());
    for (size_t k = 0; k < d.size(); k++) {
        bsgs_kangaroo_state &s = out[k];
        memset(&s, 0, sizeof s);
        if (pts[k].inf) inf.push_back(k);
        else hs::affine_to_le(pts[k], s.x, s.y);
        memcpy(s.d, &d[k], 16);
        s.flags = fl[k];
    }
    return inf;
}

void kang::report_key(const std::string &dir, int listpos, const Scalar &key, const Affine &pub)
{
    std::string console;
    const std::string win = key_lines(listpos, key, pub, console);
    fputs(console.c_str(), stdout);
    fflush(stdout);
    std::ofstream f(dir + "/win.txt", std::ios::app | std::ios::binary);
    f << win;
}

void kang::plan_launch(Plan &pl, double sqrtW, double expected0, double min_launch, bool bound, bool dp_free)
{
    const double Nk = (double)pl.kn * pl.engines, half = 2097152.0;
    auto expected = [&]() { return (expected0 > 0.0 ? expected0 : 2.0 * sqrtW) + Nk * std::ldexp(1.0, (int)pl.dp); };
    auto records = [&]() { return (double)pl.kn * pl.S / std::ldexp(1.0, (int)pl.dp); };
    pl.expected = expected();
    pl.S = (uint32_t)std::max(min_launch, std::min(1024.0, pl.expected / Nk / 8.0));
    if (bound) {
        if (records() > half) pl.S = (uint32_t)std::max(min_launch, std::floor(half * std::ldexp(1.0, (int)pl.dp) / (double)pl.kn));
        while (dp_free && records() > half && pl.dp < 32) { pl.dp++; pl.expected = expected(); }
    }
    pl.cap = (uint32_t)std::min<double>(1u << 22, 2.0 * records() + 65536.0);
}

Prologue::Prologue(const KangConfig &c)
{
    if (!hs::fe_from_hex(lo, c.pk) || hs::fe_is_zero(lo)) die("Start range can`t be zero");
    if (!hs::fe_from_hex(hi, c.pke)) die("Invalid range (-pkend) length!!!");
    if (hs::fe_cmp(hi, lo) <= 0) die("End range must be more then start range");
    const Scalar wm1 = hs::sc_sub(hi, lo);
    if (wm1.l[2] || wm1.l[3] || (wm1.l[1] >> 61)) die("-kangaroo: the range width must be at most 2^125");
    W = (((u128)wm1.l[1] << 64) | wm1.l[0]) + 1;
    if (W < ((u128)1 << 20)) die("-kangaroo: the range width must be at least 2^20");
    sqrtW = std::sqrt((double)W);
    work_path = c.dir + "/kangaroo.work"; work_tmp = c.dir + "/kangaroo.temp";
}

static std::vector<std::string> device_list(const std::string &devices)
{
    std::vector<std::string> dl;
    std::stringstream ss(devices);
    std::string tok;
    while (std::getline(ss, tok, ',')) dl.push_back(tok);
    return dl;
}

void Prologue::complete(const KangConfig &c, Mode &mode)
{
    const std::vector<std::string> dl = device_list(c.devices);
    // -wl: the work file is read before any device is looked for; a file that is missing or is not a work file of this mode ends the run here
    resume = !c.wl.empty();
    wl_path = c.wl;
    if (resume) {
        struct stat sb;
        if (stat(wl_path.c_str(), &sb) != 0 && stat((c.dir + "/" + c.wl).c_str(), &sb) == 0) wl_path = c.dir + "/" + c.wl;
        const std::string bad = read_work(wl_path, wf, true, mode.version);
        if (!bad.empty()) die(std::string(mode.wl_flag) + ": " + bad + " (only " + mode.wl_kind + " can be resumed here; a BSGS recovery file is not supported in kangaroo mode)");
        // the settings: what the command line names must be what the file was made with, and the rest is taken from the file
        if (mode.fingerprint(*this, wf.h) != wf.h.fingerprint || (c.dp >= 0 && (uint32_t)c.dp != wf.h.dp) || (c.kn && c.kn != wf.h.herd) || (c.seed_given && c.seed != wf.h.seed) ||
            (!dl.empty() && dl.size() != wf.h.engines) || !wf.h.engines || !wf.h.herd || !wf.h.per_thread || wf.h.herd % (64ull * wf.h.per_thread))
            die("Recovery file was made with other settings");
        elapsed_before = wf.h.elapsed;
        if (c.verify) check_table = wf.table;                          // (the mode restores its table from wf.table and lets go of it)
    }
    if (!mode.before_devices(*this)) { go = false; return; }
    if (mode.verify_skip) std::vector<uint8_t>().swap(check_table);

    int ngpu = 0;
    CK(bsgs_dev_count(&ngpu));
    if (ngpu <= 0) die("No GPU found");
    if (dl.empty()) for (int i = 0; i < ngpu; i++) gpus.push_back(i);
    else for (const std::string &tok : dl) gpus.push_back(atoi(tok.c_str()));
    if (resume && gpus.size() != wf.h.engines) die("Recovery file was made with other settings");
    int cus = 256;
    { bsgs_dev *d = nullptr; CK(bsgs_dev_open(gpus[0], &d)); bsgs_dev_cu_count(d, &cus); bsgs_dev_close(d); }
    mode.engines_known(*this);
    // defaults from W (plan_herd); then the expected total, the launch length and the record buffer, which depend on it
    pl = plan_herd(sqrtW, (uint32_t)gpus.size(), cus, resume ? (int)wf.h.dp : mode.dp_fixed >= 0 ? mode.dp_fixed : c.dp, c.kn);
    if (resume) { pl.kn = wf.h.herd; pl.G = wf.h.per_thread; }        // the plan of the run that saved, not this GPU's
    if (pl.kn > (1ull << 26)) die("-kn: at most 2^26 kangaroos per engine");
    mode.planned(*this);
    const double Nk = (double)pl.kn * pl.engines;
    plan_launch(pl, sqrtW, mode.expected, mode.min_launch, mode.bound_launch, mode.dp_free && !resume);
    uint64_t seed = c.seed;
    if (resume) seed = wf.h.seed;
    else if (!c.seed_given) { std::random_device rd; seed = ((uint64_t)rd() << 32) ^ rd(); }
    printf("Kangaroo: %u engine(s) x %llu kangaroos (%u per thread), -dp %u, %u steps per launch, -kseed 0x%llx\n", pl.engines, (unsigned long long)pl.kn, pl.G, pl.dp, pl.S,
           (unsigned long long)seed);
    wh.version = mode.version; wh.engines = pl.engines; wh.dp = pl.dp; wh.per_thread = pl.G; wh.herd = pl.kn; wh.seed = seed;
    wh.fingerprint = mode.fingerprint(*this, wh);

    rng = seed;
    const double mean = mode.mean_jump > 0.0 ? mode.mean_jump : std::max(1.0, std::min(std::ldexp(1.0, 62), mode.jumpscale * Nk * sqrtW / 4.0));
    js.resize(mode.jumps);
    jxy.resize(64 * (size_t)mode.jumps);
    for (uint32_t j = 0; j < mode.jumps; j++) {
        const uint64_t span = (uint64_t)(2.0 * mean) > 1 ? (uint64_t)(2.0 * mean) - 1 : 1;
        js[j] = mode.jump_scalars ? mode.jump_scalars[j] : 1 + splitmix64(rng) % span;
        hs::affine_to_le(hs::point_mul(hs::G, hs::fe_from_u64(js[j])), &jxy[64 * (size_t)j], &jxy[64 * (size_t)j + 32]);
    }
    herds.resize(pl.engines);
    if (resume) {
        rng = wf.h.rng;
        for (uint32_t e = 0; e < pl.engines; e++) {
            herds[e].resize(pl.kn);
            memcpy(herds[e].data(), wf.herds[e].data(), pl.kn * sizeof(bsgs_kangaroo_state));
            std::vector<uint8_t>().swap(wf.herds[e]);
        }
    }
}

Shared::Shared(const Prologue &p) : rng(p.rng), reseed(p.pl.engines), engine_records(p.pl.engines, 0), saved(p.pl.engines)
{
    for (uint32_t e = 0; e < p.pl.engines; e++) { reseed_m.emplace_back(new std::mutex); inbox.emplace_back(new Inbox); }
    routed.reset(new std::atomic<uint64_t>[p.pl.engines]);
    for (uint32_t e = 0; e < p.pl.engines; e++) routed[e] = 0;
    if (p.resume) {
        steps = p.wf.h.steps; dps = p.wf.h.dps; dropped = p.wf.h.dropped;
        reseed = p.wf.reseed;
    }
}

namespace {
volatile sig_atomic_t signalled = 0;
void on_signal(int) { signalled = 1; }

// TEST BUILD ONLY (bsgs_mi355x_test, -DBSGS_TEST_HOOKS; the shipped host has no such hook): BSGS_TEST_CORRUPT_KANGAROO=i flips bit 0 of the offset of kangaroo
// i of engine 0 after the first launch -- the run must then stop at the verification before its next save
void test_corrupt_kangaroo(bsgs_dev *dev, uint64_t kn)
{
#ifdef BSGS_TEST_HOOKS
    const char *v = getenv("BSGS_TEST_CORRUPT_KANGAROO");
    if (!v) return;
    const uint32_t i = (uint32_t)strtoul(v, nullptr, 10);
    if (i >= kn) return;
    fprintf(stderr, "BSGS_TEST_CORRUPT_KANGAROO=%s: TEST HOOK -- bit 0 of the offset of kangaroo %u of engine 0 is flipped (this run must stop before it saves)\n", v, i);
    bsgs_kangaroo_state s;
    CK(bsgs_kangaroo_download(dev, i, 1, &s));
    s.d[0] ^= 1u;
    CK(bsgs_kangaroo_upload_list(dev, &i, 1, &s));
#else
    (void)dev; (void)kn;
#endif
}

// every kangaroo of the device's herd against sigma*Q + d*G (bsgs_kangaroo_verify; the herd is only read): 0 all stand at their offsets, 1 *at is the
// lowest-numbered one found that does not, -1 the call failed
int herd_check(bsgs_dev *dev, const Mode &mode, uint64_t kn, uint32_t *at)
{
    uint32_t n_bad = 0;
    if (bsgs_kangaroo_verify(dev, mode.verify_q, 0, (uint32_t)kn, &n_bad, at, 1) != BSGS_OK) return -1;
    return n_bad ? 1 : 0;
}
// -wl: the file's table entries through bsgs_kangaroo_verify_points, 2^20 at a time: as herd_check, *at the entry's position in the file
int table_check(bsgs_dev *dev, const Mode &mode, const std::vector<uint8_t> &entries, uint64_t *at)
{
    const uint64_t D = entries.size() / 32, step = 1u << 20;
    std::vector<uint8_t> d(16 * std::min(D, step));
    std::vector<uint32_t> fl(std::min(D, step));
    std::vector<uint64_t> x(std::min(D, step));
    for (uint64_t pos = 0; pos < D; pos += step) {
        const uint32_t m = (uint32_t)std::min(D - pos, step);
        for (uint32_t k = 0; k < m; k++) {                             // an entry: low 64 bits of x, d, kangaroo, type or owner
            const uint8_t *en = &entries[32 * (pos + k)];
            uint32_t word;
            memcpy(&x[k], en, 8); memcpy(&d[16 * (size_t)k], en + 8, 16); memcpy(&word, en + 28, 4);
            fl[k] = mode.entry_flags(word);
        }
        uint32_t n_bad = 0, first = 0;
        if (bsgs_kangaroo_verify_points(dev, mode.verify_q, m, d.data(), fl.data(), x.data(), &n_bad, &first, 1) != BSGS_OK) return -1;
        if (n_bad) { *at = pos + first; return 1; }
    }
    return 0;
}

// one engine: all calls for a device from the thread that opened it
void engine(uint32_t e, const KangConfig &c, Prologue &p, Shared &sh, Mode &mode)
{
    const uint64_t kn = p.pl.kn;
    const bool check = c.verify && !mode.verify_skip;                  // herds and the saved table vouch for themselves ("verification")
    bsgs_dev *dev = nullptr;
    auto end_with = [&](const std::string &msg) { std::lock_guard<std::mutex> lk(sh.err_m); if (sh.err.empty()) sh.err = msg; sh.failed = true; sh.stop = true; };
    auto bad = [&](const char *what) { end_with(std::string(what) + ": " + bsgs_last_error()); };
    auto verified = [&](const char *lead, const std::string &what, Clock::time_point ts) {
        std::lock_guard<std::mutex> lk(sh.err_m);
        printf("%s[verify] %s %.3fs\n", lead, what.c_str(), since(ts));
    };
    const char *failed = nullptr;
    if (bsgs_dev_open(p.gpus[e], &dev) != BSGS_OK) failed = "bsgs_dev_open";
    else if ((failed = mode.setup_engine(dev, e)) != nullptr) {}
    else if (!p.herds[e].empty()) {
        if (bsgs_kangaroo_upload(dev, 0, (uint32_t)kn, p.herds[e].data()) != BSGS_OK) failed = "bsgs_kangaroo_upload";
        std::vector<bsgs_kangaroo_state>().swap(p.herds[e]);
    } else {
        const auto ts = Clock::now();
        if ((failed = mode.seed(dev, e, {}, sh)) == nullptr) {
            std::lock_guard<std::mutex> lk(sh.err_m);
            printf("[startup] %-44s %.3fs\n", (mode.herd_label + std::to_string(e)).c_str(), since(ts));
        }
    }
    bool ok = failed == nullptr;                                       // the device holds a herd that can walk
    if (!ok) bad(failed);
    // -wl: what was uploaded is checked before anything walks -- every kangaroo of every engine, and on the first engine's device every entry of the
    // saved table; a mismatch ends the run with the file as it is
    if (p.resume && check) {
        if (ok) {
            auto ts = Clock::now();
            uint32_t at = 0;
            const int rc = herd_check(dev, mode, kn, &at);
            if (rc < 0) bad("bsgs_kangaroo_verify");
            else if (rc) end_with("Recovery file is damaged: kangaroo " + std::to_string(at) + " of engine " + std::to_string(e) + " does not stand at its offset");
            else verified("", "herd " + std::to_string(e) + ": " + std::to_string(kn) + " kangaroos at their offsets", ts);
            ok = rc == 0;
            if (ok && e == 0) {
                ts = Clock::now();
                uint64_t entry = 0;
                const int rt = table_check(dev, mode, p.check_table, &entry);
                if (rt < 0) bad("bsgs_kangaroo_verify_points");
                else if (rt) end_with("Recovery file is damaged: table entry " + std::to_string(entry) + " does not match its offset");
                else verified("", "table: " + std::to_string(p.check_table.size() / 32) + " entries", ts);
                ok = rt == 0;
                std::vector<uint8_t>().swap(p.check_table);
            }
        }
        sh.checked++;
        while (sh.checked.load() < p.pl.engines && !sh.stop.load()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    if (p.resume && ok && !sh.failed.load()) { const std::string msg = mode.resumed(dev, e, sh); if (!msg.empty()) { end_with(msg); ok = false; } }
    bool first_launch = true;
    std::vector<bsgs_kangaroo_record> recs(ok ? p.pl.cap : 0);
    while (ok) {
        if (!sh.stop.load()) {
            std::vector<uint32_t> rs;
            { std::lock_guard<std::mutex> lk(*sh.reseed_m[e]); rs.swap(sh.reseed[e]); }
            if (!rs.empty()) {
                std::sort(rs.begin(), rs.end());
                rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
                if ((failed = mode.seed(dev, e, rs, sh)) != nullptr) { bad(failed); break; }
            }
        }
        if (!sh.stop.load() && mode.sharded) { const std::string msg = mode.drain(dev, e, sh); if (!msg.empty()) { end_with(msg); break; } }
        if (!sh.stop.load()) {
            uint32_t n = 0;
            uint64_t dropped = 0;
            if (mode.launch(dev, e, p.pl.S, recs.data(), p.pl.cap, &n, &dropped, sh) != BSGS_OK) { bad("bsgs_kangaroo_run"); break; }
            const uint64_t total = (sh.steps += kn * p.pl.S);
            sh.dropped += dropped;
            { std::lock_guard<std::mutex> lk(sh.q_m); sh.queue.emplace_back(e, std::vector<bsgs_kangaroo_record>(recs.begin(), recs.begin() + n)); }
            sh.q_cv.notify_one();
            if (c.ksteps && total >= c.ksteps) sh.stop = true;
            if (first_launch && e == 0) test_corrupt_kangaroo(dev, kn);  // (test build only)
            first_launch = false;
        }
        // the herd as it stands leaves the device between two launches when a save is requested, and at the end when the search is not done (the last save)
        const bool stopped = sh.stop.load();
        bool want = sh.save_req.load();
        if (stopped) { std::lock_guard<std::mutex> lt(sh.tab_m); want = mode.saves && !mode.done(); }
        // -kdpshard: a routed record that reached no table at a save would be lost for good (a kangaroo records a point once).  So no engine drains its
        // last inbox before every living engine has made its last launch and pushed what it routed; then each drains, and only then checks, downloads and
        // fetches.  The barrier counts the living engines and gives way to a failure and to a found key (nothing is saved then).  A save round that is
        // given up while an engine waits in it (a signal withdraws the request, a stop comes) lets that engine go on: it meets the others in the stop round
        if (want && mode.sharded && !sh.failed.load()) {
            uint64_t round;
            { std::lock_guard<std::mutex> lk(sh.save_m); round = sh.barrier.arrive(stopped); }
            SaveBarrier::State st = SaveBarrier::WAIT;
            for (;;) {
                { std::lock_guard<std::mutex> lk(sh.save_m); st = sh.barrier.state(stopped, round, sh.running, sh.save_req.load(), sh.stop.load()); }
                if (st != SaveBarrier::WAIT || sh.failed.load()) break;
                { std::lock_guard<std::mutex> lt(sh.tab_m); if (mode.done()) break; }
                std::this_thread::sleep_for(std::chrono::milliseconds(1));
            }
            if (st == SaveBarrier::GIVEN_UP) continue;
            const bool all = st == SaveBarrier::ALL;
            if (all) { const std::string msg = mode.drain(dev, e, sh); if (!msg.empty()) { end_with(msg); break; } }
        }
        if (want && check && !sh.failed.load()) {                      // before every save: a herd that went wrong never replaces a good file
            const auto ts = Clock::now();
            uint32_t at = 0;
            const int rc = herd_check(dev, mode, kn, &at);
            if (rc < 0) { bad("bsgs_kangaroo_verify"); break; }
            if (rc) { end_with("herd of engine " + std::to_string(e) + " failed verification at kangaroo " + std::to_string(at) + ": kangaroo.work left as it was"); break; }
            if (stopped) verified("\n", "herd " + std::to_string(e) + ": " + std::to_string(kn) + " kangaroos at their offsets", ts);      // (the -wt saves stay silent)
        }
        if (want) {
            sh.saved[e].resize(kn);
            if (bsgs_kangaroo_download(dev, 0, (uint32_t)kn, sh.saved[e].data()) != BSGS_OK) { bad("bsgs_kangaroo_download"); sh.saved[e].clear(); break; }
            const std::string msg = mode.fetch(dev, e, sh);
            if (!msg.empty()) { end_with(msg); sh.saved[e].clear(); break; }
        }
        if (stopped) break;
        if (want) {                                                    // parked: wait for the file
            std::unique_lock<std::mutex> lk(sh.save_m);
            sh.parked++;
            sh.save_cv.notify_all();
            while (sh.save_req.load() && !sh.stop.load()) sh.save_cv.wait_for(lk, std::chrono::milliseconds(100));
            sh.parked--;
        }
    }
    if (ok && !sh.failed.load()) { const std::string msg = mode.ending(dev, e, sh); if (!msg.empty()) end_with(msg); }
    if (dev) bsgs_dev_close(dev);
    std::lock_guard<std::mutex> lk(sh.save_m);
    sh.running--;
    sh.save_cv.notify_all();
}
}  // namespace

Outcome kang::run(const KangConfig &c, Prologue &p, Shared &sh, Mode &mode)
{
    const Plan &pl = p.pl;
    // the work file from the state as it stands: callers make sure that no engine walks and the collector's queue is empty
    // false: refused -- under -kdpshard a state with a routed record in an inbox is not a cut of the search
    auto write_state = [&]() -> bool {
        if (mode.sharded && !sh.inboxes_empty()) { fprintf(stderr, "\nWARNING: save refused, routed records wait in an inbox: %s left as it was\n", p.work_path.c_str()); return false; }
        std::lock_guard<std::mutex> lt(sh.tab_m);
        WorkHeader h = p.wh;
        h.rng = sh.rng; h.steps = sh.steps.load(); h.dps = sh.dps.load(); h.dropped = sh.dropped.load();
        h.elapsed = p.elapsed_before + since(p.t0);
        std::vector<uint8_t> entries;
        const WorkKeys *keys = mode.save(h, entries);
        std::vector<const std::vector<bsgs_kangaroo_state> *> hp;
        std::vector<std::vector<uint32_t>> rs(pl.engines);
        for (uint32_t e = 0; e < pl.engines; e++) { hp.push_back(&sh.saved[e]); std::lock_guard<std::mutex> lk(*sh.reseed_m[e]); rs[e] = sh.reseed[e]; }
        if (!write_work(p.work_path, p.work_tmp, h, entries, hp, rs, keys)) fprintf(stderr, "WARNING: cannot write %s\n", p.work_path.c_str());
        return true;
    };
    // the collector: every engine's records into the mode's one table
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
            std::lock_guard<std::mutex> lt(sh.tab_m);
            if (mode.done()) continue;
            sh.engine_records[b.first] += b.second.size();
            for (const bsgs_kangaroo_record &r : b.second) {
                if (mode.counts_records && !(r.flags & BSGS_KANGAROO_DEAD)) sh.dps++;
                if (!mode.record(b.first, r, sh)) break;
            }
        }
    });
    signalled = 0;
    signal(SIGINT, on_signal);
    signal(SIGTERM, on_signal);
    // (engines are not started if the search ended while the mode prepared it: a start at infinity in the host's seeding is the key)
    std::vector<std::thread> th;
    if (c.verify && mode.verify_skip && !sh.stop.load()) printf("[verify] skipped: %s\n", mode.verify_skip);
    sh.running = sh.stop.load() ? 0 : pl.engines;
    if (!sh.stop.load()) for (uint32_t e = 0; e < pl.engines; e++) th.emplace_back(engine, e, std::cref(c), std::ref(p), std::ref(sh), std::ref(mode));
    auto last_t = Clock::now(), last_save = Clock::now();
    uint64_t last_steps = sh.steps.load();
    bool gave_up = false, interrupted = false;
    while (!sh.stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        const auto now = Clock::now();
        if (signalled) { interrupted = true; sh.stop = true; sh.save_cv.notify_all(); break; }
        {
            std::lock_guard<std::mutex> lt(sh.tab_m);
            if (std::chrono::duration<double>(now - last_t).count() >= 2.0) {
                const uint64_t st = sh.steps.load();
                mode.status((st - last_steps) / std::chrono::duration<double>(now - last_t).count(), st, sh.dps.load());
                fflush(stdout);
                last_steps = st; last_t = now;
            }
            if (mode.give_up(sh.steps.load())) { gave_up = true; sh.stop = true; }
        }
        if (mode.saves && !sh.stop.load() && std::chrono::duration<double>(now - last_save).count() >= (double)c.wt) {
            // -wt: every engine parks between two launches with its herd downloaded and its last records queued; the collector empties the queue; then
            // table, counters, stream, herds and re-seed lists belong to one moment of the search
            const auto ts = Clock::now();
            { std::lock_guard<std::mutex> lk(sh.save_m); sh.barrier.open(); }
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
            if (all_parked && !sh.stop.load() && write_state()) printf("\n[save] %s in %.2fs\n", p.work_path.c_str(), since(ts));
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
    sh.ended = Clock::now();
    signal(SIGINT, SIG_DFL);
    signal(SIGTERM, SIG_DFL);
    if (!sh.err.empty()) die(sh.err);
    if (mode.done()) { if (mode.saves) remove(p.work_path.c_str()); return DONE; }     // a stale file never outlives its job
    bool have = true;
    for (uint32_t e = 0; e < pl.engines; e++) have = have && sh.saved[e].size() == pl.kn;
    if (have && mode.saves && !write_state()) die("-kangaroo -kdpshard: the last save was refused, routed records never reached their table");      // engines joined, queue drained: the state is final
    return gave_up ? GAVE_UP : interrupted ? INTERRUPTED : c.ksteps && sh.steps.load() >= c.ksteps ? BUDGET : ENDED;
}
