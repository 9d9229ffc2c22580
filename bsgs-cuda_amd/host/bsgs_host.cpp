// bsgs_host.cpp -- C++ host of the MI355X BSGS solver: the reference's `bsgscudaHT_1_9_6file.exe` command line,
// file formats and outputs on top of libbsgs_hip.so's native API (include/bsgs_hip.h).
//
// Mirrors (file:line of /root/reference/1_9_7File.pb): flag parser getprogparam 875-1042 and the checks
// 4412-4472, 4616-4630; start-up constants 4689-4712, 4759-4765; table files Save_HTpacked 3645-3759 /
// Save_Load_Giants 1905-2058 (names and byte layouts kept; built on the GPU when missing); per-GPU driver
// thread cuda() 2095-2553; tile dispenser GetJob 2077-2092; hit resolver checkerThread 3933-4296; checkpoint
// saveCurentCNT 3897-3931 and its restore 4634-4686; per-pubkey loop, progress line and win.txt 4995-5168.
// PureBasic is not available in this image, so the host is C++; INTEGRATION.md shows the PureBasic bindings.
//
// Build: make -C bsgs-cuda_amd host   ->  build/bsgs_mi355x
#include "host.h"

namespace {
using Clock = std::chrono::steady_clock;
double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }
// "[startup] <stage> <seconds>" lines: where the time before the first tile goes (bench.py's cold_time_to_solve_s reads them)
struct Stages {
    Clock::time_point t = Clock::now();
    void operator()(const char *what) { const auto n = Clock::now(); printf("[startup] %-44s %.3fs\n", what, std::chrono::duration<double>(n - t).count()); t = n; }
};
std::vector<int> find_gpus(const Config &c, bool cpu_only)
{
    std::vector<int> gpus;
    if (cpu_only) return gpus;                                        // the reference's CPU-only generator: no GPU is looked for, none is needed
    int ngpu = 0;
    CK(bsgs_dev_count(&ngpu));
    if (ngpu <= 0) die("No GPU found");
    if (c.devices.empty()) for (int i = 0; i < ngpu; i++) gpus.push_back(i);
    else { std::stringstream ss(c.devices); std::string tok; while (std::getline(ss, tok, ',')) gpus.push_back(atoi(tok.c_str())); }
    return gpus;
}
int bit_length(const Scalar &v) { for (int l = 3; l >= 0; l--) if (v.l[l]) return 64 * l + 64 - __builtin_clzll(v.l[l]); return 0; }

// ---- range (1_9_7File.pb:4887-4943), Tune for it, constants (1_9_7File.pb:4689-4712, 4759-4765)
void setup_range(Run &R, const std::vector<int> &gpus, bool cpu_only)
{
    Config &c = R.cfg;
    if (!c.ext && !c.w_auto) { const std::string m = table_limits(c.w, c.htsz_arg, stdin); if (!m.empty()) die(m == " " ? "" : m); }
    if (!hs::fe_from_hex(R.start, c.pk) || hs::fe_is_zero(R.start)) die("Start range can`t be zero");
    printf("START RANGE= %s\n", hs::fe_to_hex(R.start).c_str());
    // the end of range is ALWAYS in force: privkeyend defaults to 1ffffffffffffffff and endrangeflag is set whenever it is
    // non-zero (1_9_7File.pb:210, 4897-4936); a key outside [pk, pke] ends with "Reached end of space"
    Scalar e;
    if (!hs::fe_from_hex(e, c.pke)) die("Invalid range (-pkend) length!!!");
    if (!hs::fe_is_zero(e)) {
        if (hs::fe_cmp(e, R.start) <= 0) die(c.pke_given ? "End range should be more than begin range!" : "End range must be more then start range");
        R.width = hs::sc_sub(e, R.start); R.end_range = true;
        printf("  END RANGE= %s\nWIDTH RANGE= %s = 2^%d\n", hs::fe_to_hex(e).c_str(), hs::fe_to_hex(R.width).c_str(), bit_length(R.width));
    }
    R.start_neg = hs::affine_neg(hs::point_mul(hs::G, R.start));
    const int range_bits = R.end_range ? bit_length(R.width) : 0;
    if (range_bits && !cpu_only) {
        // Tune for THIS range (the reference's Tune, 1_9_7File.pb:324-431, knows the GPU only): the table that minimises build + worst-case search
        bsgs_dev *dt = nullptr;
        uint64_t fr = 0, tot = 0;
        if (bsgs_dev_open(gpus[0], &dt) == BSGS_OK) { bsgs_dev_meminfo(dt, &fr, &tot); bsgs_dev_close(dt); }
        const TunePlan pl = tune_plan(fr, (double)range_bits, (int)gpus.size(), (uint64_t)c.t * c.b * c.p);
        printf("Tune for this range (2^%d keys, %zu GPU engine(s)): %s  -> table %.2fs + search at most %.2fs\n", range_bits, gpus.size(), plan_flags(pl).c_str(), pl.build_s, pl.search_s);
        if (c.w_auto) {
            c.w = pl.w; c.ext = pl.ext; c.htsz_arg = pl.htsz_arg;
            c.htsz = pl.htsz_arg <= 31 ? pl.htsz_arg : (uint32_t)std::floor(std::log2((double)pl.htsz_arg));
            printf("-w auto: Items number set to 2^%.2f=%llu, %s\n", pl.w_log2, (unsigned long long)c.w, pl.ext ? "extended table in GPU memory (no HT files)" : "reference-format HT files");
        }
    } else if (c.w_auto) die("-w auto needs a range (-pk / -pke)");
    derive_constants(R);
    printf("GiantSUBvalue:%s\nGiantSUBpubkey: %s\n", hs::fe_to_hex(hs::sc_from_u128((hs::u128)c.w * 2)).c_str(), hs::compress_pubkey(R.addpubg).c_str());
    printf("Gstep: %s\n", hs::fe_to_hex(R.gstep).c_str());
}

// ---- table files (Save_HTpacked 3645-3759, Save_Load_Giants 1905-2058): load, or build on the GPU and save.  Files that were just generated are written by
// background threads while the start-up goes on (upload, bucket lines, scratch): the buffers they read stay alive until flush_writers() -- before the staging
// copies are released, and before any return
struct TableFiles {
    HostBuf htgpu, g2;
    struct Write { std::string path; const uint8_t *p; uint64_t n; };
    std::vector<Write> pending;                                       // started once the engines hold their tables: 15 GB going into the page cache next to the upload of the same
                                                                      // buffers slowed that upload from 0.25 s to 2 s (profiles/r07t_*)
    std::vector<std::thread> writers;
    std::string saved_msg;
    void start_writers() { for (const Write &w : pending) writers.emplace_back(write_file, w.path, w.p, w.n); pending.clear(); }
    void flush_writers() { start_writers(); for (auto &w : writers) w.join(); writers.clear(); if (!saved_msg.empty()) { fputs(saved_msg.c_str(), stdout); saved_msg.clear(); } }
};
void load_or_build_files(Run &R, TableFiles &F, const std::vector<int> &gpus)
{
    const Config &c = R.cfg;
    const uint64_t ht_items = 1ull << c.htsz;
    const std::string gxhex = hs::fe_to_hex(hs::G.x);
    const std::string stem = c.dir + "/" + gxhex + "_" + std::to_string(c.w) + "_" + std::to_string(ht_items);
    const std::string f_gpu = stem + "_htGPUv0.BIN", f_cpu = stem + "_htCPUv0.BIN";
    const std::string f_g2 = c.dir + "/" + std::to_string(c.t) + "_" + std::to_string(c.b) + "_" + std::to_string(c.p) + "_" + std::to_string(c.w) + "_g2.BIN";
    const uint64_t gpu_bytes = 4 * (ht_items + 1) + 4 * c.w, cpu_bytes = 4 * (ht_items + 1) + 8 * c.w, g2_bytes = 64 * R.maxnonce;
    Tables &tables = R.tab;
    bsgs_dev *d0 = nullptr;
    auto dev0 = [&]() { if (!d0) CK(bsgs_dev_open(gpus[0], &d0)); return d0; };
    if (c.ext) printf("Extended table: %llu items, built in GPU memory at start-up (no HT files)\n", (unsigned long long)c.w);
    else if (c.file_search && file_has_size(f_cpu, cpu_bytes) && read_file(f_gpu, F.htgpu, gpu_bytes) && (tables.htcpu_fd = open(f_cpu.c_str(), O_RDONLY)) >= 0)
        printf("Both HT files exist\nhtCPU is searched in its file (%.1f GB not loaded)\n", cpu_bytes / 1e9);
    else if (read_file(f_gpu, F.htgpu, gpu_bytes) && read_file(f_cpu, tables.htcpu, cpu_bytes)) printf("Both HT files exist\n");
    else {
        printf("Generate HT with %llu items on the %s\n", (unsigned long long)c.w, c.cpugen ? "host CPU" : "GPU");
        const auto t0 = Clock::now();
        F.htgpu.resize(gpu_bytes); tables.htcpu.resize(cpu_bytes);
        if (c.cpugen) cpu_build_tables(c.w, c.htsz, F.htgpu.data(), tables.htcpu.data());
        else CK(bsgs_build_baby_tables(dev0(), c.w, c.htsz, F.htgpu.data(), tables.htcpu.data(), BSGS_NO_INSTALL));
        F.pending.push_back({f_cpu, tables.htcpu.data(), cpu_bytes});
        F.pending.push_back({f_gpu, F.htgpu.data(), gpu_bytes});
        printf("Done in %.1fs\n", since(t0));
    }
    if (read_file(f_g2, F.g2, g2_bytes)) printf("Load BIN file:%s\n", f_g2.c_str());
    else {
        printf("Generate Giants Buffer: %llu items\n", (unsigned long long)R.maxnonce);
        F.g2.resize(g2_bytes);
        if (c.cpugen) cpu_build_g2(R.addpubg, c.t, c.b, c.p, F.g2.data());
        else {
            uint8_t axy[64];
            hs::affine_to_le(R.addpubg, axy, axy + 32);
            CK(bsgs_generate_g2(dev0(), axy, c.t, c.b, c.p));
            CK(bsgs_download_g2(dev0(), F.g2.data(), g2_bytes));
        }
        F.pending.push_back({f_g2, F.g2.data(), g2_bytes});
        F.saved_msg = "Save BIN file:" + f_g2 + "\n";                 // printed once the file IS on disk (flush_writers)
    }
    if (d0) bsgs_dev_close(d0);
}

// ---- how long a job is, in tiles (width / gstep): a job that is only a launch or two long (BASELINE config 4: a 64-bit range at -w 30 is 129 tiles) is dealt in small
// batches that wait for their checker -- the reference, one tile per launch, stops at the hit (1_9_7File.pb:2442-2523); a full launch would always run to its end --,
// its engines take scratch for such batches only, and with several keys to search two jobs run side by side (lanes).  Returns the number of lanes.
size_t plan_lanes(Run &R, size_t ngpus, size_t todo)
{
    const Config &c = R.cfg;
    auto as_double = [](const Scalar &v) { double r = 0.0; for (int l = 3; l >= 0; l--) r = r * 18446744073709551616.0 + (double)v.l[l]; return r; };
    const double job_tiles = R.end_range ? as_double(R.width) / as_double(R.gstep) + 1.0 : 0.0;
    const double tpl_est = std::min(1024.0, std::max(48.0, (double)(192ull << 24) / (double)R.maxnonce));       // the engine's launch size at this geometry, memory permitting
    const bool short_job = job_tiles > 0.0 && job_tiles < 4.0 * tpl_est * (double)ngpus;
    size_t lanes = 1;
    if (c.lanes > 0) lanes = (size_t)c.lanes;
    else if (short_job && todo >= 4 && !c.ext && c.joblog.empty()) lanes = 2;
    lanes = std::max<size_t>(1, std::min(lanes, todo));
    if (short_job) {
        // about six batches per GPU and job (fourteen with two lanes: the other lane's launch hides this one's boundaries), not below 16 (8) tiles: the narrow batchings keep
        // small launches at 35-38 G, and with the key anywhere in the range 0.55-0.6 of the tiles are searched on average instead of all of them
        const double per_job = getenv("BSGS_SHORT_JOB_BATCHES") ? std::max(1.0, atof(getenv("BSGS_SHORT_JOB_BATCHES"))) : (lanes > 1 ? 14.0 : 6.0);      // (the variable: A-B runs; 1000 keys of config 4: 10 -> 64-66 s, 14 -> 61.8 s, profiles/r07g_*)
        R.batch_hint = (uint32_t)std::min(tpl_est, std::max(lanes > 1 ? 8.0 : 16.0, std::ceil(job_tiles / (per_job * (double)ngpus))));
        printf("Short jobs (%.0f tiles each): dealt in batches of %u tiles%s\n", job_tiles, R.batch_hint, lanes > 1 ? ", two public keys searched side by side (an engine each per GPU)" : "");
    }
    return lanes;
}

// ---- the engines: one per GPU and lane (`gpus` is repeated once per lane).  The engines of lane 0 are loaded (and, several GPUs, compared); the engines of the
// other lanes are TWINS of theirs on the same GPU: they probe the same table in place (bsgs_share_tables) -- no second 21 GiB to place, clear and copy at -w 30 --
// with giants and chain scratch of their own
std::vector<bsgs_dev *> start_engines(const Run &R, std::vector<int> &gpus, size_t lanes, const TableFiles &F)
{
    const Config &c = R.cfg;
    if (lanes > 1) { const std::vector<int> base = gpus; for (size_t l = 1; l < lanes; l++) gpus.insert(gpus.end(), base.begin(), base.end()); }
    std::vector<bsgs_dev *> devs(gpus.size(), nullptr);
    for (size_t gi = 0; gi < gpus.size(); gi++) devs[gi] = open_dev(gpus[gi]);
    if (R.batch_hint) for (bsgs_dev *d : devs) CK(bsgs_set_tiles_per_launch(d, R.batch_hint));     // scratch (and its placement) for the batches this run will launch, not for 192 tiles
    const size_t primaries = gpus.size() / lanes;
    const std::vector<int> gpus0(gpus.begin(), gpus.begin() + (long)primaries);
    const std::vector<bsgs_dev *> devs0(devs.begin(), devs.begin() + (long)primaries);
    load_engines(R, gpus0, devs0, F.htgpu, F.g2);
    test_corrupt_engine(devs0);                                       // (test build only)
    if (devs0.size() > 1 && c.verify_replicas) verify_replicas(gpus0, devs0);
    if (c.verify_replicas) verify_tables(R, gpus0, devs0);            // the reference's checkHT / checkHTpackFile / checkGiantArr before it searches (1_9_7File.pb:3717, 3731, 4859, 1941)
    if (lanes > 1) {
        const auto t0 = Clock::now();
        for (size_t gi = primaries; gi < devs.size(); gi++) { CK(bsgs_share_tables(devs[gi % primaries], devs[gi])); CK(bsgs_prepare(devs[gi])); print_placement(gpus[gi], gi, devs[gi]); }
        printf("[startup] %-44s %.3fs\n", "twin engines of the other lanes (shared tables)", since(t0));
    }
    if (c.ref_quirks) { for (bsgs_dev *d : devs) CK(bsgs_set_flags(d, BSGS_FLAG_REFERENCE_QUIRKS)); printf("Reference-quirk mode: NEGMODP borrow bug reproduced\n"); }
    return devs;
}
// a job's console lines: printed as they happen (one lane), or handed to the JobList to be printed when the job's turn in the list comes (several)
struct JobText {
    bool live;
    std::string text;
    __attribute__((format(printf, 2, 3))) void say(const char *fmt, ...)
    {
        char buf[1024];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        if (live) { fputs(buf, stdout); fflush(stdout); } else text += buf;
    }
};
struct LaneEngines { size_t lane; std::vector<int> gpus; std::vector<bsgs_dev *> devs; };

// once per run: the launch time depends on which physical memory the driver handed out for the chain scratch and the
// bucket lines; try a few placements on every GPU (in parallel) and keep the fastest
void tune_placement(const LaneEngines &E, JobText &o)
{
    const size_t n = E.devs.size();
    std::vector<std::array<float, 7>> res(n);
    std::vector<int> rcs(n, 0);
    std::vector<std::string> why(n);
    std::vector<std::thread> tt;
    for (size_t gi = 0; gi < n; gi++) tt.emplace_back([&, gi]() {
        uint32_t kept[2] = {0, 0};
        rcs[gi] = bsgs_tune_placement(E.devs[gi], 3, res[gi].data(), kept, &res[gi][6]);
        if (rcs[gi]) why[gi] = bsgs_last_error();                   // the error text is per thread
    });
    for (auto &t : tt) t.join();
    for (size_t gi = 0; gi < n; gi++) {
        if (rcs[gi]) { o.say("GPU #%d: placement tuning skipped (%s)\n", E.gpus[gi], why[gi].c_str()); continue; }
        o.say("GPU #%d: placement tuned, %.1f -> %.1f ms per launch\n", E.gpus[gi], res[gi][0], res[gi][6]);
    }
}
// a seeded job searched to its end on the engines of its lane: the checker threads, a driver thread per engine, the progress line and the -wt checkpoint
void search(Job &J, const LaneEngines &E, JobList &jobs)
{
    const Config &c = J.run.cfg;
    const int G = (int)E.devs.size();
    const unsigned nchk = c.ext ? std::max(2u, std::min(16u, std::thread::hardware_concurrency() / 4)) : 1u;   // false positives cost a small BSGS each
    std::vector<std::thread> chk, th;
    for (unsigned q = 0; q < nchk; q++) chk.emplace_back(checker_thread, &J);
    for (int gi = 0; gi < G; gi++) th.emplace_back(gpu_thread, &J, E.gpus[gi], gi, E.devs[gi]);
    auto last_save = Clock::now(), last_t = last_save;
    uint64_t last_steps = 0;
    while (J.gpus_finished.load() < G) {
        { std::unique_lock<std::mutex> lk(J.done_mutex); J.done_cv.wait_for(lk, std::chrono::milliseconds(200), [&] { return J.gpus_finished.load() >= G; }); }
        const auto now = Clock::now();
        if (jobs.live() && std::chrono::duration<double>(now - last_t).count() >= 2.0) {       // progress line 5119-5142
            const uint64_t st = J.steps_done.load();
            const double rate = (st - last_steps) / std::chrono::duration<double>(now - last_t).count();
            Scalar cnt; { std::lock_guard<std::mutex> lk(J.job_mutex); cnt = J.glob_key; }
            printf("\rCnt:%s [%d] = %.0f MKeys/s x2^%.2f=2^%.2f   ", hs::fe_to_hex(cnt).c_str() + 40, G, rate / 1048576.0,
                   std::log2(2.0 * c.w), rate > 0 ? std::log2(rate * 2.0 * c.w) : 0.0);
            fflush(stdout);
            last_steps = st; last_t = now;
        }
        if (std::chrono::duration<double>(now - last_save).count() >= c.wt || J.joblog) { jobs.save_if_oldest(E.lane); last_save = now; }
    }
    for (auto &x : th) x.join();
    // drain the checker queue, then stop it
    for (;;) { { std::lock_guard<std::mutex> lk(J.chk_mutex); if (J.checker.empty()) break; } if (J.quit.load()) break; std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
    J.all_done = true; J.chk_cv.notify_all();
    for (auto &x : chk) x.join();
}
// one public key of the list (1_9_7File.pb:4995-5168), from its claim to its output
void search_job(const Run &R, JobList &jobs, const LaneEngines &E, const JobList::Claim &cl, FILE *joblog, bool &tune)
{
    const Config &c = R.cfg;
    JobText o{jobs.live(), ""};
    Affine realpub;
    if (!hs::parse_pubkey(realpub, jobs.pub(cl.listpos)) || !hs::on_curve(realpub)) die("Invalid Public Key (-pb) length!!!");
    if (cl.resumed && pub_hex(realpub) != jobs.recovery().pub) die("Find position but the keys are different");
    o.say("\nFindpubkey  : %s\n", hs::compress_pubkey(realpub).c_str());
    const Affine findpub = hs::point_add(realpub, R.start_neg);      // 1_9_7File.pb:5042
    o.say("Searchpubkey: %s\n", hs::compress_pubkey(findpub).c_str());
    Scalar key0 = hs::fe_from_u64(1);
    if (cl.resumed && !hs::fe_from_hex(key0, jobs.recovery().cnt)) die("bad counter");
    Job J(R, cl.listpos, realpub, findpub, key0, E.devs.size(), E.lane == 0 ? joblog : nullptr);
    jobs.publish(E.lane, J);
    if (!c.host_centres) {
        if (J.walk_p0.inf) die("the public key equals (counter + p*w)*G: the first tile centre is the point at infinity");
        uint8_t p0[64], st[64];
        hs::affine_to_le(J.walk_p0, p0, p0 + 32); hs::affine_to_le(R.pubadd, st, st + 32);
        for (bsgs_dev *d : E.devs) CK(bsgs_set_walk(d, p0, st));    // from here on the host only advances the counter
        if (tune) { tune = false; tune_placement(E, o); }
    }
    const auto t0 = Clock::now();
    bool trivial = false;                                             // keys 1 and 2 are answered without search (5069-5107)
    for (uint64_t k : {1, 2}) {
        const Affine q = hs::point_mul(hs::G, hs::fe_from_u64(k));
        if (hs::fe_equal(q.x, realpub.x) && hs::fe_equal(q.y, realpub.y)) { J.winkey = hs::fe_from_u64(k); trivial = true; }
    }
    if (trivial) J.found = true;
    else search(J, E, jobs);
    const double secs = since(t0);
    std::string win;
    if (J.found) {                                                    // win.txt 1_9_7File.pb:5146-5160
        std::string console;
        win = key_lines(J.listpos, J.winkey, realpub, console);
        o.say("%s", console.c_str());
    } else o.say("\nReached end of space\n");
    o.say("Job time %.2fs, %llu tiles, %.3e giant steps\n", secs, (unsigned long long)J.tiles_done.load(), (double)J.steps_done.load());
    o.say("Checker: %llu hits resolved in %.3fs of CPU time (%.2f%% of one core)\n", (unsigned long long)J.hits_checked.load(), J.checker_ns.load() * 1e-9,
          secs > 0 ? 100.0 * J.checker_ns.load() * 1e-9 / secs : 0.0);
    jobs.finish(E.lane, o.text, J.found, win);                        // withdraws J before it goes
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && std::string(argv[1]) == "-selftest") return selftest(argc, argv);
    for (int i = 1; i < argc; i++) if (strcasecmp(argv[i], "-kangaroo") == 0) return kangaroo_main(argc, argv);     // host_kangaroo.cpp
    printf("BSGS MI355X (drop-in for bsgscudaHT 1.9.7-file0) on %s\n", bsgs_version());
    Run R;
    R.cfg = parse_args(argc, argv);
    const Config &c = R.cfg;
    Stages stage;
    const bool cpu_only = c.cpugen && c.onlygen;
    if (c.cpugen && (c.ext || c.w_auto)) die("-cpugen builds files in the reference`s format: not with -ext / -w auto / -w above 3069485950");
    std::vector<int> gpus = find_gpus(c, cpu_only);
    stage("runtime + device discovery");
    for (int g : gpus) tune(g);
    stage("Tune lines (open / close every GPU)");
    setup_range(R, gpus, cpu_only);
    TableFiles files;
    load_or_build_files(R, files, gpus);
    stage("table + giants files (load, or build + save)");
    if (c.onlygen) { files.flush_writers(); printf("onlygen: files ready\n"); return 0; }

    Recovery rec = read_recovery(c);
    JobList jobs(read_pubs(c), std::move(rec), c.dir, [&c](int listpos, const std::string &pub, const Scalar &cnt) { save_checkpoint(c, listpos, pub, cnt); });
    std::thread mini_builder;                                         // extended tables: the resolver's own multiples of G, built on the host BEHIND the GPU start-up
    if (c.ext) mini_builder = std::thread([&R]() {
        const auto t0 = Clock::now();
        R.tab.mini.build(R.cfg.w, std::max(1u, std::thread::hardware_concurrency() / 2));
        printf("Resolver table: 2^%u multiples of G in %.1fs (behind the start-up)\n", R.tab.mini.mb, since(t0));
    });
    const size_t lanes = plan_lanes(R, gpus.size(), jobs.todo());
    jobs.open_lanes(lanes);
    const std::vector<bsgs_dev *> devs = start_engines(R, gpus, lanes, files);
    stage("upload, bucket lines, chain scratch, replicas");
    files.start_writers();
    FILE *joblog = nullptr;
    if (!c.joblog.empty()) { joblog = fopen(c.joblog.c_str(), "w"); if (!joblog) die("Can`t create " + c.joblog); }
    // freshly generated files keep being written BEHIND the search (their writers are joined before the process leaves; a file appears under its name only once it is
    // complete: write_file): the 13 GB of HT files of a -w 30 run cost the first jobs nothing.  Only the resolver's table must be there before the first hit.
    if (mini_builder.joinable()) mini_builder.join();
    stage("resolver table (behind the start-up)");

    // ---- the jobs: one public key after the other (1_9_7File.pb:4995-5168) -- or, when a job is only a launch or two long (BASELINE config 4: 1000 keys over a 64-bit
    // range), `lanes` of them side by side, each on an engine of its own per GPU: while one job waits for its checker, dispenses, or parses the next key, the other's
    // launch keeps the GPU busy, and no tile is searched on speculation.  win.txt and the console keep the list order; currentwork.txt describes the OLDEST job in flight.
    const Run &run = R;
    const size_t G = gpus.size() / lanes;                             // engines per lane
    auto run_lane = [&](size_t l) {
        const LaneEngines E{l, std::vector<int>(gpus.begin() + l * G, gpus.begin() + (l + 1) * G), std::vector<bsgs_dev *>(devs.begin() + l * G, devs.begin() + (l + 1) * G)};
        bool tune = c.tune && l == 0;
        JobList::Claim cl;
        while (jobs.claim(l, cl)) search_job(run, jobs, E, cl, joblog, tune);
    };
    std::vector<std::thread> lt;
    for (size_t l = 1; l < lanes; l++) lt.emplace_back(run_lane, l);
    run_lane(0);
    for (auto &t : lt) t.join();
    if (joblog) fclose(joblog);
    files.flush_writers();                                            // the files that were still being written behind the search
    files.htgpu.release();                                            // host staging copies (1_9_7File.pb:4818-4843)
    files.g2.release();
    printf("Found %d of %zu\n", jobs.found(), jobs.size());
    fflush(stdout);
    if (getenv("BSGS_HOST_CLEAN_EXIT")) { for (size_t gi = devs.size(); gi-- > 0;) bsgs_dev_close(devs[gi]); return 0; }      // twins (borrowed tables) before their owners
    // the search is over and every file is on disk: leave without the runtime's teardown (freeing a few hundred GiB of device memory buffer by buffer and unloading
    // the code objects costs 0.15-0.3 s of a 64-bit solve that takes one; the driver reclaims everything with the process)
    _exit(0);
}
