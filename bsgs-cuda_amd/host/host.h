// host.h -- declarations shared by the translation units of bsgs_mi355x, the C++ host of the MI355X BSGS solver (see bsgs_host.cpp for the reference
// file:line map).  host_config.cpp: command line, limits, checkpoint; host_files.cpp: table files and the CPU-only generator; host_resolver.cpp: dispenser and hit
// resolver; host_jobs.cpp: Job, the key list and its lanes (JobList); host_tune.cpp: Tune; host_engines.cpp: per-GPU engines (load, verify, search thread);
// host_selftest.cpp: -selftest; bsgs_host.cpp: main and the start-up steps.  -kangaroo: host_kangaroo_run.cpp: the prologue and the run loop of every mode (engines, collector, saving, signals)
// behind the seam of host_kangaroo_run.h; host_kangaroo.cpp: command line, one key (plain and -ksym) and its table; host_kangaroo_multi.cpp: -infile and its table for a list of keys;
// host_kangaroo_work.cpp: the work file kangaroo.work.
#pragma once
#include "../../include/bsgs_hip.h"
#include "../csrc/host_secp.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fcntl.h>
#include <fstream>
#include <functional>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

using hs::Affine;
using hs::Scalar;

// ---- configuration ---------------------------------------------------------------------------------------------------
struct Config {
    uint32_t t = 256, b = 132, p = 400;           // defaults 1_9_7File.pb:181-184
    uint64_t w = 1ull << 25;
    uint32_t htsz = 25;
    std::string devices;                           // -d
    std::string pub = "036d05521c67b9cc1c0ef906b42215c7120c7302c34d9316a2726199bedac50936";   // 1_9_7File.pb:191
    std::string pk = "0x01", pke = "1ffffffffffffffff";                                        // 1_9_7File.pb:197, 210
    bool pke_given = false;
    std::string infile, recovery_file;
    int wt = 180;
    bool onlygen = false;                          // onlygen_1_9_6File0.exe behaviour: build files and exit
    bool cpugen = false;                           // -cpugen: table and giants files built on the host CPU (with -onlygen: no GPU is touched at all)
    uint64_t max_tiles = 0;                        // test hook: stop after this many tiles (0 = unlimited)
    bool ext = false;                              // extended table (bucket lines + overflow list, no HT files); implied by w >= 3069485951
    std::string dir = ".";                         // where table / output files live
    bool verify_replicas = true;                   // verify before searching (-noverify skips): census + sampled k*G + sampled giants on every engine, and -- several engines -- table checksums and the hits of one tile compared across them
    bool ref_quirks = false;                       // -refquirks: reproduce the reference kernel's NEGMODP bug bit for bit (BSGS_FLAG_REFERENCE_QUIRKS)
    bool host_centres = false;                     // -hostcentres: tile centres added on the host and uploaded (the reference's way) instead of the device walk
    bool tune = false;                             // -tune: also choose the bucket-line placement by measurement at start-up (bsgs_tune_placement)
    std::string joblog;                            // test hook: log every dispenser / checkpoint event to this file
    uint32_t htsz_arg = 25;                        // what the extended-table entry points take as `htsz`: the exponent, or -- `-htsz` with a fraction, `-buckets` -- the bucket COUNT
    std::string startup = "auto";                  // -startup: how N engines get their replicas -- broadcast | local | allgather | auto (include/bsgs_hip.h BSGS_STARTUP_*)
    std::string transport = "auto";                // -transport: rccl | peer | auto
    int lanes = -1;                                // -lanes: jobs (public keys of -infile) searched side by side, each on its own engine per GPU; -1 = automatic (2 for short jobs)
    bool w_auto = false;                           // -w auto: the table Tune picks for the range given (tune_plan)
    bool file_search = true;                       // -sf (hidden in the reference too, 1_9_7File.pb:907-918; its default is 1, 1_9_7File.pb:178, and so is this host's): htCPU looked up in the file instead of RAM when the file is there at start-up (a table built in this run is still in RAM)
};

[[noreturn]] void die(const std::string &msg);
std::string cut_hex(std::string s);
std::string sha1_hex(const std::string &msg);
void usage(const Config &c);
Config parse_args(int argc, char **argv);
std::string table_limits(uint64_t w, uint32_t htsz, FILE *answers);
std::string fingerprint(const Config &c);

// ---- files ---------------------------------------------------------------------------------------------------------------
// the table images on the host (up to 36 GB): plain allocations that are NOT zero-filled first -- a std::vector's resize writes every byte once before the file read or the
// download from the GPU writes it again, a second and a half for the 12 GiB of a -w 30 run
struct HostBuf {
    uint8_t *p = nullptr;
    uint64_t n = 0;
    HostBuf() {}
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { free(p); }
    // Large images (the 5.4 + 9.6 GB of a -w 30 table) are taken 2 MiB-aligned, offered to transparent huge pages and FIRST-TOUCHED BY SEVERAL THREADS: the kernel
    // clears every page it hands out, and one thread faulting 15 GB in (inside a device-to-host copy or a read()) is most of a 3.4 s "build + bring to the host" stage
    void resize(uint64_t bytes);
    void release() { free(p); p = nullptr; n = 0; }
    uint8_t *data() { return p; }
    const uint8_t *data() const { return p; }
    uint64_t size() const { return n; }
    const uint8_t &operator[](uint64_t i) const { return p[i]; }
};
bool file_has_size(const std::string &path, uint64_t expect);
bool read_file(const std::string &path, HostBuf &out, uint64_t expect);
void write_file(const std::string &path, const void *p, uint64_t n);
void cpu_build_tables(uint64_t w, uint32_t htsz, uint8_t *htgpu, uint8_t *htcpu);
void cpu_build_g2(const Affine &A, uint32_t t, uint32_t b, uint32_t p, uint8_t *g2);

#define CK(call) do { int rc_ = (call); if (rc_ != BSGS_OK) die(std::string("error " #call "-") + std::to_string(rc_) + ": " + bsgs_last_error()); } while (0)

// ---- run and job state ----------------------------------------------------------------------------------------------
struct MiniBsgs {
    unsigned mb = 0;
    std::vector<std::pair<uint64_t, uint32_t>> baby;     // (low 64 bits of x(jG), j), j = 1..2^mb, sorted
    Affine Q;                                            // 2^mb * G
    void build(uint64_t w, unsigned threads);
    size_t lookup(uint64_t x64) const;
    std::vector<uint64_t> find(const Affine &T, uint64_t w) const;     // every b' in [1, w] with x(b'G) = x(T)
};

// what every job of a run reads and nobody writes once the start-up is over: the resolver's tables
struct Tables {
    HostBuf htcpu;
    int htcpu_fd = -1;                            // -sf 1 (the reference's default, isFilesearch 1_9_7File.pb:178): htCPU stays in its FILE, a lookup is two reads (ReadHTpackFile /
                                                  // compareHTpackFile 1_9_7File.pb:3056-3099) -- 9.6 GB of host memory and most of the load time of a -w 30 run saved
    MiniBsgs mini;                                // extended tables: the resolver's own small BSGS instead of htCPU
};
struct Tile { Scalar key; uint64_t index; };          // counter and dispenser index of a tile: centre = walk_p0 + index * PUBADDBIG
struct PendingHit { uint32_t code, idx; Tile tile; };

// what every job of a run reads and nobody writes once the start-up is over: main() fills it in, everything after the start-up sees it const
struct Run {
    Config cfg;
    uint64_t maxnonce = 0;
    uint32_t batch_hint = 0;                       // short jobs: tiles per batch (each batch waits for its checker); 0 = a launch per batch
    Scalar center_big, gstep, start, width;      // p*w ; 4*maxnonce*w ; -pk ; pke-pk
    bool end_range = false;
    Affine addpubg, center, pubadd, start_neg;   // -(2w)G ; -(p*w)G ; -(gstep)G ; -(start)G
    Tables tab;
};
void derive_constants(Run &R);                    // maxnonce, center_big, center, gstep, pubadd, addpubg from cfg (1_9_7File.pb:4689-4712, 4759-4765)
std::string pub_hex(const Affine &q);             // x || y in hex: how currentwork.txt names a public key

// one public key's search (the reference's globals *GlobKey / GlobPub / checker() / quit): a fresh object per job, seeded completely by its constructor
struct Job {
    Job(const Run &run, int listpos, const Affine &realpub, const Affine &findpub, const Scalar &key0, size_t engines, FILE *joblog);
    const Run &run;
    const int listpos;
    const Affine realpub, findpub;
    const std::string pub_hex;
    FILE *const joblog;                           // test hook (-joblog): the jobs of lane 0 only
    const Affine walk_p0;                         // centre of tile 0 of this job: Q' - key0*G - C*G (1_9_7File.pb:5056-5064)
    std::mutex job_mutex;                         // the dispenser: counter of the next tile to hand out, its index (counter = key0 + index * gstep)
    Scalar glob_key;
    uint64_t glob_index = 0;
    bool past_end = false;
    std::mutex chk_mutex; std::condition_variable chk_cv; std::deque<PendingHit> checker;      // the checker queue
    std::atomic<bool> quit{false}, all_done{false};
    std::atomic<uint64_t> steps_done{0}, tiles_done{0};
    std::atomic<uint64_t> hits_pushed{0};                   // hits handed to the checker threads
    std::atomic<uint64_t> hits_checked{0}, checker_ns{0};   // resolver load: false positives cost CPU (a small BSGS each with an extended table)
    std::atomic<int> gpus_finished{0}; std::mutex done_mutex; std::condition_variable done_cv;
    std::mutex inflight_mutex;
    std::vector<Scalar> inflight;                 // per GPU: counter of the oldest tile it has not finished (checkpoint = min, 1_9_7File.pb:3904-3911)
    std::vector<bool> inflight_valid;
    Scalar winkey;
    bool found = false;
    Scalar checkpoint_counter();                  // what currentwork.txt saves for this job: the minimum counter in flight
};

void save_checkpoint(const Config &c, int listpos, const std::string &pub_hex, const Scalar &cnt);
Affine tile_centre(const Job &J, uint64_t index);
size_t get_jobs(Job &J, size_t n, std::vector<Tile> &out, int slot = -1);
int htcpu_lookup_file(int fd, uint64_t ht_items, uint64_t key64, uint32_t *pos, int max);
int htcpu_lookup(const HostBuf &img, uint64_t ht_items, uint64_t key64, uint32_t *pos, int max);
void checker_thread(Job *J);

// ---- the list of public keys (-pb / -infile) and its lanes: host_jobs.cpp -------------------------------------------------------------------------
struct Recovery { bool on = false; int pos = 0; std::string pub, cnt; std::set<int> won; };    // -wl (1_9_7File.pb:4634-4686); won: positions win.txt reports
Recovery read_recovery(const Config &c);
std::vector<std::string> read_pubs(const Config &c);

// Hands out list positions to lanes, prints / appends to win.txt in list order, and keeps currentwork.txt naming the oldest job in flight; one mutex guards
// all of it.  A lane's Job is visible to the other lanes only while it is published: from after its constructor until before its destructor.
class JobList {
public:
    using SaveFn = std::function<void(int listpos, const std::string &pub_hex, const Scalar &cnt)>;
    struct Claim { int listpos = 0; bool resumed = false; };
    JobList(std::vector<std::string> pubs, Recovery rec, std::string dir, SaveFn save);
    size_t size() const { return pubs_.size(); }
    size_t todo() const;                          // positions from the -wl one on
    void open_lanes(size_t lanes) { lanes_.assign(lanes, Lane()); live_ = lanes == 1; }     // before the first claim
    bool live() const { return live_; }           // one lane: a job's lines appear as they happen; several: when its turn in the list comes
    const Recovery &recovery() const { return rec_; }
    const std::string &pub(int listpos) const { return pubs_[(size_t)listpos - 1]; }
    bool claim(size_t lane, Claim &out);          // the next position to search; false when the list is done
    void publish(size_t lane, Job &J) { std::lock_guard<std::mutex> lk(m_); lanes_[lane].job = &J; }
    void save_if_oldest(size_t lane);             // the -wt timer: only the oldest job in flight is saved
    void finish(size_t lane, const std::string &text, bool found, const std::string &win);     // output, withdrawal, checkpoint hand-off
    int found() const { return found_; }
private:
    struct Out { bool done = false, found = false; std::string text, win; };
    struct Lane { int pos = 0; bool resumed = false; Job *job = nullptr; };     // pos 0: idle; job: once published
    void emit();
    void save_lane(const Lane &L);
    std::mutex m_;
    const std::vector<std::string> pubs_;
    const Recovery rec_;
    bool resume_pending_;                         // the -wl position has not been claimed yet
    const std::string dir_;
    const SaveFn save_;
    std::vector<Out> outs_;
    std::vector<Lane> lanes_;
    size_t next_emit_ = 0, next_job_ = 0;
    int found_ = 0;
    bool live_ = true;
};

struct TuneAdvice { double w_log2; uint32_t htsz; bool ext; uint32_t ext_w_log2, ext_htsz; };
struct TunePlan { double w_log2; uint32_t htsz_arg; bool ext; double build_s, search_s, total_s; uint64_t w; };      // w = the number of baby points itself (it need not be a power of two)
TuneAdvice tune_advice(uint64_t free_bytes);
TunePlan tune_plan(uint64_t free_bytes, double range_bits, int n_gpus, uint64_t maxnonce);
std::string plan_flags(const TunePlan &p);
void tune(int gpu);

bsgs_dev *open_dev(int gpu);
void print_placement(int gpu, size_t gi, bsgs_dev *dev);
void load_engines(const Run &R, const std::vector<int> &gpus, const std::vector<bsgs_dev *> &devs, const HostBuf &htgpu, const HostBuf &g2);
void verify_replicas(const std::vector<int> &gpus, const std::vector<bsgs_dev *> &devs);
void verify_tables(const Run &R, const std::vector<int> &gpus, const std::vector<bsgs_dev *> &devs);
void test_corrupt_engine(const std::vector<bsgs_dev *> &devs);       // test build only (-DBSGS_TEST_HOOKS); a no-op in the shipped host
void per_gpu(const std::vector<int> &gpus, const std::function<void(size_t)> &fn);
void gpu_thread(Job *J, int gpu, int slot, bsgs_dev *dev);
int selftest(int argc, char **argv);
// the lines a found key is reported with (1_9_7File.pb:5146-5160): returns the win.txt text, `console` receives the console block
std::string key_lines(int listpos, const Scalar &key, const Affine &pub, std::string &console);
// host_kangaroo.cpp: bsgs_mi355x -kangaroo, -selftest kangaroo (the table of distinguished points on a scripted record stream) and kangaroo-table-roundtrip;
// host_kangaroo_work.cpp: -selftest kangaroo-work
int kangaroo_main(int argc, char **argv);
int kangaroo_selftest(const std::vector<std::string> &args);
int kangaroo_work_selftest(const std::vector<std::string> &args);
int kangaroo_roundtrip_selftest(const std::vector<std::string> &args);
int kangaroo_dpdev_selftest(const std::vector<std::string> &args);               // -selftest kangaroo-dpdev [sym]: the hand-back rule of -kdpdev on scripted records and pairs
int kangaroo_dpshard_selftest(const std::vector<std::string> &args);             // -selftest kangaroo-dpshard [sym] <engines> <kn>: the hand-back rule of -kdpshard, kangaroo numbers global
int kangaroo_barrier_selftest(const std::vector<std::string> &args);             // -selftest kangaroo-barrier <event>...: -kdpshard's barrier before a save, scripted
int kangaroo_dpshard_plan_selftest(const std::vector<std::string> &args);        // -selftest kangaroo-dpshard-plan: the plan of -kdpshard for E engines
int kangaroo_dpkeys_selftest(const std::vector<std::string> &args);              // -selftest kangaroo-dpkeys [sym]: the hand-back rule of -kdpkeys on scripted records and pairs
int kangaroo_dpkeys_sym_selftest(const std::vector<std::string> &args);          // ... its part for the symmetric walk's table (host_kangaroo_symlist.cpp)
int kangaroo_dpkeys_plan_selftest(const std::vector<std::string> &args);         // -selftest kangaroo-dpkeys-plan: the plan of -kdpkeys (dp, herd, launch, record buffer, capacity)
int kangaroo_dpdev_plan_selftest(const std::vector<std::string> &args);          // -selftest kangaroo-dpdev-plan: the plan of -kdpdev (dp, herd, launch, record buffer, capacity)
int kangaroo_sym_selftest(const std::vector<std::string> &args);                 // -selftest kangaroo-sym: the symmetric walk's table
int kangaroo_sym_roundtrip_selftest(const std::vector<std::string> &args);       // -selftest kangaroo-sym-roundtrip: through a version-2 work file
int kangaroo_multi_roundtrip_selftest(const std::vector<std::string> &args);     // -selftest kangaroo-multi-roundtrip: through a version-3 work file
int kangaroo_symlist_selftest(const std::vector<std::string> &args);             // -selftest kangaroo-symlist: the table of -infile -kwalk sym (host_kangaroo_symlist.cpp)
int kangaroo_symlist_roundtrip_selftest(const std::vector<std::string> &args);   // -selftest kangaroo-symlist-roundtrip: through a version-4 work file
int kangaroo_multi_selftest(const std::vector<std::string> &args);               // -selftest kangaroo-multi: the table for a list of keys (host_kangaroo_multi.cpp)
int kangaroo_tames_selftest(const std::vector<std::string> &args);               // -selftest kangaroo-tames: the header of a tame table file (host_kangaroo_tames.cpp)
int kangaroo_tames_gen_selftest(const std::vector<std::string> &args);           // -selftest kangaroo-tames-gen: the rule of -ktamesgen -ktamesdev on scripted hand-backs
int kangaroo_tames_image_selftest(const std::vector<std::string> &args);         // -selftest kangaroo-tames-image: the device image of tags read from stdin
int kangaroo_tames_search_selftest(const std::vector<std::string> &args);        // -selftest kangaroo-tames-search: the search rule on scripted records
