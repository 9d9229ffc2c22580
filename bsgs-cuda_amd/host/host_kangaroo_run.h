// host_kangaroo_run.h -- the one prologue and the one run loop of bsgs_mi355x -kangaroo (host_kangaroo_run.cpp), and the seam the modes stand
// behind: KeyMode (host_kangaroo.cpp: one public key, plain and -ksym), ListSearch<Table> (host_kangaroo_list.h: -infile) with its two walks ListMode
// (host_kangaroo_multi.cpp) and SymListMode (host_kangaroo_symlist.cpp: -kwalk sym), GenMode and SearchMode (host_kangaroo_tames.cpp: -ktamesgen, -ktames).
// The driver owns the engine threads, the collector, the monitor with the save handshake, the signals, the shutdown and the work file's common part; a Mode
// owns its table of distinguished points, how a kangaroo is started and what a record means.  A table kept in device memory (-kdpdev, -kdpkeys) is reached
// through DevDpTable (host_kangaroo_dptable.h), which KeyMode and ListSearch hold behind the launch, resumed and fetch hooks.
#pragma once
#include "host_kangaroo.h"

namespace kang {
class Mode;

// what a run works from: the range, the work file of -wl, the devices, the completed plan, the seed and the jump table
struct Prologue {
    explicit Prologue(const KangConfig &c);        // the range: validated, or the run ends here
    // -wl (read and checked before any device is looked for), mode.before_devices, the device list, the plan, the seed, the jump table; go = false: the
    // mode found nothing left to search
    void complete(const KangConfig &c, Mode &mode);
    Scalar lo, hi;
    u128 W;
    double sqrtW;
    bool resume = false, go = true;
    std::string wl_path, work_path, work_tmp;
    WorkFile wf;                                   // -wl: header, key list, re-seed lists; the table until the mode has restored it
    std::vector<uint8_t> check_table;              // -wl: the file's table entries as read, until the first engine has verified them
    std::vector<std::vector<bsgs_kangaroo_state>> herds;      // per engine, the herd to upload: the file's, or what a mode computed before the engines start
    double elapsed_before = 0.0;
    Clock::time_point t0 = Clock::now();           // what "Job time" counts from: each mode sets it where it always did
    std::vector<int> gpus;
    Plan pl;
    WorkHeader wh;                                 // what every save of this run shares
    std::vector<uint64_t> js;                      // jump table: s_j uniform in [1, 2m), m = scale * N_k sqrt(W) / 4 (at most 2^62): a function of the seed
    std::vector<uint8_t> jxy;                      // and the plan, never saved
    uint64_t rng;                                  // the seeded stream behind the jump table (-wl: the file's)
};

// -kdpshard: the barrier in front of an engine's last drain before a save ("a save stays a consistent cut").  Two kinds of round.  A SAVE round
// is opened by the saver before it asks for a save; its count belongs to that round alone, and an engine that waits in it leaves it -- without draining,
// nothing is saved from it -- when the round is given up (the request withdrawn, a stop, a newer round): a stop then brings the STOP round, the last one,
// whose count is never reset and which every living engine enters once.  Plain data under Shared::save_m; -selftest kangaroo-barrier scripts it.
struct SaveBarrier {
    uint64_t round = 0;
    uint32_t at_save = 0, at_stop = 0;
    enum State { WAIT, ALL, GIVEN_UP };
    void open() { round++; at_save = 0; }                                           // the saver, before save_req is set
    uint64_t arrive(bool stopped) { if (stopped) at_stop++; else at_save++; return round; }
    // stopped: the engine arrived in the stop round; my_round: what arrive() returned; living: engine threads alive; save_req, stop: as they stand now
    State state(bool stopped, uint64_t my_round, uint32_t living, bool save_req, bool stop) const
    {
        if (stopped) return at_stop >= living ? ALL : WAIT;
        if (round == my_round && at_save >= living) return ALL;
        return round != my_round || !save_req || stop ? GIVEN_UP : WAIT;
    }
};

// what the engines, the collector, the saver and the mode share
struct Shared {
    explicit Shared(const Prologue &p);
    std::atomic<bool> stop{false};
    std::atomic<uint64_t> steps{0}, dps{0}, dropped{0};
    std::mutex rng_m;
    uint64_t rng;                                  // the seeded stream: initial herds in engine order, then every re-seed
    std::mutex tab_m;                              // the mode's table and what hangs on it: held around record(), done(), give_up(), status() and save()
    std::mutex q_m; std::condition_variable q_cv;
    std::deque<std::pair<uint32_t, std::vector<bsgs_kangaroo_record>>> queue;     // (engine, records of one launch)
    bool collector_busy = false;                   // (under q_m) a batch has left the queue and is not in the table yet
    std::vector<std::unique_ptr<std::mutex>> reseed_m;
    std::vector<std::vector<uint32_t>> reseed;     // per engine: kangaroos (local index) to start afresh
    std::vector<uint64_t> engine_records;
    std::mutex err_m; std::string err;
    std::atomic<bool> failed{false};               // err is set
    std::atomic<uint32_t> checked{0};              // -wl: engines whose herd (the first one: and the saved table) went through the verification; none walks before all have
    // saving ("a save is a consistent cut"): engines park between two launches with their herd downloaded
    std::atomic<bool> save_req{false};
    std::mutex save_m; std::condition_variable save_cv;
    uint32_t parked = 0, running = 0;              // (under save_m) engines waiting for the save to end / engine threads alive
    std::vector<std::vector<bsgs_kangaroo_state>> saved;      // per engine: the herd as downloaded at the last park or at the end
    Clock::time_point ended;                       // when the engines and the collector had ended, before the last save
    // -kdpshard ("divided over engines"): what other engines routed to engine e waits in inbox[e] until e inserts it before its next launch;
    // routed[e]: records engine e sent away; barrier (under save_m): which engines have made their last launch before a save and pushed what it routed
    struct Inbox { std::mutex m; std::vector<bsgs_kangaroo_record> recs; };
    std::vector<std::unique_ptr<Inbox>> inbox;
    std::unique_ptr<std::atomic<uint64_t>[]> routed;
    SaveBarrier barrier;
    bool inboxes_empty() { for (auto &b : inbox) { std::lock_guard<std::mutex> lk(b->m); if (!b->recs.empty()) return false; } return true; }
    void push_reseed(uint32_t e, uint32_t i) { std::lock_guard<std::mutex> lk(*reseed_m[e]); reseed[e].push_back(i); }
};

class Mode {
public:
    virtual ~Mode() {}
    // what the prologue asks: the work file's version, the floor of the launch length, the jump table's size and scale, how a refused -wl is worded
    uint32_t version = WORK_VERSION, jumps = BSGS_KANGAROO_JUMPS;
    double min_launch = 8.0, jumpscale = 1.0;
    const char *wl_flag = "-kangaroo -wl", *wl_kind = "a kangaroo.work file";
    // what a mode that walks with a table made earlier sets before Prologue::complete (host_kangaroo_tames.cpp): the dp of that table (-1: the command line's
    // or the plan's), the mean jump (0: jumpscale * N_k sqrt(W) / 4), the jump scalars themselves (null: drawn from the seed), the steps the run expects before
    // the DP overhead (0: 2 sqrt(W)), and whether the run writes kangaroo.work at all
    int dp_fixed = -1;
    double mean_jump = 0.0, expected = 0.0;
    const uint64_t *jump_scalars = nullptr;
    bool saves = true;
    // a mode whose distinguished points stay in device memory (-kdpdev): the launch itself counts what the walk produced, so the collector does not count the
    // records that come back; the launch is kept so short that the records it is expected to write fill at most half of the largest record buffer, and when
    // the floor of the launch length does not do it, dp is raised as long as the command line (or a work file) has not fixed it
    bool counts_records = true, bound_launch = false, dp_free = false;
    // a mode whose table in device memory is divided over the engines (-kdpshard): an engine drains its inbox before every launch, and before a save no
    // engine drains its last inbox until every living engine has made its last launch (the barrier of the run loop)
    bool sharded = false;
    virtual std::string drain(bsgs_dev *dev, uint32_t e, Shared &sh) { (void)dev; (void)e; (void)sh; return ""; }
    // once the device list stands (p.gpus) and before the herd is planned: a mode whose dp depends on the number of engines fixes it here
    virtual void engines_known(Prologue &p) { (void)p; }
    const char *herd_label = "herds (GPU), engine ";                  // the [startup] line of a herd seeded in its engine's thread
    virtual std::string fingerprint(const Prologue &p, const WorkHeader &h) const = 0;
    // between the work file and the devices: the mode's own resume checks ("Recovery file was made with other settings"), its header fields, its first
    // lines, the keys known without a search; false: nothing is left to search
    virtual bool before_devices(Prologue &p) = 0;
    // once the herd is planned (p.pl: engines, kangaroos, dp) and before the jump table is drawn: a mode whose mean jump depends on the herd sets it here
    virtual void planned(const Prologue &p) { (void)p; }
    // in an engine's thread; nullptr, or the name of the call that failed
    virtual const char *setup(bsgs_dev *dev) = 0;
    virtual const char *setup_engine(bsgs_dev *dev, uint32_t e) { (void)e; return setup(dev); }      // ... for a mode that needs the engine's number
    // starts the kangaroos idx of engine e (empty: the whole herd, from the offsets drawn in engine order before the run); draws under the locks it needs
    virtual const char *seed(bsgs_dev *dev, uint32_t e, const std::vector<uint32_t> &idx, Shared &sh) = 0;
    // under sh.tab_m.  One record of engine e into the table: kangaroos to start afresh go on sh's lists, a finished search sets sh.stop; false: the rest of
    // the batch is not looked at
    virtual bool record(uint32_t e, const bsgs_kangaroo_record &r, Shared &sh) = 0;
    // in an engine's thread: one launch of `steps` steps of engine e's herd, its records to recs.  Today's call; a mode whose records are matched on the
    // device names the call that does that
    virtual int launch(bsgs_dev *dev, uint32_t e, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t cap, uint32_t *n, uint64_t *dropped, Shared &sh)
    {
        (void)e; (void)sh;
        return bsgs_kangaroo_run(dev, steps, recs, cap, n, dropped, nullptr);
    }
    // in an engine's thread, after its last launch and before its device is closed (only when nothing failed): a mode that keeps something in device memory
    // fetches it here; "", or the message the run ends with
    virtual std::string ending(bsgs_dev *dev, uint32_t e, Shared &sh) { (void)dev; (void)e; (void)sh; return ""; }
    // in an engine's thread, -wl only: after the herd and the saved table went through the verification (or -noverify skipped it) and before the first launch: a
    // mode that keeps its table in device memory loads it here; "", or the message the run ends with
    virtual std::string resumed(bsgs_dev *dev, uint32_t e, Shared &sh) { (void)dev; (void)e; (void)sh; return ""; }
    // in an engine's thread, where its herd has been downloaded for a save (parked between two launches, or at the end of a search that is not done): a mode
    // that keeps its table in device memory reads it into host memory here, so that save() writes what belongs to this moment; "", or the message
    virtual std::string fetch(bsgs_dev *dev, uint32_t e, Shared &sh) { (void)dev; (void)e; (void)sh; return ""; }
    // what the verification needs (bsgs_kangaroo_verify, bsgs_kangaroo_verify_points; set in before_devices): the one Q of every wild kangaroo, or null: the
    // key list the engines got in setup(); why the device cannot check this search, or null; the flags a table entry's type or owner word stands for
    const uint8_t *verify_q = nullptr;
    const char *verify_skip = nullptr;
    virtual uint32_t entry_flags(uint32_t word) const = 0;
    virtual bool done() const = 0;
    virtual bool give_up(uint64_t steps) = 0;
    virtual void status(double rate, uint64_t steps, uint64_t dps) const = 0;
    // the mode's part of a work file: the table's entries and counters, its own header fields; the key list's state or nullptr
    virtual const WorkKeys *save(WorkHeader &h, std::vector<uint8_t> &entries) = 0;
};

// the launch of a plan whose herd and dp stand: the expected total (expected0, or 2 sqrt(W) when that is 0, plus the DP overhead N_k 2^dp), S = an eighth of a
// kangaroo's share of it within [min_launch, 1024], and the record buffer for twice the records a launch is expected to write (at most 2^22).  bound: S, then
// dp (only when dp_free), give way until kn S / 2^dp is at most 2^21, half of the largest record buffer
void plan_launch(Plan &pl, double sqrtW, double expected0, double min_launch, bool bound, bool dp_free);

// a key of a list is known: its KEY[n] block (n = listpos, from 1) on the console and at the end of <dir>/win.txt at once, through key_lines as the BSGS path
// writes it
void report_key(const std::string &dir, int listpos, const Scalar &key, const Affine &pub);

enum Outcome { DONE, GAVE_UP, BUDGET, INTERRUPTED, ENDED };           // ENDED: stopped for none of the other reasons
// engines, collector, monitor, shutdown and the last save; the mode turns the outcome into its closing text and exit code
Outcome run(const KangConfig &c, Prologue &p, Shared &sh, Mode &mode);
}  // namespace kang
