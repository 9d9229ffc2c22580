// host_jobs.cpp -- one public key's search (Job), and the list of keys the lanes take their jobs from (JobList): -wl and win.txt skipping, output in list
// order, and the checkpoint that names the oldest job in flight (1_9_7File.pb:4634-4686, 4995-5168).
#include "host.h"

void derive_constants(Run &R)
{
    const Config &c = R.cfg;
    R.maxnonce = (uint64_t)c.t * c.b * c.p;
    R.addpubg = hs::affine_neg(hs::point_mul(hs::G, hs::sc_from_u128((hs::u128)c.w * 2)));
    R.center_big = hs::sc_from_u128((hs::u128)c.p * c.w);
    R.center = hs::affine_neg(hs::point_mul(hs::G, R.center_big));
    R.gstep = hs::sc_mul_small(hs::sc_from_u128((hs::u128)R.maxnonce * c.w), 4);
    R.pubadd = hs::affine_neg(hs::point_mul(hs::G, R.gstep));
}
std::string pub_hex(const Affine &q) { return hs::fe_to_hex(q.x) + hs::fe_to_hex(q.y); }
// win.txt 1_9_7File.pb:5146-5160
std::string key_lines(int listpos, const Scalar &key, const Affine &pub, std::string &console)
{
    const std::string head = "KEY[" + std::to_string(listpos) + "]: ";
    const std::string l1 = head + "0x" + hs::fe_to_hex(key);
    const std::string l2 = std::string(head.size() - 5, ' ') + "Pub: " + hs::compress_pubkey(pub);
    console = "\n****************************\n" + l1 + "\n" + l2 + "\n****************************\n";
    return l1 + "\r\n" + l2 + "\r\n";
}
// dispenser seed (1_9_7File.pb:5046-5064)
Job::Job(const Run &run, int listpos, const Affine &realpub, const Affine &findpub, const Scalar &key0, size_t engines, FILE *joblog)
    : run(run), listpos(listpos), realpub(realpub), findpub(findpub), pub_hex(::pub_hex(realpub)), joblog(joblog),
      walk_p0(hs::point_add(hs::point_add(findpub, hs::affine_neg(hs::point_mul(hs::G, key0))), run.center)), glob_key(key0),
      inflight(engines, hs::fe_from_u64(0)), inflight_valid(engines, false) {}
// ---- recovery (-wl, 1_9_7File.pb:4634-4686)
Recovery read_recovery(const Config &c)
{
    Recovery r;
    if (c.recovery_file.empty()) { remove((c.dir + "/win.txt").c_str()); return r; }      // 1_9_7File.pb:4959-4963
    std::ifstream f(c.recovery_file);
    std::string l1, l2, l3, l4;
    auto strip = [](std::string s) { while (!s.empty() && (s.back() == '\r' || s.back() == '\n')) s.pop_back(); return s; };
    if (!std::getline(f, l1) || !std::getline(f, l2) || !std::getline(f, l3) || !std::getline(f, l4)) die("Can`t read recovery file");
    if (strip(l4) != fingerprint(c)) die("Recovery file was made with other settings");
    r.pos = atoi(strip(l1).c_str()); r.pub = strip(l2); r.cnt = strip(l3); r.on = true;
    // list positions win.txt already reports are not searched again (with several lanes a younger job can be reported before the checkpoint names its successor)
    std::ifstream wf(c.dir + "/win.txt", std::ios::binary);
    std::string wl;
    while (std::getline(wf, wl)) if (wl.rfind("KEY[", 0) == 0) r.won.insert(atoi(wl.c_str() + 4));
    printf("Recovery: listpos %d counter %s\n", r.pos, r.cnt.c_str());
    return r;
}
// ---- public keys (-pb or -infile, one per line, searched sequentially: 4370-4385, 4995-5168)
std::vector<std::string> read_pubs(const Config &c)
{
    if (c.infile.empty()) return {c.pub};
    std::vector<std::string> pubs;
    std::ifstream f(c.infile);
    if (!f) die("Can`t open " + c.infile);
    std::string line;
    while (std::getline(f, line)) { while (!line.empty() && isspace((unsigned char)line.back())) line.pop_back(); if (!line.empty()) pubs.push_back(cut_hex(line)); }
    return pubs;
}
JobList::JobList(std::vector<std::string> pubs, Recovery rec, std::string dir, SaveFn save)
    : pubs_(std::move(pubs)), rec_(std::move(rec)), resume_pending_(rec_.on), dir_(std::move(dir)), save_(std::move(save)), outs_(pubs_.size()) {}
size_t JobList::todo() const
{
    return pubs_.size() - (rec_.on && rec_.pos >= 1 && (size_t)rec_.pos <= pubs_.size() ? (size_t)rec_.pos - 1 : 0);
}
bool JobList::claim(size_t lane, Claim &out)
{
    std::lock_guard<std::mutex> lk(m_);
    while (next_job_ < pubs_.size() && resume_pending_ && (int)next_job_ + 1 != rec_.pos) outs_[next_job_++].done = true;      // -wl: everything before the saved position is skipped
    while (next_job_ < pubs_.size() && rec_.won.count((int)next_job_ + 1)) {      // ... and so is every position win.txt reports already (then the saved counter belongs to a finished job)
        outs_[next_job_].done = true;
        if (resume_pending_ && (int)next_job_ + 1 == rec_.pos) resume_pending_ = false;
        next_job_++;
    }
    if (next_job_ >= pubs_.size()) { lanes_[lane] = Lane(); return false; }
    out.listpos = (int)++next_job_;
    out.resumed = resume_pending_;                                  // the saved position resumes from the saved counter, everything after it starts fresh
    resume_pending_ = false;
    lanes_[lane] = Lane{out.listpos, out.resumed, nullptr};
    return true;
}
// a published job: its (immutable) position and key, its counter under the job's own locks.  A position that is claimed and not yet published: from its start
// counter, as a restart would search it
void JobList::save_lane(const Lane &L)
{
    if (L.job) { save_(L.job->listpos, L.job->pub_hex, L.job->checkpoint_counter()); return; }
    Affine q;
    if (!hs::parse_pubkey(q, pubs_[(size_t)L.pos - 1]) || !hs::on_curve(q)) return;
    Scalar cnt = hs::fe_from_u64(1);
    if (L.resumed && !hs::fe_from_hex(cnt, rec_.cnt)) return;
    save_(L.pos, ::pub_hex(q), cnt);
}
void JobList::save_if_oldest(size_t lane)
{
    std::lock_guard<std::mutex> lk(m_);
    bool oldest = true;                                             // currentwork.txt: the oldest job in flight (a restart re-does the younger ones from their start)
    for (const Lane &L : lanes_) oldest &= L.pos == 0 || L.pos >= lanes_[lane].pos;
    if (oldest) save_lane(lanes_[lane]);
}
// under m_: print / append to win.txt everything that is complete, in list order
void JobList::emit()
{
    while (next_emit_ < outs_.size() && outs_[next_emit_].done) {
        Out &o = outs_[next_emit_];
        if (!live_) fputs(o.text.c_str(), stdout);
        if (o.found) {
            std::ofstream f(dir_ + "/win.txt", std::ios::app | std::ios::binary);
            f << o.win;
            found_++;
        }
        o.text.clear();
        next_emit_++;
    }
    fflush(stdout);
}
void JobList::finish(size_t lane, const std::string &text, bool found, const std::string &win)
{
    std::lock_guard<std::mutex> lk(m_);
    Out &o = outs_[(size_t)lanes_[lane].pos - 1];
    o.text = text; o.found = found; o.win = win; o.done = true;
    emit();
    // currentwork.txt must stop naming this job the moment it is over (the timer would let it stand for up to -wt seconds: a restart in that window searched a
    // reported key again and appended a second KEY[n]): it now names the oldest job still in flight, or -- none in flight -- the next list position from its start
    lanes_[lane] = Lane();
    const Lane *oldest = nullptr;
    for (const Lane &L : lanes_) if (L.pos > 0 && (!oldest || L.pos < oldest->pos)) oldest = &L;
    if (oldest) save_lane(*oldest);
    else if (next_job_ < pubs_.size()) save_lane(Lane{(int)next_job_ + 1, false, nullptr});
}
