// host_kangaroo_list.h -- what the two searches of a key list in one range share behind the driver's seam (host_kangaroo_run.h): ListSearch<Table>, the Mode of
// bsgs_mi355x -kangaroo -infile, and list_main, its command.  Here once: the key file, the keys solved before any device is opened, the assignment of wild
// kangaroos (Assigner), the offsets of the herds, seeding and re-seeding with the key per position, what a FOUND event brings about (the KEY[n] block and
// win.txt, equal points of the list, the key's kangaroos started afresh), the give-up bound scaled by the open keys, the status line, saving and the
// closing lines.  A walk supplies the rest (host_kangaroo_multi.cpp ListMode: the plain walk, Q_k counted from -pk, the key in the flags;
// host_kangaroo_symlist.cpp SymListMode: the symmetric walk, Q_k counted from the middle of the range, the key beside the flags): its table, where offsets
// count from, how an offset is drawn, the device's herd, where a state keeps its key, what a record does to the table.
// -kdpkeys: the table in device memory is DevDpTable's (host_kangaroo_dptable.h), the member dpt; the list says which owner words are legal, sizes the table
// by sqrt(L_open W), and hands what DevDpTable::take names a pair or a record alone to the walk's table.
#pragma once
#include "host_kangaroo_dptable.h"
#include "host_kangaroo_multi.h"

#include <map>

namespace kang {
template <class Table> struct ListSearch : Mode {
    typedef typename Table::Event Event;
    ListSearch(const KangConfig &c, const std::vector<Affine> &P) : c(c), P(P), L((uint32_t)P.size())
    {
        if (c.cpuseed) herd_label = "herds (host), engine ";
        dpt.enable(c, *this);
    }
    // ---- what a walk supplies
    virtual void own_settings(Prologue &) {}                                       // its header fields, and its part of "made with other settings"
    virtual Scalar origin(const Prologue &p) const = 0;                            // offsets count from here: Q_k = P_k - origin*G, and a wild start at infinity is origin - d
    virtual Table *new_table(const Prologue &p) const = 0;
    virtual bool restore_table(Prologue &p) = 0;                                   // -wl: the file's table, links, solved keys and counters
    virtual i128 offset(uint64_t &rng, bool wild) const = 0;
    virtual uint32_t state_key(const bsgs_kangaroo_state &s) const = 0;            // the key a saved wild kangaroo names
    virtual void put_key(bsgs_kangaroo_state &s, uint32_t key) const = 0;          // the host's comb: the key into a state whose flags are the type
    virtual void print_expectation(const Prologue &p) const = 0;
    virtual void add_record(const bsgs_kangaroo_record &r, uint32_t kid, std::vector<Event> &ev) = 0;
    // -kdpkeys: a record (as the walk wrote it) that the device table handed back as a duplicate, against the stored entry it came with
    virtual void add_pair_record(const bsgs_kangaroo_record &stored, const bsgs_kangaroo_record &r, uint32_t kid, std::vector<Event> &ev) = 0;
    virtual void save_own(WorkHeader &) const {}
    virtual void closing() const {}                                                // its line between the job's figures and the engines'

    std::string fingerprint(const Prologue &p, const WorkHeader &h) const override { return keys_fingerprint(P, p.lo, p.hi, h); }
    void report(uint32_t k) { report_key(c.dir, (int)k + 1, table->key(k), P[k]); found_n++; }      // a key is known
    bool before_devices(Prologue &p) override
    {
        pro = &p;
        if (p.resume && p.wf.keys.solved.size() != L) die("Recovery file was made with other settings");
        own_settings(p);
        if (!p.resume) { Config rc; rc.dir = c.dir; read_recovery(rc); }         // (win.txt starts empty, as on the BSGS path; a resumed run appends to the one it has)
        p.t0 = Clock::now();
        table.reset(new_table(p));
        for (uint32_t k = 0; k < L; k++) same[hs::compress_pubkey(P[k])].push_back(k);
        // keys solved before any device is opened: P_k == origin*G has no affine Q_k; it keeps its slot (G stands in, no kangaroo is assigned)
        base = origin(p);
        const Affine nbG = hs::affine_neg(hs::point_mul(hs::G, base));
        presolved.assign(L, false);
        qxy.resize(64 * (size_t)L);
        Q.resize(L);
        for (uint32_t k = 0; k < L; k++) {
            Q[k] = hs::point_add(P[k], nbG);
            if (Q[k].inf) { presolved[k] = true; table->presolve(k, base); if (p.resume) found_n++; else report(k); Q[k] = hs::G; }
            hs::affine_to_le(Q[k], &qxy[64 * (size_t)k], &qxy[64 * (size_t)k + 32]);
        }
        const uint64_t file_entries = p.resume ? p.wf.h.table : 0;
        if (c.kdpkeys && p.resume) {                                               // an entry's owner word is 0 or names a key of this list
            const Table *t = table.get();
            if (!dpt.split(p.wf.table, [t](uint32_t owner) { return t->owner_fits(owner); })) die("-kangaroo -wl: the table section of " + p.wl_path + " does not load");
            p.wf.h.table = p.wf.table.size() / 32;
        }
        if (p.resume) {                                                            // the file's solved keys are in win.txt already: counted, not written again
            const uint32_t before = table->solved();
            if (!restore_table(p)) die("-kangaroo -wl: the table section of " + p.wl_path + " does not load");
            std::vector<uint8_t>().swap(p.wf.table);
            found_n += (int)(table->solved() - before);
        }
        open0 = L - table->solved();
        if (!open0) printf("Found %d of %u\n", found_n, L);
        // the table in device memory: -kdpdev's rule with sqrt(L_open W) in the place of sqrt(W)
        if (c.kdpkeys && open0) dp_fixed = dpt.plan(c, std::sqrt((double)open0 * (double)p.W), file_entries);
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
        print_expectation(p);
        asg.reset(new Assigner(L, presolved, (kn - half) * pl.engines));
        if (p.resume) {
            std::vector<uint32_t> keys((kn - half) * pl.engines);
            for (uint32_t e = 0; e < pl.engines; e++) for (uint64_t i = half; i < kn; i++) {
                const uint32_t k = state_key(p.herds[e][i]);
                if (k >= L) die("-kangaroo -wl: a kangaroo of " + p.wl_path + " names key " + std::to_string(k));
                keys[(uint64_t)e * (kn - half) + (i - half)] = k;
            }
            asg->restore(keys, *table);
            printf("Resumed: %llu steps, %zu DPs, %u of %u keys solved\n", (unsigned long long)p.wf.h.steps, table_size(), table->solved(), L);
        }
        if (c.cpuseed) comb.reset(new Comb());
        steps_mark = s.steps.load();
        last_solved = table->solved();
        off0.resize(pl.engines);
        if (!p.resume) for (uint32_t e = 0; e < pl.engines; e++) { off0[e].resize(kn); for (uint64_t i = 0; i < kn; i++) off0[e][i] = offset(s.rng, i >= half); }
    }
    // under sh->tab_m.  The consequences of FOUND events: the block is written, equal points of the list are solved with it, the key's kangaroos start afresh
    void on_events(const std::vector<Event> &ev)
    {
        const uint64_t wild = pro->pl.kn - half;
        for (const Event &x : ev) {
            if (x.what != Table::FOUND) continue;
            report(x.a);
            asg->solved(x.a);
            for (uint64_t w = 0; w < asg->keys().size(); w++) if (asg->keys()[w] == x.a) sh->push_reseed((uint32_t)(w / wild), (uint32_t)(half + w % wild));
            for (uint32_t o : same[hs::compress_pubkey(P[x.a])]) if (!table->known(o)) {
                std::vector<Event> more;
                table->found(o, x.key, more);
                on_events(more);
            }
        }
        if (table->solved() == L) sh->stop = true;
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
                d.push_back(offset(s.rng, wild));
            }
            if (use.empty()) return nullptr;
        }
        uint32_t ninf = 0, first = 0;
        if (c.cpuseed) {                                                           // the same herd from the host's comb
            std::vector<const Affine *> q(d.size());
            for (size_t k = 0; k < d.size(); k++) q[k] = fl[k] ? &Q[key[k]] : nullptr;
            std::vector<bsgs_kangaroo_state> st;
            const std::vector<size_t> inf = comb_states(*comb, d, fl, q, st);
            for (size_t k = 0; k < d.size(); k++) put_key(st[k], key[k]);
            for (size_t k : inf) st[k].flags |= BSGS_KANGAROO_DEAD;
            if ((use.empty() ? bsgs_kangaroo_upload(dev, 0, (uint32_t)st.size(), st.data()) : bsgs_kangaroo_upload_list(dev, use.data(), (uint32_t)use.size(), st.data())) != BSGS_OK) return "bsgs_kangaroo_upload";
            if (!inf.empty()) { ninf = 1; first = (uint32_t)inf[0]; }
        } else if (bsgs_kangaroo_seed_keys(dev, use.empty() ? nullptr : use.data(), 0, (uint32_t)d.size(), (const uint8_t *)d.data(), fl.data(), key.data(), &ninf, &first) != BSGS_OK) return "bsgs_kangaroo_seed_keys";
        if (ninf) {
            if (fl[first]) {                                                       // Q_key + d G = infinity: the key is origin - d
                std::lock_guard<std::mutex> lt(s.tab_m);
                if (!table->known(key[first])) {
                    std::vector<Event> ev;
                    table->found(key[first], hs::sc_add(base, sc_from_i128(-d[first])), ev);
                    on_events(ev);
                }
            }
            s.push_reseed(e, use.empty() ? first : use[first]);
        }
        return nullptr;
    }
    // -kdpkeys: the keyed table after the key list (a walk's setup() ends with dpt.begin); the launch, the load at -wl and the read for a save are its own
    int launch(bsgs_dev *dev, uint32_t e, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t cap, uint32_t *n, uint64_t *dropped, Shared &s) override
    {
        return dpt.on ? dpt.launch(dev, steps, recs, cap, n, dropped, s) : Mode::launch(dev, e, steps, recs, cap, n, dropped, s);
    }
    std::string resumed(bsgs_dev *dev, uint32_t, Shared &) override { return dpt.resumed(dev, pro->wl_path); }
    std::string fetch(bsgs_dev *dev, uint32_t, Shared &) override { return dpt.fetch(dev); }
    size_t table_size() const { return table->size() + (size_t)dpt.entries.load(); }      // "in the table": the host's entries and the device's
    bool record(uint32_t e, const bsgs_kangaroo_record &r, Shared &s) override
    {
        std::vector<Event> ev;
        const uint32_t kid = (uint32_t)(e * pro->pl.kn + r.kangaroo);
        const DevDpTable::Taken t = dpt.take(r);                                   // t.walk: the record as the walk wrote it
        switch (t.kind) {
        case DevDpTable::STORED_HALF: case DevDpTable::ORPHAN: return true;
        case DevDpTable::PAIR:
            if (!table->owner_fits(t.stored->flags)) {                             // the table names a key the list does not have
                std::lock_guard<std::mutex> lk(s.err_m);
                if (s.err.empty()) s.err = "-kangaroo -kdpkeys: the table in GPU memory is damaged: an entry names owner " + std::to_string(t.stored->flags) + ", the list has " + std::to_string(L) + " keys";
                s.failed = true; s.stop = true;
                return false;
            }
            add_pair_record(*t.stored, t.walk, kid, ev);
            break;
        default: add_record(t.walk, kid, ev);                                      // no -kdpkeys, or what the device hands back alone: the host's own map
        }
        for (const Event &x : ev) if (x.what == Table::RESEED) s.push_reseed(e, r.kangaroo);
        on_events(ev);
        return true;
    }
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
        h.false_matches = table->false_matches(); h.reseeds = table->reseeds();
        save_own(h);
        dpt.save(h, entries, table->size());                                       // -kdpkeys: the device's entries first
        table->write_entries(entries);
        table->write_keys(wk);
        return &wk;
    }

    const KangConfig &c;
    const std::vector<Affine> &P;
    const uint32_t L;
    const Prologue *pro = nullptr;
    Shared *sh = nullptr;
    Scalar base;
    std::unique_ptr<Table> table;
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
    DevDpTable dpt;                                // -kdpkeys
};

// bsgs_mi355x -kangaroo -infile FILE with the walk of ModeT: every key of the list in [pk, pke] with ONE herd per engine
template <class ModeT> int list_main(const KangConfig &c)
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
    ModeT mode(c, P);
    p.complete(c, mode);                                                           // dp, kn, the jump mean and the launch length from W, as for one key
    if (!p.go) return 0;
    if (c.kdpkeys) mode.dpt.banner(p.pl.cap);
    Shared sh(p);
    mode.prepare(p, sh);
    const Outcome o = run(c, p, sh, mode);

    const auto &table = *mode.table;
    if (o == GAVE_UP) printf("\nKangaroo: %u of %u keys open after 20 times the expected steps (are the keys in the range?)\n", L - table.solved(), L);
    else if (o != DONE) printf("\nKangaroo: stopped after %llu steps (%s), %u of %u keys open\n", (unsigned long long)sh.steps.load(), o == BUDGET ? "-ksteps" : "signal",
                               L - table.solved(), L);
    printf("Job time %.2fs, %.3e kangaroo steps, %llu DPs (%zu in the table, %llu dropped), %llu false matches, %llu re-seeds, %llu links kept, %llu links resolved\n", p.elapsed_before + since(p.t0),
           (double)sh.steps.load(), (unsigned long long)sh.dps.load(), mode.table_size(), (unsigned long long)sh.dropped.load(), (unsigned long long)table.false_matches(),
           (unsigned long long)table.reseeds(), (unsigned long long)table.links_kept(), (unsigned long long)table.links_resolved());
    mode.closing();
    for (uint32_t e = 0; e < p.pl.engines; e++) printf("Engine %u (GPU #%d): %llu records\n", e, p.gpus[e], (unsigned long long)sh.engine_records[e]);
    printf("Found %d of %u\n", mode.found_n, L);
    fflush(stdout);
    return o == DONE ? 0 : (o == BUDGET || o == INTERRUPTED) ? 3 : 1;
}
}  // namespace kang
