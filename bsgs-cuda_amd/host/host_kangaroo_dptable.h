// host_kangaroo_dptable.h -- DevDpTable: the host's client of the table of distinguished points in device memory (include/bsgs_hip.h "Kangaroo,
// distinguished-point table in device memory" and its keyed form), once for -kdpdev (KeyMode, host_kangaroo.cpp) and -kdpkeys (ListSearch,
// host_kangaroo_list.h).  A mode keeps its own table on the host, says which type or owner words are legal and which square root sizes the table, and judges
// what take() names a pair or a record alone; the rest is here.  Under -kdpshard (KeyMode only) it is the client of E tables, one per engine, each the
// shard of its engine ("Kangaroo, distinguished-point table divided over engines"): a launch hands its routed groups to the destinations' inboxes in Shared,
// an engine drains its inbox before its next launch, and every kangaroo id that comes back is global (engine * kn + index).
#pragma once
#include "host_kangaroo_run.h"

namespace kang {
struct DevDpTable {
    bool sharded = false;                          // -kdpshard: E tables, one per engine; capacity is each table's
    uint32_t E = 1, cap = 0;                       // engines; the record buffer of each (shards())
    uint64_t kn = 0;                               // kangaroos per engine: ids are e * kn + index
    bool on = false, keyed = false;                // -kdpdev or -kdpkeys; -kdpkeys: an owner per entry, and the key of a handed-back record in `reserved`
    uint64_t capacity = 0;                         // of the device table
    std::atomic<uint64_t> entries{0};              // entries in it after the last launch (the monitor's status line reads it)

    // in the mode's constructor: under the flag the launch counts the records, and is kept within the record buffer
    void enable(const KangConfig &c, Mode &m)
    {
        on = c.kdpdev || c.kdpkeys || c.kdpshard; keyed = c.kdpkeys; sharded = c.kdpshard; m.sharded = sharded;
        if (on) { m.counts_records = false; m.bound_launch = true; m.dp_free = c.dp < 0; }
    }
    // the capacity (-kdpn, or from sq: sqrt(W) for one key, sqrt(L_open W) for a list; doubled for a work file that holds more than this run would plan for);
    // returns the dp: -dp, or the one that fills at most half of the capacity
    // engines (-kdpshard): each of them holds 1 / engines of the points, so the rule is the one table's with sq / engines: capacity per engine = -kdpn or the
    // power of two at or above 4 sq / engines, dp = ceil(log2(4 sq / (engines * capacity)))
    int plan(const KangConfig &c, double sq, uint64_t file_entries, uint32_t engines = 1)
    {
        sq /= (double)engines;
        capacity = dpdev_capacity(sq, c.kdpn);
        while (capacity < 2 * file_entries / engines && capacity < (1ull << 31)) capacity *= 2;
        return c.dp >= 0 ? c.dp : (int)dpdev_dp(sq, capacity);
    }
    // -kdpshard, once the plan stands: the engines, their herds and record buffers
    void shards(uint32_t engines, uint64_t herd, uint32_t record_cap)
    {
        E = engines; kn = herd; cap = record_cap;
        pend.resize(E); devt.resize(E); out.resize(E);
        for (uint32_t e = 0; e < 16; e++) ent[e] = 0;
    }
    static uint32_t shard_of(uint64_t tag, uint32_t engines) { return (uint32_t)(((tag >> 48) * engines) >> 16); }
    // the transport of a routed group: host buffer to host buffer (a peer-to-peer path can take its place)
    static void relay(const bsgs_kangaroo_record *src, size_t n, std::vector<bsgs_kangaroo_record> &dst) { dst.insert(dst.end(), src, src + n); }
    // -wl: the file's entries go to the device once they are verified (resumed()); tag 0 stays in file_table, for the host's own map.  fits: whether an
    // entry's type or owner word is legal; false: the section does not load
    bool split(std::vector<uint8_t> &file_table, const std::function<bool(uint32_t)> &fits)
    {
        std::vector<uint8_t> own;
        for (size_t i = 0; i + 32 <= file_table.size(); i += 32) {
            const uint8_t *en = &file_table[i];
            uint64_t k64; uint32_t word;
            memcpy(&k64, en, 8); memcpy(&word, en + 28, 4);
            if (!fits(word)) return false;
            std::vector<uint8_t> &to = !k64 ? own : sharded ? pend[shard_of(k64, E)] : pending;
            to.insert(to.end(), en, en + 32);
        }
        file_table.swap(own);
        entries = pending.size() / 32;
        for (uint32_t e = 0; sharded && e < E; e++) { ent[e] = pend[e].size() / 32; entries += ent[e].load(); }
        return true;
    }
    // the end of a mode's setup(): the table behind the herd (keyed: behind the key list); nullptr, or the name of the call that failed
    const char *begin(bsgs_dev *dev, uint32_t e = 0) const
    {
        if (sharded) return bsgs_kangaroo_dptable_begin_shard(dev, capacity, e, E, (uint32_t)(e * kn)) == BSGS_OK ? nullptr : "bsgs_kangaroo_dptable_begin_shard";
        if (!on || (keyed ? bsgs_kangaroo_dptable_begin_keys : bsgs_kangaroo_dptable_begin)(dev, capacity) == BSGS_OK) return nullptr;
        return keyed ? "bsgs_kangaroo_dptable_begin_keys" : "bsgs_kangaroo_dptable_begin";
    }
    // the walk, the insert and the pairing in device memory; only the hand-backs reach the collector, and the DP count is the walk's
    int launch(bsgs_dev *dev, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t cap, uint32_t *n, uint64_t *dropped, Shared &sh, uint32_t e = 0)
    {
        uint64_t seen = 0, now = 0, dead = 0;
        int rc;
        if (sharded) {                                                 // the routed groups to their engines' inboxes
            uint32_t n_routed[16] = {0};
            out[e].resize(this->cap);
            rc = bsgs_kangaroo_run_dptable_shard(dev, steps, recs, cap, n, out[e].data(), this->cap, n_routed, &seen, &now, dropped, nullptr);
            if (rc != BSGS_OK) return rc;
            size_t at = 0;
            for (uint32_t s = 0; s < E; s++) {
                if (n_routed[s]) { std::lock_guard<std::mutex> lk(sh.inbox[s]->m); relay(out[e].data() + at, n_routed[s], sh.inbox[s]->recs); }
                at += n_routed[s];
            }
            sh.routed[e] += at;
            ent[e] = now;
            now = 0;
            for (uint32_t s = 0; s < E; s++) now += ent[s].load();
        } else rc = (keyed ? bsgs_kangaroo_run_dptable_keys : bsgs_kangaroo_run_dptable)(dev, steps, recs, cap, n, &seen, &now, dropped, nullptr);
        if (rc != BSGS_OK) return rc;
        for (uint32_t i = 0; i < *n; i++) dead += recs[i].reserved != BSGS_KANGAROO_DPT_STORED && (recs[i].flags & BSGS_KANGAROO_DEAD);
        sh.dps += seen - std::min(seen, dead);
        entries = now;
        return rc;
    }
    // -kdpshard, in engine e's thread before a launch and before a save: what the other engines routed here goes into this shard, in pieces of at most the
    // record buffer; what the table hands back goes to the collector under this engine's number.  A record that comes back routed names another shard: an error
    std::string drain(bsgs_dev *dev, uint32_t e, Shared &sh)
    {
        std::vector<bsgs_kangaroo_record> in;
        { std::lock_guard<std::mutex> lk(sh.inbox[e]->m); in.swap(sh.inbox[e]->recs); }
        for (size_t at = 0; at < in.size(); at += cap) {
            const uint32_t m = (uint32_t)std::min<size_t>(cap, in.size() - at);
            std::vector<bsgs_kangaroo_record> back(2 * (size_t)m);
            bsgs_kangaroo_record stray[16];                            // room for a record of every other shard: enough to name where a stray one belongs
            uint32_t n = 0, n_routed[16] = {0};
            uint64_t now = 0, dropped = 0;
            if (bsgs_kangaroo_dptable_insert_shard(dev, in.data() + at, m, back.data(), 2 * m, &n, stray, 16, n_routed, &now, &dropped) != BSGS_OK)
                return std::string("bsgs_kangaroo_dptable_insert_shard: ") + bsgs_last_error();
            for (uint32_t s = 0; s < E; s++) if (n_routed[s]) return "-kangaroo -kdpshard: a record in the inbox of engine " + std::to_string(e) + " belongs to engine " + std::to_string(s);
            if (dropped) return "-kangaroo -kdpshard: records of an inbox were dropped";
            ent[e] = now;
            back.resize(n);
            if (n) { { std::lock_guard<std::mutex> lk(sh.q_m); sh.queue.emplace_back(e, std::move(back)); } sh.q_cv.notify_one(); }
        }
        if (!in.empty()) { uint64_t sum = 0; for (uint32_t s = 0; s < E; s++) sum += ent[s].load(); entries = sum; }
        return "";
    }
    // -wl: the file's entries, verified, into the device table; a tag that occurs twice, is 0 or finds no slot: the section does not load
    std::string resumed(bsgs_dev *dev, const std::string &wl_path, uint32_t e = 0)
    {
        std::vector<uint8_t> &pending = sharded ? pend[e] : this->pending;      // (each engine loads its own share, in its own thread)
        if (!on || pending.empty()) return "";
        uint64_t stored_n = 0, dup = 0, zero = 0, full = 0, now = 0;
        const auto ts = Clock::now();
        if (bsgs_kangaroo_dptable_load(dev, (const bsgs_kangaroo_dp_entry *)pending.data(), pending.size() / 32, &stored_n, &dup, &zero, &full, &now) != BSGS_OK)
            return std::string("bsgs_kangaroo_dptable_load: ") + bsgs_last_error();
        if (dup || full || zero) return "-kangaroo -wl: the table section of " + wl_path + " does not load";
        printf("[startup] %-44s %.3fs\n", ("table (GPU memory), " + std::to_string(now) + " entries").c_str(), since(ts));
        if (sharded) ent[e] = now; else entries = now;
        std::vector<uint8_t>().swap(pending);
        return "";
    }
    // the device table as it stands, for save()
    std::string fetch(bsgs_dev *dev, uint32_t e = 0)
    {
        if (!on) return "";
        uint64_t n = 0;
        if (bsgs_kangaroo_dptable_read(dev, nullptr, 0, &n) != BSGS_OK) return std::string("bsgs_kangaroo_dptable_read: ") + bsgs_last_error();      // the count alone
        std::vector<uint8_t> got(32 * n);
        if (n && bsgs_kangaroo_dptable_read(dev, (bsgs_kangaroo_dp_entry *)got.data(), n, &n) != BSGS_OK) return std::string("bsgs_kangaroo_dptable_read: ") + bsgs_last_error();
        if (32 * n != got.size()) return "bsgs_kangaroo_dptable_read: the table changed between the count and the read";
        std::lock_guard<std::mutex> lk(dev_m);
        (sharded ? devt[e] : dev_table).swap(got);
        return "";
    }
    // the device's half of a mode's save(): what fetch() read when the herds were downloaded opens `out` -- moved, not copied: every save follows a fetch() of
    // its own -- and counts in h.table beside the host's entries, which the mode appends
    void save(WorkHeader &h, std::vector<uint8_t> &out, size_t host_entries)
    {
        std::lock_guard<std::mutex> lk(dev_m);
        for (uint32_t e = 0; sharded && e < E; e++) { dev_table.insert(dev_table.end(), devt[e].begin(), devt[e].end()); std::vector<uint8_t>().swap(devt[e]); }      // the shards in engine order
        h.table = host_entries + dev_table.size() / 32;
        out.swap(dev_table);
        std::vector<uint8_t>().swap(dev_table);
        out.reserve(out.size() + 32 * host_entries);
    }
    // the device's sizing rule (bsgs_kang_table_slots and KT_MIN_SLOTS, csrc/kangaroo_table.hip.h) restated for the banner: the power of two at or above
    // 2 * (capacity + record buffer), at least 128
    uint64_t slots(uint32_t record_cap) const { uint64_t s = 128; while (s < 2 * (capacity + record_cap)) s *= 2; return s; }
    void banner(uint32_t record_cap) const
    {
        if (sharded) {
            printf("Kangaroo: distinguished points stay in GPU memory (-kdpshard): %u tables, one per engine, of %llu entries, %llu slots each, %.2f GiB in all; records of another engine's share are relayed\n",
                   E, (unsigned long long)capacity, (unsigned long long)slots(record_cap), (double)E * (double)slots(record_cap) * 32.0 / 1073741824.0);
            return;
        }
        printf("Kangaroo: distinguished points stay in GPU memory (%s): table of %llu entries, %llu slots, %.2f GiB; hand-backs only cross the bus\n",
               keyed ? "-kdpkeys" : "-kdpdev", (unsigned long long)capacity, (unsigned long long)slots(record_cap), (double)slots(record_cap) * 32.0 / 1073741824.0);
    }
    // under sh.tab_m.  What a record of a launch is: NOT_MINE (the flag is off) or ALONE (DEAD, tag 0, a full device table), both for the mode's own map;
    // STORED_HALF (the entry the next record met: kept here until that record comes); PAIR (a duplicate, to be judged against *stored, the entry it came
    // with, and never stored); ORPHAN (a duplicate with no stored half before it -- never: the device does not split a pair -- to be skipped).  walk: the
    // record as the walk wrote it -- keyed, `reserved` = reason | key << BSGS_KANGAROO_DPT_KEY_SHIFT holds the key again
    enum Kind { NOT_MINE, STORED_HALF, PAIR, ORPHAN, ALONE };
    struct Taken { Kind kind; bsgs_kangaroo_record walk; const bsgs_kangaroo_record *stored; };
    Taken take(const bsgs_kangaroo_record &r)
    {
        Taken t{NOT_MINE, r, &half};
        if (!on) return t;
        if (r.reserved == BSGS_KANGAROO_DPT_STORED) { half = r; have_stored = true; t.kind = STORED_HALF; return t; }
        if (keyed) t.walk.reserved = r.reserved >> BSGS_KANGAROO_DPT_KEY_SHIFT;
        const bool dup = (keyed ? r.reserved & ((1u << BSGS_KANGAROO_DPT_KEY_SHIFT) - 1u) : r.reserved) == BSGS_KANGAROO_DPT_DUPLICATE;
        t.kind = !dup ? ALONE : have_stored ? PAIR : ORPHAN;
        if (dup) have_stored = false;
        return t;
    }
    // -selftest kangaroo-dpdev / kangaroo-dpkeys: the items behind the range and the keys, as the device would hand them back.  rec(text, paired) judges one
    // scripted record through take_scripted(); paired: it stands behind S,<tag hex>,<d hex>,<kangaroo>,<type or owner word>, the stored half it is a duplicate
    // of, which went through take() before it.  false: an item does not parse or is refused
    bool scripted_items(const std::vector<std::string> &a, const std::function<bool(const std::string &, bool)> &rec)
    {
        for (size_t i = 3; i < a.size(); i++) {
            const bool paired = on && a[i].compare(0, 2, "S,") == 0;
            if (paired) {
                const std::vector<std::string> s = split_commas(a[i++]);
                Scalar tag, d;
                if (i >= a.size() || s.size() != 5 || !hs::fe_from_hex(tag, s[1]) || tag.l[1] || tag.l[2] || tag.l[3] || !hs::fe_from_hex(d, s[2]) || d.l[2] || d.l[3]) return false;
                bsgs_kangaroo_record st;
                memset(&st, 0, sizeof st);
                memcpy(st.x, &tag.l[0], 8); memcpy(st.d, &d.l[0], 16);
                st.kangaroo = (uint32_t)strtoul(s[3].c_str(), nullptr, 10); st.flags = (uint32_t)strtoul(s[4].c_str(), nullptr, 10);
                st.reserved = BSGS_KANGAROO_DPT_STORED;
                if (take(st).kind != STORED_HALF) return false;
            }
            if (!rec(a[i], paired)) return false;
        }
        return true;
    }
    // a scripted record r, as the walk wrote it, of key `key`: alone it is DEAD or met a full table; a pair must share its tag, else ORPHAN: refused
    Taken take_scripted(bsgs_kangaroo_record r, uint32_t key, bool paired)
    {
        if (on) r.reserved = (paired ? BSGS_KANGAROO_DPT_DUPLICATE : r.flags & BSGS_KANGAROO_DEAD ? BSGS_KANGAROO_DPT_DEAD : BSGS_KANGAROO_DPT_FULL) | (keyed ? key << BSGS_KANGAROO_DPT_KEY_SHIFT : 0u);
        Taken t = take(r);
        if (t.kind != PAIR || !memcmp(t.stored->x, r.x, 8)) return t;
        fprintf(stderr, "the record does not share the tag of the stored entry it is paired with\n");
        t.kind = ORPHAN;
        return t;
    }
    bsgs_kangaroo_record half;                     // the first record of a handed-back pair, until its record comes
private:
    bool have_stored = false;
    std::vector<std::vector<uint8_t>> pend, devt;  // -kdpshard: the same two per engine
    std::vector<std::vector<bsgs_kangaroo_record>> out;      // -kdpshard: the routed records of an engine's launch, until they are relayed
    std::atomic<uint64_t> ent[16];                 // -kdpshard: entries per engine; `entries` is their sum
    std::vector<uint8_t> pending, dev_table;       // -wl: the file's entries on their way to the device; the device table as fetch() read it
    std::mutex dev_m;                              // dev_table: fetch() in the engine's thread, save() in the saver's
};
}  // namespace kang
