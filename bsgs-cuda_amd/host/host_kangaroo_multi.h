// host_kangaroo_multi.h -- MultiKeyTable: the table of distinguished points of kangaroo mode for a list of public keys in one range
// (host_kangaroo_multi.cpp; the rule: include/bsgs_hip.h "Kangaroo, many keys"), and Assigner, which the list search of either walk shares out its wild
// kangaroos with (host_kangaroo_symlist.cpp is the other).
#pragma once
#include "host_kangaroo.h"

#include <set>
#include <unordered_map>

class MultiKeyTable {
public:
    enum What { NEW, REPEAT, RESEED, FALSE_MATCH, LINK, FOUND };
    // what one record did: RESEED a = the kangaroo to start afresh; LINK a, b = the two keys; FOUND a = the key's list position (from 0), key = its value
    struct Event { What what; uint32_t a, b; Scalar key; };
    MultiKeyTable(const Scalar &a, unsigned __int128 W, const std::vector<Affine> &pubs);
    // a key known before the search: P_k == a*G, or one a work file reports as solved
    void presolve(uint32_t k, const Scalar &key);
    // one record into the table; its events are appended to ev (one record can solve several keys through links)
    void add(const uint8_t x[32], unsigned __int128 d, uint32_t kid, uint32_t flags, std::vector<Event> &ev);
    // -kdpkeys: a record the device table handed back as a duplicate, against the stored entry it came with (d, kangaroo, owner word): exactly the events
    // add() gives for a record that meets that entry in the map; never NEW, and the map is not touched
    void add_pair(__int128 entry_d, uint32_t entry_kid, uint32_t entry_owner, unsigned __int128 d, uint32_t kid, uint32_t flags, std::vector<Event> &ev);
    bool owner_fits(uint32_t owner) const { return owner <= pubs_.size(); }         // an owner word of this list: 0, or 1 + a list position
    // key k learnt outside the table (a wild start at infinity): the same consequences as a collision that solves it
    void found(uint32_t k, const Scalar &key, std::vector<Event> &ev);
    bool known(uint32_t k) const { return known_[k]; }
    const Scalar &key(uint32_t k) const { return key_[k]; }
    uint32_t solved() const { return solved_; }
    size_t size() const { return map_.size(); }
    uint64_t false_matches() const { return false_; }
    uint64_t reseeds() const { return reseeds_; }
    uint64_t links_kept() const { return kept_; }
    uint64_t links_resolved() const { return resolved_; }
    uint64_t links_open() const { return live_links_; }
    // the work file's view (version 3): one 32-byte entry per stored point -- low 64 bits of x, d, kangaroo, owner -- and the key list's state
    void write_entries(std::vector<uint8_t> &out) const;
    void write_keys(kang::WorkKeys &out) const;
    // a fresh table from a work file: false when an entry or a link does not fit the list
    bool restore(const uint8_t *entries, uint64_t n, uint64_t false_matches, uint64_t reseeds, const kang::WorkKeys &keys);
private:
    struct Entry { __int128 d; uint32_t kid, owner; };           // owner: 0 tame, 1 + list position for a wild kangaroo of that key
    struct Link { uint32_t j, k; __int128 delta; bool alive; };  // k_j = k_k + delta
    bool verify(uint32_t k, __int128 off, Scalar *key) const;
    static uint32_t record_owner(uint32_t flags) { return flags & BSGS_KANGAROO_WILD ? 1u + ((flags >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu) : 0u; }
    void judge(const Entry &e, __int128 d, uint32_t kid, uint32_t owner, std::vector<Event> &ev);
    const Scalar a_;
    const unsigned __int128 W_;
    const std::vector<Affine> pubs_;
    std::vector<bool> known_;
    std::vector<Scalar> key_;
    std::vector<__int128> off_;                                  // k_k - a of a solved key
    std::unordered_map<uint64_t, Entry> map_;
    std::vector<Link> links_;
    std::vector<std::vector<uint32_t>> adj_;                     // per key: its links, in the order they were kept
    uint64_t false_ = 0, reseeds_ = 0, kept_ = 0, resolved_ = 0, live_links_ = 0;
    uint32_t solved_ = 0;
};

// which key a wild kangaroo works on (include/bsgs_hip.h "Kangaroo, many keys", assignment; tests/kangaroo_multi_model.py Assigner)
class Assigner {
public:
    Assigner(uint32_t L, const std::vector<bool> &presolved, uint64_t n_wild) : count_(L, 0), key_(n_wild)
    {
        for (uint32_t k = 0; k < L; k++) if (!presolved[k]) open_.push_back(k);
        for (uint64_t w = 0; w < n_wild; w++) { key_[w] = open_[w % open_.size()]; count_[key_[w]]++; }
        for (uint32_t k : open_) by_count_.insert({count_[k], k});
    }
    uint32_t key(uint64_t w) const { return key_[w]; }
    void solved(uint32_t k) { by_count_.erase({count_[k], k}); }                   // k takes no kangaroo from now on
    // the key of wild kangaroo w from now on: its own while that is open, else the open key with the fewest kangaroos, lowest position first; false: none open
    template <class TABLE> bool reseed(uint64_t w, const TABLE &t, uint32_t *k)
    {
        const uint32_t old = key_[w];
        if (!t.known(old)) { *k = old; return true; }
        if (by_count_.empty()) return false;
        const uint32_t best = by_count_.begin()->second;
        by_count_.erase(by_count_.begin());
        count_[old]--; count_[best]++;
        by_count_.insert({count_[best], best});
        key_[w] = best; *k = best;
        return true;
    }
    const std::vector<uint32_t> &keys() const { return key_; }
    // -wl: every wild kangaroo's key as its saved state names it
    template <class TABLE> void restore(const std::vector<uint32_t> &keys, const TABLE &t)
    {
        key_ = keys;
        std::fill(count_.begin(), count_.end(), 0u);
        for (uint32_t k : key_) count_[k]++;
        by_count_.clear();
        for (uint32_t k : open_) if (!t.known(k)) by_count_.insert({count_[k], k});
    }
private:
    std::vector<uint32_t> open_, count_, key_;
    std::set<std::pair<uint32_t, uint32_t>> by_count_;                             // (kangaroos, list position) of the keys still open
};

