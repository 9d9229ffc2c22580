// host_kangaroo_multi.h -- MultiKeyTable: the table of distinguished points of kangaroo mode for a list of public keys in one range
// (host_kangaroo_multi.cpp; the rule: include/bsgs_hip.h "Kangaroo, many keys").
#pragma once
#include "host_kangaroo.h"

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
