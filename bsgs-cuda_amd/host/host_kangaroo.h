// host_kangaroo.h -- what the kangaroo hosts share (host_kangaroo.cpp: one public key, plain and -ksym; host_kangaroo_multi.cpp: a list of keys in one range;
// host_kangaroo_run.{h,cpp}: the prologue and the run loop both go through; host_kangaroo_work.cpp: the work file): the seeded stream and the herd offsets,
// the host's comb and its start points, the command line, the plan of a run from the range width, the work file's reader and writer, the selftests' helpers.
#pragma once
#include "host.h"

namespace kang {
using Clock = std::chrono::steady_clock;
typedef unsigned __int128 u128;
typedef __int128 i128;
inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

inline uint64_t splitmix64(uint64_t &state)
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline u128 draw128(uint64_t &state) { const uint64_t lo = splitmix64(state), hi = splitmix64(state); return ((u128)hi << 64) | lo; }
// start offsets (tests/kangaroo_model.py herd_offset): tame t uniform in [1, W), wild u uniform in [-W/2, W/2), both from the seeded stream
inline i128 herd_offset(uint64_t &state, u128 W, bool wild)
{
    const u128 r = draw128(state);
    return wild ? (i128)(r % W) - (i128)(W / 2) : (i128)(1 + r % (W - 1));
}
// the symmetric walk (tests/kangaroo_sym_model.py herd_offset): tame uniform in [0, W/2), wild uniform in [-W/4, W/4), the same stream
inline i128 herd_offset_sym(uint64_t &state, u128 W, bool wild)
{
    u128 r = draw128(state) % (W / 2);
    while (!wild && !r) r = draw128(state) % (W / 2);                 // a tame kangaroo at 0 would stand on the point at infinity: the next draw
    return wild ? (i128)r - (i128)(W / 4) : (i128)r;
}
inline Scalar sc_from_i128(i128 v) { return v >= 0 ? hs::sc_from_u128((u128)v) : hs::sc_neg(hs::sc_from_u128((u128)-v)); }

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
// start points from the comb: state k is d[k] * G, plus *Q[k] where Q[k] is not null, with flags fl[k]; returns the positions that stand at infinity (x and y
// zero there; what such a start means is the caller's: the key itself for one key, a dead kangaroo and a solved key for a list)
std::vector<size_t> comb_states(const Comb &C, const std::vector<i128> &d, const std::vector<uint32_t> &fl, const std::vector<const Affine *> &Q, std::vector<bsgs_kangaroo_state> &out);

struct KangConfig {
    std::string devices, pub = Config().pub, pk = Config().pk, pke = Config().pke, dir = ".", wl;
    int dp = -1;                                   // -dp (default: from W; resumed: from the work file)
    uint64_t kn = 0;                               // -kn: kangaroos per engine (default: from W; resumed: from the work file)
    uint64_t seed = 0;
    bool seed_given = false;
    int wt = 180;                                  // -wt: seconds between two saves of kangaroo.work
    uint64_t ksteps = 0;                           // -ksteps: stop (saved, rc 3) once this many steps were walked in total
    bool cpuseed = false;                          // -kcpuseed: start points from the host's comb instead of bsgs_kangaroo_seed
    std::string infile;                            // -infile: a list of public keys in the one range (host_kangaroo_multi.cpp)
    bool pub_given = false;
    bool sym = false;                              // -ksym, or -kwalk sym with -pb: the symmetric walk (negation map)
    bool symlist = false;                          // -kwalk sym with -infile: the symmetric walk for the key list (host_kangaroo_symlist.cpp)
    uint32_t jumps = 0;                            // -kjumps: jump points of the symmetric walk (default 1024; resumed: from the work file)
    double jumpscale = 0.0;                        // -kjumpscale: mean jump = scale * N_k sqrt(W) / 4 (default KSYM_JUMPSCALE; resumed: from the work file)
    bool verify = true;                            // -noverify: herds and the saved table are not checked against their offsets (at -wl, before every save)
    std::string ktamesgen, ktames;                 // -ktamesgen FILE: make a tame table; -ktames FILE: search with one (host_kangaroo_tames.cpp)
    uint64_t ktn = 0;                              // -ktn: entries of the table -ktamesgen makes
    bool ktamesdev = false;                        // -ktamesdev with -ktamesgen: the growing table lives in device memory (bsgs_kangaroo_run_tames_gen)
    bool tames_sym = false;                        // -kwalk sym with -ktamesgen / -ktames: the table of the symmetric walk (file version 2)
    std::string ktamesfrom;                        // -ktamesfrom IN with -ktamesgen -ktamesdev: IN is loaded into the growing table and extended to -ktn entries
    std::string ktamesmerge;                       // -ktamesmerge A,B[,C...] with -ktamesgen: the tables are merged by tag on the host
    uint64_t ktnplan = 0;                          // -ktnplan N with -ktamesgen: the walk is planned for a table of N entries (0: for -ktn)
    bool range_given = false;                      // -pk or -pke stood on the command line
    bool kdpdev = false;                           // -kdpdev with -pb, plain and -ksym: the table of distinguished points lives in device memory (bsgs_kangaroo_run_dptable)
    uint64_t kdpn = 0;                             // -kdpn N with -kdpdev or -kdpkeys: the capacity of that table (default: dpdev_capacity)
    bool kdpshard = false;                         // -kdpshard with -pb, plain and -ksym: that table divided over the engines of -d, each share in its engine's memory (bsgs_kangaroo_run_dptable_shard)
    bool kdpkeys = false;                          // -kdpkeys with -infile, plain and -kwalk sym: the list search's table lives in device memory (bsgs_kangaroo_run_dptable_keys)
};
KangConfig parse_kangaroo_args(int argc, char **argv);

struct Plan { uint32_t engines, dp, G, S, cap; uint64_t kn; double expected; };
// defaults from W: expected DPs (2 sqrt(W) / 2^dp) within 2^25 host entries, DP overhead N_k 2^dp at most sqrt(W) / 8, a full herd is 16 kangaroos per
// thread at four waves per SIMD; dp_arg < 0 / kn_arg == 0: chosen here.  S and cap are left to the caller (they depend on the expected total).
Plan plan_herd(double sqrtW, uint32_t engines, int cus, int dp_arg, uint64_t kn_arg);
// -kdpdev ("the table of distinguished points in device memory"): the capacity is -kdpn, or the power of two at or above 4 sqrt(W) within
// [2^16, 2^27]; the default dp = max(0, ceil(log2(4 sqrt(W) / capacity))): the 2 sqrt(W) / 2^dp expected DPs fill at most half the capacity, a quarter of the
// slots.  The herd then follows by plan_herd's rule, up to the full herd.
uint64_t dpdev_capacity(double sqrtW, uint64_t kdpn);
uint32_t dpdev_dp(double sqrtW, uint64_t capacity);

// ---- the work file <dir>/kangaroo.work: version 1 the plain walk, 2 -ksym, 3 a list of keys (-infile), 4 a list with -kwalk sym --------
const uint32_t WORK_VERSION = 1, WORK_VERSION_SYM = 2, WORK_VERSION_KEYS = 3;       // 2: written and read by -ksym only; the header continues behind the fingerprint
const uint32_t WORK_VERSION_SYMKEYS = 4;           // the layout of 3 with the header fields of 2 behind the fingerprint, links of 48 bytes, NEG in bit 31 of an owner word
struct WorkHeader {
    uint32_t version = WORK_VERSION, jumps = 0;
    double jumpscale = 0.0;
    uint64_t cycles = 0;
    uint32_t engines = 0, dp = 0, per_thread = 0;
    uint64_t herd = 0, seed = 0, rng = 0, steps = 0, dps = 0, dropped = 0, false_matches = 0, reseeds = 0, table = 0;
    double elapsed = 0.0;
    std::string fingerprint;                       // 40 hex digits
};
// version 3: k_j = k_k + delta.  Version 4: sigma1 k''_j + d1 = +-(sigma2 k''_k + d2), sigma = +-1 (delta unused)
struct WorkLink { uint32_t j, k; i128 delta; int32_t s1 = 0, s2 = 0; i128 d1 = 0, d2 = 0; };
// versions 3 and 4, between header and table: per key a status byte (1 solved) and the key when solved, the link counters, the open links
struct WorkKeys { std::vector<uint8_t> solved; std::vector<Scalar> key; std::vector<WorkLink> links; uint64_t kept = 0, resolved = 0; };
struct WorkFile {
    WorkHeader h;
    WorkKeys keys;
    std::vector<uint8_t> table;                    // 32 bytes per entry
    std::vector<std::vector<uint8_t>> herds;       // per engine: herd * 96 bytes (bsgs_kangaroo_state)
    std::vector<std::vector<uint32_t>> reseed;     // per engine: kangaroos waiting for a new start
};
// host_kangaroo_work.cpp.  write_work: under `tmp`, then renamed; herds by pointer: they are the large part
bool write_work(const std::string &dst, const std::string &tmp, const WorkHeader &h, const std::vector<uint8_t> &table,
                const std::vector<const std::vector<bsgs_kangaroo_state> *> &herds, const std::vector<std::vector<uint32_t>> &reseed, const WorkKeys *keys = nullptr);
// "" when the file is a complete work file of version `want` (0: of any version), else what is wrong with it; with_body = false reads the header and checks
// the sections' sizes only
std::string read_work(const std::string &path, WorkFile &w, bool with_body, uint32_t want);
// SHA-1 over what a resumed run must share with the run that saved: one key (versions 1 and 2), a list (versions 3 and 4)
std::string kangaroo_fingerprint(const Affine &P, const Scalar &lo, const Scalar &hi, const WorkHeader &h);
std::string keys_fingerprint(const std::vector<Affine> &P, const Scalar &lo, const Scalar &hi, const WorkHeader &h);

// what the -selftest kangaroo* items share: the range (width below 2^128) and the comma-separated public keys of a command line, the work file a round trip
// goes through (a temporary one, or BSGS_SELFTEST_WORK to write and keep; "" when none can be made), a scripted record split at its commas
bool parse_pubs(const std::string &csv, std::vector<Affine> &pubs);
bool parse_range_pubs(const std::string &pk, const std::string &pke, const std::string &csv, Scalar &lo, Scalar &hi, u128 &W, std::vector<Affine> &pubs);
std::string selftest_work_path(bool &keep);
std::vector<std::string> split_commas(const std::string &rec);
}  // namespace kang

int kangaroo_multi_main(const kang::KangConfig &c);      // host_kangaroo_multi.cpp: -kangaroo -infile
int kangaroo_symlist_main(const kang::KangConfig &c);    // host_kangaroo_symlist.cpp: -kangaroo -infile -kwalk sym
int kangaroo_tames_main(const kang::KangConfig &c);      // host_kangaroo_tames.cpp: -kangaroo -ktamesgen, -kangaroo -ktames
