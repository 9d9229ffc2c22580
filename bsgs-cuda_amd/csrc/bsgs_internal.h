// bsgs_internal.h -- private to libbsgs_hip.so: the device object shared by its translation units.
#pragma once
#include "giant_kernel.hip.h"
#include "../../include/bsgs_hip.h"
#include <cstring>
#include <string>
#include <vector>

int bsgs_fail(int code, const char *fmt, ...);
#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) return bsgs_fail(BSGS_ERR_HIP, "%s -> %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define fail bsgs_fail

#define KANG_ROUTE_HEADER 256u                              // the outbox of a sharded distinguished-point table: 16 counts and 16 cursors (u64), then records
#define KANG_REC_HEADER 64u                                 // a record buffer (the walk's rec, the match's tames_rec): u64 count of records, then records from byte 64

// kangaroo.hip: the herd, its scratch, jump table and record buffer; kangaroo_seed.hip: the comb table, the staging of a seed call and the key list;
// kangaroo_verify.hip: the one Q of a call and the list of failures; kangaroo_tames.hip: the tame table's image and the buffer of matched records;
// kangaroo_tames_gen.hip: the table that grows during generation, whose handed-back records share the matched records' buffer; kangaroo_tames_extend.hip: its load and sorted read;
// kangaroo_dptable.hip: the distinguished-point table of a search with its own buffer of hand-backs (both tables: KangTable); kangaroo_dptable_keys.hip: its insert for a key list;
// kangaroo_dptable_shard.hip: its insert for one shard of a table divided over engines, with the outbox of the records that belong to other shards
// the table in device memory (kangaroo_table.hip.h has the rule): tag[slots] (0 = empty), the offset of each, its owner (kangaroo, type; null for the tame
// table), eight counters.  It exists where tag is set; slots is a power of two
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
struct KangTable {
    u64 *tag = nullptr;
    u32x4 *d = nullptr;
    u32x2 *who = nullptr;
    u64 *ctr = nullptr;
    uint64_t slots = 0;
};

struct bsgs_kangaroo {
    u32x4 *st = nullptr, *chain = nullptr, *table = nullptr, *staging = nullptr;
    u32 *flags = nullptr, *rec = nullptr, *idx = nullptr;
    uint8_t *rec_host = nullptr;
    uint32_t N = 0, G = 0, T = 0, block = 0, dp = 0, cap = 0, staging_n = 0;
    u32x4 *comb = nullptr;                 // 16 x 255 affine points v * 2^(8k) * G, x || y (64 bytes each): built at the first seed call
    u32x4 *seed_in = nullptr;              // one chunk of a seed call: offsets [cap] | flags [cap] | index list [cap]
    u32x4 *seed_z = nullptr;               // the chunk's Jacobian Z, [2][cap]
    u32 *seed_out = nullptr;               // {kangaroos at infinity, lowest position of one}
    uint32_t seed_cap = 0;
    u32x4 *mark = nullptr;                 // bsgs_kangaroo_setup_sym: the cycle check's marks, [2][N]
    uint32_t R = 0;                        // bsgs_kangaroo_setup_sym: jump points of the symmetric walk (0: the plain walk)
    u32 *key = nullptr;                    // bsgs_kangaroo_setup_sym_keys: the key of each kangaroo, [N], = flags + N (nullptr for every other herd)
    u32x4 *keys = nullptr;                 // bsgs_kangaroo_set_keys: n_keys affine points Q_k, x || y (64 bytes each)
    uint32_t n_keys = 0;
    u32x4 *verify_q = nullptr;             // bsgs_kangaroo_verify*: the call's one Q, x || y (64 bytes)
    u32 *verify_out = nullptr;             // {positions that failed, then the first verify_cap of them}
    uint32_t verify_cap = 0;
    u32x4 *tames = nullptr;                // bsgs_kangaroo_tames_install: the image, tames_lines lines of 64 bytes (a power of two), tames_n entries
    u32 *tames_rec = nullptr;              // the records of a launch that matched, laid out as rec
    uint64_t tames_lines = 0, tames_n = 0;
    KangTable gen;                         // bsgs_kangaroo_tames_gen_begin: the tame table that grows during generation (no owners)
    KangTable dpt;                         // bsgs_kangaroo_dptable_begin: the distinguished-point table of a search
    u32 *dpt_out = nullptr;                // its hand-backs of a launch: u64 places taken, u64 records handed back | 2 * cap records from byte 64
    bool dpt_keyed = false;                // bsgs_kangaroo_dptable_begin_keys: who[s].y is the work file's owner word (0 tame, 1 + key, bit 31 NEG), not a type
    uint32_t dpt_shards = 0, dpt_shard = 0, dpt_base = 0;      // bsgs_kangaroo_dptable_begin_shard: shard dpt_shard of dpt_shards (0: the table is not divided), ids = dpt_base + local
    u32 *dpt_route = nullptr;              // its outbox: u64 hist[16], u64 cursor[16] | cap records from byte KANG_ROUTE_HEADER, grouped by destination
};

struct bsgs_dev {
    int id = 0;
    hipStream_t stream = nullptr;          // the engine's main stream: uploads, relayouts, tile launches (part 0 of a split launch), read-backs
    // Launch overlap (bsgs_hip.hip enqueue_common): a launch of 2 x BSGS_TILE_CHUNK tiles or more goes out as two kernels with disjoint scratch, part 0 on `stream`, part 1 on
    // `stream_b`, so that one part's blocks fill the slots the other's ramp and tail leave idle; the centres of the queued tiles are made on `stream_cen`, which never
    // waits behind a tile kernel.  BSGS_LAUNCH_OVERLAP=0: one kernel per launch, everything on `stream`.
    hipStream_t stream_b = nullptr, stream_cen = nullptr;
    hipEvent_t ev_cen = nullptr, ev_a = nullptr, ev_b = nullptr;      // ordering only (no timing): centres ready; `stream` / `stream_b` reached this point
    bool overlap = true;                   // BSGS_LAUNCH_OVERLAP
                                           // (the synchronous calls bsgs_run / bsgs_run_walk never split: their launch is collected at once, and two kernels that start together
                                           // on an idle GPU ramp and end together: 146.4 against 145.4 ms, profiles/r13a_lone_launches.log)
    uint32_t split_n0 = 0;                 // first tile of part 1 in the most recent launch; 0 = that launch was one kernel on `stream` (nothing newer runs on `stream_b`)
    uint32_t last_split = 0;               // the same, kept across bsgs_collect (test library: bsgs_debug_last_split)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    unsigned debug_flags = 0;
    bool phase_probe = false;
    unsigned block_size = 256;             // threads per workgroup of the tile kernel (four waves: one Fermat inversion per block)
    hipDeviceProp_t prop;
    // geometry
    uint32_t t = 0, b = 0, p = 0;          // the caller's geometry (file layout, hit index i = tid*p + j)
    uint64_t T = 0, maxnonce = 0;
    uint32_t Ti = 0, pi = 0;               // the engine's own: Ti threads x pi giants per inversion, Ti*pi = maxnonce
    uint64_t chain_bytes = 0;              // size of the chain scratch
    // pair-batched kernel, one stream: the scratch in separately allocated, graded pieces of 2^chain_piece_log tiles (ensure_chain)
    std::vector<u32x4 *> chain_pieces;
    uint32_t chain_piece_log = 0;
    uint64_t chain_piece_bytes = 0;
    uint32_t chain_graded = 0, chain_rejected = 0;      // pieces graded / handed back by the last graded allocation
    std::vector<void *> group0_reserve;                 // big tables: pieces of the grader's memory group held back for the chain scratch
    uint64_t group0_piece_bytes = 0;
    uint32_t group0_graded = 0; float group0_grade_lo = 0.f, group0_grade_hi = 0.f;
    unsigned long long *grade_idx = nullptr, *grade_out = nullptr;   // the grader's index / output streams (kept for the engine's life: grades are relative to them)
    hipEvent_t grade_ea = nullptr, grade_eb = nullptr;
    uint32_t chain_from_reserve = 0;
    uint32_t chain_separated = 0;                       // the last graded allocation saw two classes (a piece >= 5 % below the best); 0 = the grades carried no information
    std::vector<float> chain_grades;                    // every grade of the last graded allocation, kept pieces first
    float chain_grade_best = 0.f, chain_grade_worst = 0.f;   // grade (G gathers/s) of the best / worst piece kept
    uint32_t chain_pad = 0;                       // extra u32x4 elements between the scratch areas of consecutive tiles
    std::vector<void *> pending_dev, pending_pinned;   // per-enqueue centre buffers, released by bsgs_collect
    // buffers
    u32x4 *g2 = nullptr;        // [p][4][T]
    // The same giants dealt to MORE threads with shorter batches (giant i = thread * pi + slot for every factorisation Ti * pi = maxnonce, so hit
    // indices do not change): built on demand for launches of so few tiles that the default batching leaves most of the GPU idle -- the reference's own
    // pattern is ONE tile per launch (1_9_7File.pb:2442-2459).  `narrow_off`: BSGS_NARROW_LAUNCHES=0 (A-B), or a layout that did not fit once.
    struct Batching { uint32_t Ti = 0, pi = 0; u32x4 *g2 = nullptr; };
    std::vector<Batching> narrow;
    bool narrow_off = false;               // this geometry's narrow copies did not fit once (reset by set_geometry / a table change)
    bool narrow_env_off = false;           // BSGS_NARROW_LAUNCHES=0
    uint32_t last_Ti = 0, last_pi = 0;     // batching of the last tile launch (bsgs_debug_last_batching)
    uint32_t tiles_per_block = 2;          // BSGS_TILES_PER_BLOCK: 2 = two tiles per block of the quad-chain kernel where a launch allows it (launch_tiles), 1 = never
    uint32_t last_tpb = 1;                 // tiles per block of the last tile launch (bsgs_debug_last_tiles_per_block)
    u32x4 *chain = nullptr;     // one-buffer scratch: [tile][p][2][T] (per-giant kernel) or the chained kernel's layout when not in pieces
    u32 *csr = nullptr;         // htGPU image
    bool csr_owned = true;
    u32x4 *lines = nullptr;
    bool lines_owned = true;    // false: lines / ovf were handed over by bsgs_install_table_ext_device (borrowed)
    u64 *ovf = nullptr;         // "lines + overflow list" formats (no CSR on the device): hash set of (bucket << 32 | hash)
    uint64_t ovf_n = 0;         // slots (power of two)
    bool bound_copies = true;   // the set holds a COPY of every over-full (and exactly full) line's last word: the direct builder's convention, assumed for tables installed from outside;
                                // false: made from an htGPU image (the line holds real entries only).  Only the census' duplicate count depends on it.
    uint64_t ht_items = 0, w = 0, lines_bytes = 0, overflow = 0;
    uint32_t bucket_mul = 0;    // 0: ht_items is a power of two, bucket = x & (ht_items - 1); else = ht_items: any number of buckets, bucket from 48 bits of the key (giant_kernel.hip.h bucket_mul48; extended tables, 128-byte lines)
    uint32_t layout = 0;        // probe layout: 1 csr, 2 lines64, 3 lines128 (ovf != NULL: reported as 4 / 5)
    u32 *hitbuf = nullptr;      // device
    u32 *hit_host = nullptr;    // pinned mirror
    uint32_t max_hits = 1u << 16;
    uint32_t queued = 0;
    uint32_t tiles_per_launch = 0;         // 0 = automatic (fill the chip: Ti * tiles >= 1024 threads per CU)
    uint32_t auto_tpl = 0;                 // the automatic choice, made once the giants and the table are resident (memory permitting: 4x)
    uint64_t launches = 0;
    int variant = 13;           // BSGS_KERNEL_VARIANT (A-B and tests; all bit-identical): 13 (default) = chained kernel, one stored product per FOUR giants, one probe
                                // in flight per wave (falls back to 10 when the engine's batch length is not a multiple of 4); 10 = one stored product per PAIR, two
                                // probes in flight; 0 = the per-giant kernel (also taken for the CSR layout and for odd batch lengths)
    bool timing_open = false;
    // tile centres of the queued launches, device + pinned staging (grow-only; replaced buffers wait in pending_* for bsgs_collect)
    fe *cen_dev = nullptr;
    uint8_t *cen_pin = nullptr;
    uint64_t cen_cap = 0;                  // tiles
    // device-side tile walk (bsgs_set_walk): P_k = P0 + k*D ; table = affine 2^j * D, j = 0..63
    bool walk_set = false;
    fe walk_p0x, walk_p0y;
    fe *walk_table = nullptr;
    // flags (bsgs_set_flags)
    uint32_t flags = 0;
    u32 *quirk_list = nullptr;             // device: giants whose Gy trips the reference's NEGMODP (BSGS_FLAG_REFERENCE_QUIRKS)
    std::vector<uint32_t> quirk_host;      // the same, sorted, for the hit filter of bsgs_collect
    bool quirk_ready = false;
    u64 *digest = nullptr;                 // bsgs_run_digest: [tile][Ti][2]
    uint64_t digest_bytes = 0;
    // receive buffers of an extended table that arrives by broadcast (bsgs_alloc_table_ext_recv): allocated like the engine's own
    // (bsgs_lines_malloc: tables above 40 GiB get a memory group reserved for the chain scratch), owned by the engine
    void *recv_lines = nullptr, *recv_ovf = nullptr;
    const char *last_kernel = "";          // the tile kernel instantiation of the most recent launch (bsgs_debug_last_kernel)
    bsgs_kangaroo *kangaroo = nullptr;     // bsgs_kangaroo_setup: independent of giants and table
};

// the big, long-lived device buffers (bucket lines, chain scratch, giants).  BSGS_CONTIGUOUS=1: ask for physically contiguous
// memory first (hipDeviceMallocContiguous), plain hipMalloc when that is refused.
hipError_t bsgs_big_malloc(void **p, size_t bytes);
hipError_t bsgs_big_free(void *p);                           // releases what bsgs_big_malloc / bsgs_lines_malloc / the piece allocators handed out (hipMalloc'ed or chunk-mapped)
hipError_t bsgs_lines_malloc(bsgs_dev *d, void **out, size_t bytes);       // bucket lines: the candidate in the gather-slow memory class (bsgs_hip.hip)
// placement.hip
void free_chain_pieces(bsgs_dev *d);                        // the graded pieces of the chain scratch
void free_reserve(bsgs_dev *d);
void trim_reserve(bsgs_dev *d, size_t keep);                // ... all but `keep` pieces of it                             // the memory group held back for the scratch of a large table
void release_grader(bsgs_dev *d);
void park_release(int device);                              // hand every parked piece of this device back to the driver
uint64_t parked_bytes(int device);                          // bytes this process has parked on the device
hipError_t bsgs_mem_available(size_t *avail, size_t *total);   // hipMemGetInfo of the current device + what is parked there (ours on demand)
bool alloc_graded_pieces(bsgs_dev *d, size_t npieces, uint64_t piece_bytes);     // fills d->chain_pieces; false = not enough memory
template <typename T> static inline hipError_t bsgs_big_malloc(T **p, size_t bytes) { return bsgs_big_malloc((void **)p, bytes); }

// shared between the translation units of the library
// tile_lines64.hip / tile_lines128.hip: the tile-kernel instantiations per bucket-line size (tile_launch.inc)
hipError_t bsgs_launch_tile_lines64(const TileArgs &A, dim3 grid, dim3 block, size_t lds, hipStream_t st, uint32_t group, bool dbg, const char **name);
hipError_t bsgs_launch_tile_lines128(const TileArgs &A, dim3 grid, dim3 block, size_t lds, hipStream_t st, uint32_t group, bool dbg, const char **name);
hipError_t bsgs_launch_tile_lines64_any(const TileArgs &A, dim3 grid, dim3 block, size_t lds, hipStream_t st, uint32_t group, bool dbg, const char **name);
// bsgs_hip.hip (the engine core)
void bsgs_free_table(bsgs_dev *d);
void bsgs_free_recv(bsgs_dev *d);                            // receive buffers that were never installed
int bsgs_set_geometry(bsgs_dev *d, uint32_t t, uint32_t b, uint32_t p);      // (re)allocates the giants for this geometry and picks the engine's own batching
uint32_t bsgs_chain_group(const bsgs_dev *d, uint32_t pi);   // giants per stored running product of the tile kernel a launch with batch length pi takes (4 / 2 chained, 1 per-giant)
uint32_t bsgs_auto_tiles_per_launch(const bsgs_dev *d);      // the launch size in effect
hipError_t bsgs_sync_streams(bsgs_dev *d);                   // drains the tile streams and the centres stream: before the scratch, the centres or the hit buffer change hands
// The split of a launch of n tiles into two kernels: part 0 = tiles [0, n0), part 1 = [n0, n); 0 = the launch stays one kernel.  piece_tiles = tiles per scratch piece
// (0: the scratch is one buffer), pieces = how many there are, chunk = BSGS_TILE_CHUNK, pair = the launch walks two tiles per block (both parts must be even then).
// Pieces: the piece boundary nearest n / 2, so that part 1's pieces are none of part 0's.  One buffer: n / 2, made even when n is even.
static inline uint32_t bsgs_launch_split(uint32_t n, uint32_t piece_tiles, uint32_t pieces, uint32_t chunk, bool pair)
{
    if (chunk == 0 || n < 2 * (uint64_t)chunk) return 0;
    uint32_t n0;
    if (piece_tiles) {
        if (piece_tiles < 2) return 0;                                             // pieces of one tile
        n0 = (uint32_t)(((uint64_t)(n / 2) + piece_tiles / 2) / piece_tiles * piece_tiles);
        if (n0 / piece_tiles >= pieces || ((uint64_t)n + piece_tiles - 1) / piece_tiles > pieces) return 0;
    } else {
        n0 = n / 2;
        if ((n & 1u) == 0 && (n0 & 1u)) n0++;
    }
    if (n0 == 0 || n0 >= n) return 0;
    if (pair && ((n0 | (n - n0)) & 1u)) return 0;
    return n0;
}
static inline bool bsgs_lines_layout(const bsgs_dev *d) { return d->layout == BSGS_TABLE_LINES64 || d->layout == BSGS_TABLE_LINES128; }
static inline size_t bsgs_hitbuf_bytes(const bsgs_dev *d) { return 64 + (size_t)d->max_hits * 16; }
static inline void bsgs_le_to_fe(fe &f, const uint8_t *le) { memcpy(f.v, le, 32); }
uint64_t bsgs_ovf_slots(uint64_t entries);                   // size of the overflow hash set for `entries` keys (power of two, load <= 1/2)
int bsgs_ovf_fill(bsgs_dev *d, const u64 *list, uint64_t n, u64 *table, uint64_t slots);   // table := hash set of list[0..n)
int bsgs_kangaroo_split_keys(bsgs_dev *d, const u32 *idx_dev, uint32_t first, uint32_t n);      // kangaroo.hip: flags WILD | key << 8 of the kangaroos just seeded -> flags, key[]
int bsgs_kangaroo_launch(bsgs_dev *d, uint32_t steps);     // kangaroo.hip: the three steps of bsgs_kangaroo_run, shared with bsgs_kangaroo_run_tames (kangaroo_tames.hip)
int bsgs_kangaroo_finish(bsgs_dev *d, uint64_t *count, const u32 *other, uint64_t *other_count, float *kernel_ms);
int bsgs_kangaroo_copy_out(bsgs_dev *d, const u32 *buf, uint64_t held, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *given);
void bsgs_kangaroo_release(bsgs_dev *d);                     // kangaroo.hip: frees the herd (bsgs_dev_close, a new bsgs_kangaroo_setup)
// kangaroo_tames_gen.hip: the host side of a KangTable, shared with kangaroo_tames_extend.hip and kangaroo_dptable.hip.  Texts of the caller's go into its errors.
uint64_t bsgs_kang_table_slots(uint64_t capacity, uint32_t record_cap);
void bsgs_kang_table_free(KangTable *t);
// the herd that a table call needs -> *k; `herds`: what a keyed herd is told; `begin`: what a missing table is told (null: the call needs no table)
int bsgs_kang_table_herd(bsgs_dev *d, bsgs_kangaroo **k, KangTable bsgs_kangaroo::*table, const char *herds, const char *begin);
int bsgs_kangaroo_tames_gen_herd(bsgs_dev *d, bsgs_kangaroo **k, bool table);      // ... with the growing tame table's texts
// allocate and zero: the arrays (owners: with who), *out of out_bytes where there is none; tags, counters and out's header zeroed, the stream drained, slots set.
// On an error no table is left, whatever failed (*out stays), and *nomem tells a refused allocation from a failed call
hipError_t bsgs_kang_table_begin(bsgs_dev *d, KangTable *t, uint64_t slots, bool owners, u32 **out, size_t out_bytes, bool *nomem);
int bsgs_kang_table_entries(bsgs_dev *d, const KangTable *t, uint64_t *n_entries);
// *n records of the caller's into the walk's record buffer, their count at its head, and the header of the hand-backs `out` zeroed; *n is the source of a
// copy on the stream: the caller keeps it until it has drained the stream
int bsgs_kang_table_stage(bsgs_dev *d, bsgs_kangaroo *k, u32 *out, const bsgs_kangaroo_record *recs, const uint64_t *n);
// behind the chunks of a load (e: how they went): the counters read and handed out; they must add up to n (text: n, the sum)
int bsgs_kang_table_loaded(bsgs_dev *d, const KangTable *t, hipError_t e, uint64_t n, uint64_t *n_stored, uint64_t *n_duplicate, uint64_t *n_zero, uint64_t *n_full,
                           uint64_t *n_entries, const char *text);
// behind a harvest (its caller has zeroed ctr[CTR_MET] before it): what it met against the entries counted (`what`: the table's name in the error)
int bsgs_kang_table_met_check(uint64_t met, uint64_t entries, const char *what);
// kangaroo_dptable.hip: the host side of the distinguished-point table, shared with kangaroo_dptable_keys.hip (the table for a key list) and
// kangaroo_dptable_shard.hip (the table divided over engines).  `kind`: whose calls; a table begun one way refuses the run and the insert of the others
// (BSGS_ERR_STATE), load, read and end serve all.  `rt`: where the routed records of a sharded table go (null for the other kinds)
enum { BSGS_DPT_EITHER = -1, BSGS_DPT_UNKEYED = 0, BSGS_DPT_KEYED = 1, BSGS_DPT_SHARDED = 2 };
struct DptRouted { bsgs_kangaroo_record *recs; uint32_t max; uint32_t *n; uint32_t base; };      // n[dpt_shards]; base: added to the ids of this call's records
int bsgs_kang_dpt_begin(bsgs_dev *d, uint64_t capacity, int kind);
int bsgs_kang_dpt_run(bsgs_dev *d, int kind, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, uint64_t *n_seen, uint64_t *n_entries,
                      uint64_t *dropped, float *kernel_ms, const DptRouted *rt = nullptr);
int bsgs_kang_dpt_insert(bsgs_dev *d, int kind, const bsgs_kangaroo_record *recs_in, uint32_t n, bsgs_kangaroo_record *recs_out, uint32_t max_recs, uint32_t *nrecs,
                         uint64_t *n_entries, uint64_t *dropped, const DptRouted *rt = nullptr);
int bsgs_kang_dpt_resolve(bsgs_dev *d, bsgs_kangaroo *k, uint32_t blocks);      // the resolve kernel behind an insert, on the stream
static inline uint32_t bsgs_kang_dpt_out_cap(const bsgs_kangaroo *k) { return 2u * k->cap; }      // every record of a launch a duplicate: two places each (cap <= 2^26)
// kangaroo_dptable_keys.hip: the keyed insert of the records in k->rec (their count at its head) on the stream
int bsgs_kang_dpt_insert_keys_launch(bsgs_dev *d, bsgs_kangaroo *k, uint32_t blocks);
// kangaroo_dptable_shard.hip: the sharded insert and the scatter of the foreign records in k->rec on the stream, ids = base + the record's; and, once the
// stream has drained, the routed groups -> rt (cut at rt->max; *cut = records that did not fit)
int bsgs_kang_dpt_insert_shard_launch(bsgs_dev *d, bsgs_kangaroo *k, uint32_t blocks, uint32_t base);
int bsgs_kang_dpt_routed_out(bsgs_dev *d, bsgs_kangaroo *k, uint64_t held, const DptRouted *rt, uint64_t *cut);
// hand a finished "lines + overflow list" table to the engine (it becomes the owner of both buffers)
int bsgs_install_lines(bsgs_dev *d, u32x4 *lines, int lplog, u64 *ovf, uint64_t ovf_n, uint64_t ht_items, uint64_t w,
                       uint64_t overflow_buckets);


// startup.hip: the fabric between the engines of one process -- RCCL over xGMI (dlopen'ed on first use) or direct peer copies
struct bsgs_fabric;
int bsgs_fabric_open(bsgs_fabric **f, bsgs_dev *const *devs, int n, uint32_t transport);      // transport: BSGS_TRANSPORT_*
void bsgs_fabric_close(bsgs_fabric *f);
const char *bsgs_fabric_name(const bsgs_fabric *f);
int bsgs_fabric_is_rccl(const bsgs_fabric *f);
int bsgs_fabric_broadcast(bsgs_fabric *f, void *const *bufs, size_t bytes, int root);          // bufs[i] on engine i; every engine's stream drained on return
int bsgs_fabric_allgather(bsgs_fabric *f, void *const *bufs, size_t slice_bytes);              // in place: engine i's slice number i is there already
