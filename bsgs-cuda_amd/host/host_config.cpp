// host_config.cpp -- the reference's command line (getprogparam 1_9_7File.pb:875-1042), its -w / -htsz limits (4412-4472), the configuration fingerprint and the
// checkpoint file (saveCurentCNT 3897-3931).
#include "host.h"

// ---- SHA1 (configuration fingerprint of currentwork.txt, 1_9_7File.pb:4635-4636) -------------------------------
std::string sha1_hex(const std::string &msg)
{
    uint32_t h[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};
    std::string m = msg;
    const uint64_t bits = (uint64_t)msg.size() * 8;
    m.push_back((char)0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 7; i >= 0; i--) m.push_back((char)(bits >> (8 * i)));
    auto rol = [](uint32_t v, int s) { return (v << s) | (v >> (32 - s)); };
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[80];
        for (int i = 0; i < 16; i++)
            w[i] = ((uint32_t)(uint8_t)m[off + 4 * i] << 24) | ((uint32_t)(uint8_t)m[off + 4 * i + 1] << 16) |
                   ((uint32_t)(uint8_t)m[off + 4 * i + 2] << 8) | (uint32_t)(uint8_t)m[off + 4 * i + 3];
        for (int i = 16; i < 80; i++) w[i] = rol(w[i - 3] ^ w[i - 8] ^ w[i - 14] ^ w[i - 16], 1);
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
        for (int i = 0; i < 80; i++) {
            uint32_t f, k;
            if (i < 20) { f = (b & c) | (~b & d); k = 0x5A827999u; }
            else if (i < 40) { f = b ^ c ^ d; k = 0x6ED9EBA1u; }
            else if (i < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8F1BBCDCu; }
            else { f = b ^ c ^ d; k = 0xCA62C1D6u; }
            const uint32_t t = rol(a, 5) + f + e + k + w[i];
            e = d; d = c; c = rol(b, 30); b = a; a = t;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
    }
    char out[41];
    snprintf(out, sizeof out, "%08x%08x%08x%08x%08x", h[0], h[1], h[2], h[3], h[4]);
    return out;
}

[[noreturn]] void die(const std::string &msg)
{
    fprintf(stderr, "%s\n", msg.c_str());
    exit(1);
}
std::string cut_hex(std::string s)
{
    if (s.size() >= 2 && s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) s = s.substr(2);
    for (auto &c : s) c = (char)tolower(c);
    return s;
}

void usage(const Config &c)
{
    printf(" -t      Number of GPU threads, default %u\n -b      Number of GPU blocks, default %u\n -p      Number of pparam, default %u\n"
           " -d      Select GPU IDs, default all\n-pb      Set single uncompressed/compressed pubkey for searching\n"
           "-pk      Range start from , default %s\n-pke     End range \n-w       Set number of baby items 2^ or decimal representation\n"
           "-htsz    Set number of HashTable 2^ , default %u\n-infile  Set file with pubkey for searching in uncompressed/compressed  format (search sequential)\n"
           "-wl      Set recovery file from which the state will be loaded\n-wt      Set timer for autosaving current state, default every %dseconds\n"
           "-onlygen Generate the table files and exit (onlygen_1_9_6File0.exe)\n-cpugen  Build missing table / giants files on the host CPU; with -onlygen no GPU is touched (the reference`s CPU-only generator)\n-dir     Directory for table files, currentwork.txt and win.txt\n"
           "-ext     Extended baby table built in GPU memory (no HT files); automatic for -w above the reference limit, up to 2^36\n"
           "-noverify    Skip the verification before the search (census of the table, sampled k*G and giants on every GPU; several GPUs: replicas compared)\n"
           "-refquirks   Reproduce the reference kernel's -Gy borrow bug bit for bit (default: correct arithmetic, finds a superset)\n"
           "-hostcentres Add the tile centres on the host and upload them (default: derived on the GPU from the tile counter)\n"
           "-tune        Time a few placements of the GPU buffers at start-up and keep the fastest (the engine already places them by grade)\n"
           "-startup     Several GPUs: broadcast (GPU 0 holds the table, the others receive it over xGMI), local (every GPU builds / uploads its own),\n"
           "             allgather (extended tables: every GPU builds 1/N of the bucket lines, then all-gather); default: local for extended tables, else broadcast\n"
           "-transport   Several GPUs: rccl | peer (direct peer copies) | auto (RCCL when the GPUs are distinct and librccl loads)\n"
           "-lanes       -infile: public keys searched side by side, each on an engine of its own per GPU (default: 2 when a job is only a launch or two long, else 1)\n"
           "-w auto      The table Tune picks for the range given: the one that minimises table build + worst-case search (a 64-bit range: -w 30 -ext)\n"
           "-buckets     Extended table: the number of buckets itself (any number below 2^32; 64-byte lines up to 12.5 items per bucket, else 128-byte lines), e.g. -w 35 -buckets 3221225472\n",
           c.t, c.b, c.p, c.pk.c_str(), c.htsz, c.wt);
    printf("-kangaroo    Pollard's kangaroo search of a public key (-pb), or of every key of a list (-infile) with one herd, in [-pk, -pke], 2^20 <= width <= 2^125, no baby table; with -d, -dir, -wl, -wt (not with -w -htsz -onlygen;\n"
           "             -infile: not with -pb, -ksym; saved as kangaroo.work version 3, which only -infile -wl continues)\n"
           "-kwalk W     Kangaroo: plain (default) or sym, the symmetric walk (negation map): with -pb the same as -ksym, with -infile the list search with that walk (kangaroo.work version 4)\n"
           "-dp N        Kangaroo: distinguished points have the top N bits of x zero (0..32; default chosen from the range)\n"
           "-kn N        Kangaroo: kangaroos per engine (default chosen from the range)\n"
           "-kseed S     Kangaroo: seed of the herds and the jump table (default: random, printed)\n"
           "-wt N        Kangaroo: the whole search (table of distinguished points, herds, counters) is saved to <dir>/kangaroo.work every N seconds (default 180, at least 30),\n"
           "             and once more when the run stops without the key; the file is removed when the key is found\n"
           "-wl FILE     Kangaroo: continue from a kangaroo.work file: same -pb -pk -pke and number of -d entries; -dp -kn -kseed are taken from the file\n"
           "-ksteps N    Kangaroo: stop once N steps were walked in total (checked after each launch), save kangaroo.work, exit code 3 (SIGINT / SIGTERM do the same)\n"
           "-noverify    Kangaroo: skip the check of every kangaroo (and, at -wl, of every saved table entry) against its offset on the GPU: at -wl before the first step, and before every save\n"
           "-kcpuseed    Kangaroo: compute the kangaroos' start points on the host CPU instead of the GPU (same herd; for cross-checks)\n"
           "-ksym        Kangaroo: the symmetric walk (negation map: P and -P are one point of the walk; wild-wild collisions solve too; cycles are retired and re-seeded)\n"
           "-kjumps R    Kangaroo -ksym: jump points, a power of two 64..4096 (default 1024)\n"
           "-kjumpscale F  Kangaroo -ksym: mean jump = F * N_k sqrt(W) / 4 (default 2)\n"
           "-kdpdev      Kangaroo -pb, plain and -ksym (one -d entry): distinguished points are kept and paired in GPU memory; only collisions, dead kangaroos and cycles cross the bus,\n"
           "             so the default plan is a low -dp and the full herd; kangaroo.work is the same file with and without the flag (not with -infile, -ktames*, -ktamesgen);\n"
           "             without -d it runs on GPU #0; every save (-wt, and the last) reads the whole table: 32 bytes per entry of GPU memory for the read and of host memory for the file\n"
           "-kdpshard    Kangaroo -pb, plain and -ksym: -kdpdev's table divided over the engines of -d by tag, each share kept and paired in its engine's GPU memory; records that belong to\n"
           "             another engine's share are relayed to it (without -d: every GPU; -d 0,0 runs two engines on one GPU; -kdpn: entries per engine; kangaroo.work is the plain\n"
           "             multi-engine file, resumable with and without the flag on the same number of -d entries; not with -kdpdev, -kdpkeys, -infile, -ktames*)\n"
           "-kdpn N      Kangaroo -kdpdev / -kdpkeys / -kdpshard: entries the table in GPU memory is sized for, 1..2^31, 64 bytes each (default: the power of two at or above 4 sqrt(width), 2^16..2^27;\n"
           "             -kdpkeys: 4 sqrt(open keys x width))\n"
           "-kdpkeys     Kangaroo -infile, plain and -kwalk sym (one -d entry): the list search's distinguished points are kept in GPU memory with the key that owns each and paired there;\n"
           "             only collisions, dead kangaroos and cycles cross the bus.  The plan is -kdpdev's with sqrt(open keys x width) in the place of sqrt(width); kangaroo.work is the same\n"
           "             file with and without the flag (not with -pb, -kdpdev, -ktames*, -ktamesgen; without -d it runs on GPU #0; saves read the whole table, as -kdpdev).  A search that runs\n"
           "             towards its upper end, keys x 2 sqrt(width) steps, fills the table past its plan: it takes entries up to its slots, records that find none fall to the host's own\n"
           "             table -- that costs time, never correctness; -kdpn sizes the table for such a search\n"
           "-ktamesgen F Kangaroo: make a tame table of -ktn T distinguished points of the range [-pk, -pke] and write it to F (nothing else is saved; no -wl, -wt)\n"
           "-ktn T       Kangaroo -ktamesgen: entries of the table, 1..2^31\n"
           "-ktames F    Kangaroo: search -pb or every key of -infile with the tame table F of this range: all kangaroos wild, records matched against the table on the GPU\n"
           "             (the table is verified on the GPU at load, -noverify skips; not with -ksym, -kwalk sym, -wl, -dp; nothing is saved)\n"
           "-ktamesdev   Kangaroo -ktamesgen (plain and -kwalk sym; one -d entry): the growing table is kept in GPU memory and each launch's records are inserted there; only merges,\n"
           "             dead kangaroos and cycles come back, so -kn may be raised to the full herd (the default herd stays what the range gives); the table is verified on the GPU before it is written\n"
           "-ktamesfrom F Kangaroo -ktamesgen OUT -ktamesdev -ktn T: extend the table F to T entries: dp, range, jumps and scalars come from F, its entries are loaded into GPU memory\n"
           "             and a new herd (another -kseed) walks until T are there; OUT may be F\n"
           "-ktnplan N   Kangaroo -ktamesgen: plan the walk (mean jump, default -dp) for a table of N entries, N at least -ktn: for a table that will be extended or merged later\n"
           "-ktamesmerge A,B[,C...] Kangaroo -ktamesgen OUT [-ktn T] [-kwalk sym]: merge tables of one walk by tag on the host, one entry per tag (the first table that has it);\n"
           "             -ktn keeps the T lowest tags; every entry written is verified on the first -d device unless -noverify (then no GPU is opened)\n"
           "-kwalk sym   Kangaroo -ktamesgen: the tame table of the symmetric walk (file version 2; with -kjumps, -kjumpscale: default 1024 and 1)\n"
           "-ktamessym F Kangaroo: as -ktames with a table of the symmetric walk: jump points, scale and scalars come from the file (-ktames refuses such a table, and -kwalk)\n");
}

Config parse_args(int argc, char **argv)
{
    Config c;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        for (auto &ch : a) ch = (char)tolower(ch);
        auto next = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
        if (a == "-h") { usage(c); exit(0); }
        else if (a == "-t") { c.t = (uint32_t)atoi(next().c_str()); printf("Number of GPU threads set to #%u\n", c.t); }
        else if (a == "-b") { c.b = (uint32_t)atoi(next().c_str()); printf("Number of GPU blocks set to #%u\n", c.b); }
        else if (a == "-p") { c.p = (uint32_t)atoi(next().c_str()); printf("Number of pparam set to #%u\n", c.p); }
        else if (a == "-d") { c.devices = next(); printf("Used GPU devices #%s\n", c.devices.c_str()); }
        else if (a == "-pb") { c.pub = cut_hex(next()); printf("Pubkey set to %s\n", c.pub.c_str()); }
        else if (a == "-pk") { c.pk = cut_hex(next()); printf("Range begin: 0x%s\n", c.pk.c_str()); }
        else if (a == "-pke") { c.pke = cut_hex(next()); c.pke_given = true; printf("Range end: 0x%s\n", c.pke.c_str()); }
        else if (a == "-w") {                                   // <=32: 2^value (fractional allowed), else decimal  (1009-1022)
            const std::string v = next();
            if (v == "auto" || v == "AUTO") { c.w_auto = true; printf("Items number: chosen for the range (Tune)\n"); continue; }
            const double d = atof(v.c_str());
            // the reference switches to decimal above 32; 33..36 are exponents of the extended table here
            if (d <= 36.0) { c.w = (uint64_t)std::pow(2.0, d); printf("Items number set to 2^%s=%llu\n", v.c_str(), (unsigned long long)c.w); }
            else { c.w = strtoull(v.c_str(), nullptr, 10); printf("Items number set to %llu = 2^%f\n", (unsigned long long)c.w, std::log2((double)c.w)); }
        }
        else if (a == "-htsz") {
            const std::string v = next();
            const double d = atof(v.c_str());
            c.htsz = (uint32_t)d; c.htsz_arg = c.htsz;
            if (d != std::floor(d)) {               // a fraction (as -w takes one, 1_9_7File.pb:1009-1022): extended tables may have any number of buckets
                c.htsz_arg = (uint32_t)std::llround(std::pow(2.0, d));
                printf("HT size set to 2^%s=%u buckets (extended table)\n", v.c_str(), c.htsz_arg);
            } else printf("HT size set to 2^%u\n", c.htsz);
        }
        else if (a == "-buckets") { c.htsz_arg = (uint32_t)strtoull(next().c_str(), nullptr, 10); c.htsz = 0; while ((2ull << c.htsz) <= c.htsz_arg) c.htsz++; printf("HT size set to %u buckets (extended table)\n", c.htsz_arg); }
        else if (a == "-sf") { c.file_search = atoi(next().c_str()) != 0; printf(c.file_search ? "Search in file\n" : "Search in RAM\n"); }
        else if (a == "-lanes") { c.lanes = atoi(next().c_str()); if (c.lanes < 1 || c.lanes > 4) die("-lanes 1..4"); }
        else if (a == "-startup") { c.startup = next(); for (auto &ch : c.startup) ch = (char)tolower(ch); }
        else if (a == "-transport") { c.transport = next(); for (auto &ch : c.transport) ch = (char)tolower(ch); }
        else if (a == "-infile") { c.infile = next(); printf("Will be used file: %s\n", c.infile.c_str()); }
        else if (a == "-wl") { c.recovery_file = next(); printf("Recovery work file: %s\n", c.recovery_file.c_str()); }
        else if (a == "-wt") { c.wt = std::max(30, atoi(next().c_str())); printf("Saving timer every %d seconds\n", c.wt); }
        else if (a == "-onlygen") c.onlygen = true;
        else if (a == "-cpugen") c.cpugen = true;
        else if (a == "-maxtiles") c.max_tiles = strtoull(next().c_str(), nullptr, 10);
        else if (a == "-dir") c.dir = next();
        else if (a == "-ext") c.ext = true;
        else if (a == "-refquirks") c.ref_quirks = true;
        else if (a == "-verifyreplicas") c.verify_replicas = true;
        else if (a == "-noverify") c.verify_replicas = false;
        else if (a == "-hostcentres") c.host_centres = true;
        else if (a == "-tune") c.tune = true;
        else if (a == "-joblog") c.joblog = next();
        else if (a == "-kdpdev" || a == "-kdpn" || a == "-kdpkeys" || a == "-kdpshard") die(a + " belongs to -kangaroo (the table of distinguished points of a kangaroo search, kept in GPU memory)");
        else die("Unknown parameter " + a);
    }
    // limits 1_9_7File.pb:4412-4418, 4616-4618
    if (c.w >= 3069485951ull) {                    // beyond the reference's u32 file format: extended device-resident table
        if (c.w > (1ull << 36)) die("-w must be at most 2^36");
        c.ext = true;
        printf("-w above the reference limit 3069485951: extended table in GPU memory, no HT files\n");
    }
    if (c.htsz > 31 || c.htsz < 1) die("-htsz must be 1..31");
    if (c.htsz_arg > 31) {
        if (!(c.htsz_arg & (c.htsz_arg - 1))) { c.htsz = 0; while ((1u << c.htsz) < c.htsz_arg) c.htsz++; c.htsz_arg = c.htsz; }      // a power of two after all
        else { c.ext = true; printf("%u buckets (not a power of two): extended table in GPU memory, no HT files\n", c.htsz_arg); }
    }
    if (c.startup != "auto" && c.startup != "broadcast" && c.startup != "local" && c.startup != "allgather") die("-startup: broadcast | local | allgather | auto");
    if (c.transport != "auto" && c.transport != "rccl" && c.transport != "peer") die("-transport: rccl | peer | auto");
    if (c.p & 1) die("-p must be even");
    if (!c.t || !c.b || !c.p) die("-t -b -p must be non-zero");
    return c;
}

// ---- the reference's limits on -w / -htsz for tables in ITS format (1_9_7File.pb:4412-4472): -w below 3069485951, -htsz below 32, and the "UNSAFE mode" question
// (answer Y on stdin to go on) where duplicate 32-bit values in one bucket become likely; then its warning about a -htsz that is too low.  Extended tables
// (built in GPU memory, no HT files: -ext, -w above 2^32, -buckets) are outside that format and outside these limits.  Returns "" to go on, else the exit message.
std::string table_limits(uint64_t w, uint32_t htsz, FILE *answers)
{
    if (w >= 3069485951ull) return "-w should be less or equil to 3069485951 Or 2^31.515349920643907";
    if (htsz > 31) return "-htsz should be less than 32";
    static const struct { uint32_t htsz; uint64_t limit; const char *shown; } unsafe[] = {
        {27, 1331331443ull, "1331331443 or 2^30.310222637591963"}, {28, 1777178603ull, "1777178603 Or 2^30.726941530690112"}, {29, 3069485951ull, "3069485950 Or 2^31.515349920643907"},
        {30, 3069485951ull, "3069485951 Or 2^31.515349920643907"}, {31, 3069485951ull, "3069485951 Or 2^31.515349920643907"}};
    for (const auto &u : unsafe)
        if (htsz == u.htsz && w > u.limit) {
            printf("With -htsz %u value -w should be less or equil to %s\nDue to the possibility of duplicate values in the hash table\n"
                   "It is unsafe to use values higher than those specified above\nTo continue in UNSAFE mode type Y and press ENTER\n", u.htsz, u.shown);
            fflush(stdout);
            char line[64] = {0};
            if (!answers || !fgets(line, sizeof line, answers)) return " ";
            std::string ans(line);
            while (!ans.empty() && (ans.back() == '\n' || ans.back() == '\r')) ans.pop_back();
            if (ans != "Y") return " ";
        }
    const int need = (int)std::floor(std::log2((double)w)) - (int)htsz;
    if (need > 3) printf("WARNING! -htsz parametr is to low, should be at least %d\n", (int)std::floor(std::log2((double)w)) - 2);
    return "";
}

// ---- checkpoint: saveCurentCNT 1_9_7File.pb:3897-3931 ------------------------------------------------------------
std::string fingerprint(const Config &c)
{
    std::ostringstream s;
    s << c.t << c.b << c.p << c.w << c.pk << c.pke << (c.htsz_arg > 31 ? c.htsz_arg : c.htsz);     // Str(t)+Str(b)+Str(p)+Str(w)+pk+pke+Str(htsz)  (4635-4636); a bucket count stands for htsz
    return sha1_hex(s.str());
}
// the minimum counter over the GPUs' unfinished batches (a restart re-does at most the batches in flight); both locks are
// held so that a batch cannot leave the dispenser between reading its counter and reading the in-flight table
Scalar Job::checkpoint_counter()
{
    std::lock_guard<std::mutex> lk(job_mutex);
    std::lock_guard<std::mutex> lk2(inflight_mutex);
    Scalar cnt = glob_key;
    for (size_t g = 0; g < inflight.size(); g++) if (inflight_valid[g] && hs::fe_cmp(inflight[g], cnt) < 0) cnt = inflight[g];
    if (joblog) { fprintf(joblog, "save %s\n", hs::fe_to_hex(cnt).c_str()); fflush(joblog); }
    return cnt;
}
// (the product saves only under the JobList's mutex)
void save_checkpoint(const Config &c, int listpos, const std::string &pub_hex, const Scalar &cnt)
{
    const std::string tmp = c.dir + "/currentwork.temp", dst = c.dir + "/currentwork.txt";
    {
        std::ofstream f(tmp, std::ios::binary);
        f << listpos << "\r\n" << pub_hex << "\r\n" << hs::fe_to_hex(cnt) << "\r\n" << fingerprint(c) << "\r\n";
    }
    rename(tmp.c_str(), dst.c_str());
}
