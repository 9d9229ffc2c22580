// host_selftest.cpp -- -selftest: the host-side logic that needs no GPU (CPU test tier, tests/test_host_logic.py).
#include "host.h"

// JobList driven by a script, no GPU and no threads: N [wl=POS:HEXCNT] [won=P,P...] then events c<lane> (claim), p<lane> (publish: a Job of the claimed key
// seeded from its start counter), t<lane> (the published job dispenses 3 tiles and finishes them), f<lane> (finish).  Keys are 1*G .. N*G, two lanes.
// Prints "claim <lane> <pos> <resumed>" / "claim <lane> none", "emit <pos>" in the order the list emits, "save <pos> <pubkey> <counter>" for every checkpoint.
static int selftest_joblist(const std::vector<std::string> &a)
{
    const int n = atoi(a[0].c_str());
    Recovery rec;
    std::vector<std::string> pubs;
    for (int k = 1; k <= n; k++) pubs.push_back(pub_hex(hs::point_mul(hs::G, hs::fe_from_u64((uint64_t)k))));
    Run R;
    R.cfg.t = 64; R.cfg.b = 8; R.cfg.p = 16; R.cfg.w = 65536;
    derive_constants(R);
    size_t e = 1;
    for (; e < a.size() && a[e].find('=') != std::string::npos; e++) {
        const std::string v = a[e].substr(a[e].find('=') + 1);
        if (a[e].rfind("wl=", 0) == 0) { rec.on = true; rec.pos = atoi(v.c_str()); rec.cnt = v.substr(v.find(':') + 1); if (rec.pos < 1 || rec.pos > n) return 2; rec.pub = pubs[(size_t)rec.pos - 1]; }
        else if (a[e].rfind("won=", 0) == 0) { std::stringstream ss(v); std::string tok; while (std::getline(ss, tok, ',')) rec.won.insert(atoi(tok.c_str())); }
        else return 2;
    }
    JobList jobs(pubs, rec, "/nonexistent", [](int pos, const std::string &pub, const Scalar &cnt) { printf("save %d %s %s\n", pos, pub.c_str(), hs::fe_to_hex(cnt).c_str()); });
    jobs.open_lanes(2);
    JobList::Claim claimed[2];
    std::unique_ptr<Job> job[2];
    for (; e < a.size(); e++) {
        const char ev = a[e][0];
        const size_t l = (size_t)atoi(a[e].c_str() + 1);
        if (a[e].size() != 2 || l > 1 || (ev == 'c') == (claimed[l].listpos > 0) || (ev == 't' && !job[l])) return 2;      // (a script the list would never see)
        if (ev == 'c') {
            if (!jobs.claim(l, claimed[l])) { claimed[l] = JobList::Claim(); printf("claim %zu none\n", l); }
            else printf("claim %zu %d %d\n", l, claimed[l].listpos, claimed[l].resumed ? 1 : 0);
        } else if (ev == 'p') {
            Affine q; hs::parse_pubkey(q, jobs.pub(claimed[l].listpos));
            Scalar key0 = hs::fe_from_u64(1);
            if (claimed[l].resumed) hs::fe_from_hex(key0, rec.cnt);
            job[l].reset(new Job(R, claimed[l].listpos, q, q, key0, 1, nullptr));
            jobs.publish(l, *job[l]);
        } else if (ev == 't') {
            std::vector<Tile> tiles;
            get_jobs(*job[l], 3, tiles, 0);
            job[l]->inflight_valid[0] = false;
        } else if (ev == 'f') {
            jobs.finish(l, "emit " + std::to_string(claimed[l].listpos) + "\n", false, "");
            job[l].reset(); claimed[l] = JobList::Claim();
        } else return 2;
    }
    return 0;
}

// ---- -selftest: the host-side logic that needs no GPU (CPU test tier, tests/test_host_logic.py) ------------------------
// prints "key value" lines: SHA1, the configuration fingerprint, host EC arithmetic, public-key parsing, the dispenser
// sequence and the table-free resolver, each for the inputs given on the command line
int selftest(int argc, char **argv)
{
    std::vector<std::string> a(argv + 2, argv + argc);
    auto pt = [](const Affine &q) { return q.inf ? std::string("inf") : hs::fe_to_hex(q.x) + " " + hs::fe_to_hex(q.y); };
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i] == "sha1" && i + 1 < a.size()) printf("sha1 %s\n", sha1_hex(a[++i]).c_str());
        else if (a[i] == "fingerprint") {
            Config c; c.t = 256; c.b = 88; c.p = 130; c.w = 982162051; c.pk = "8000000000000000"; c.pke = "ffffffffffffffff"; c.htsz = 28;
            printf("fingerprint %s\n", fingerprint(c).c_str());
        } else if (a[i] == "mul" && i + 1 < a.size()) {
            Scalar k; if (!hs::fe_from_hex(k, a[++i])) return 2;
            printf("mul %s\n", pt(hs::point_mul(hs::G, k)).c_str());
        } else if (a[i] == "parse" && i + 1 < a.size()) {
            Affine q; const bool ok = hs::parse_pubkey(q, cut_hex(a[++i])) && hs::on_curve(q);
            printf("parse %s %s\n", ok ? pt(q).c_str() : "invalid", ok ? hs::compress_pubkey(q).c_str() : "");
        } else if (a[i] == "multiples" && i + 2 < a.size()) {                 // n multiples of k*G through the batched normalisation
            Scalar k; if (!hs::fe_from_hex(k, a[++i])) return 2;
            const size_t n = (size_t)atoi(a[++i].c_str());
            const std::vector<Affine> v = hs::multiples(hs::point_mul(hs::G, k), n);
            printf("multiples %s\n", pt(v.back()).c_str());
        } else if (a[i] == "jobs" && i + 5 < a.size()) {                     // dispenser: t b p w n -> counters and centres of n tiles
            Run R;
            R.cfg.t = (uint32_t)atoi(a[i + 1].c_str()); R.cfg.b = (uint32_t)atoi(a[i + 2].c_str()); R.cfg.p = (uint32_t)atoi(a[i + 3].c_str());
            R.cfg.w = strtoull(a[i + 4].c_str(), nullptr, 10);
            const size_t n = (size_t)atoi(a[i + 5].c_str());
            Affine pub; if (!hs::parse_pubkey(pub, cut_hex(a[i + 6])) ) return 2;
            i += 6;
            derive_constants(R);
            Job J(R, 1, pub, pub, hs::fe_from_u64(1), 0, nullptr);
            std::vector<Tile> tiles;
            get_jobs(J, n, tiles);
            for (const Tile &t : tiles) printf("job %s %s\n", hs::fe_to_hex(t.key).c_str(), pt(tile_centre(J, t.index)).c_str());
        } else if (a[i] == "minibsgs" && i + 2 < a.size()) {                 // w (decimal), then hex scalars m: all b' <= w with x(b'G) = x(mG)
            const uint64_t w = strtoull(a[++i].c_str(), nullptr, 10);
            MiniBsgs mb; mb.build(w, 4);
            printf("minibsgs_bits %u\n", mb.mb);
            for (++i; i < a.size(); i++) {
                Scalar m; if (!hs::fe_from_hex(m, a[i])) return 2;
                std::string out;
                for (uint64_t b : mb.find(hs::point_mul(hs::G, m), w)) out += " " + std::to_string(b);
                printf("find %s%s\n", a[i].c_str(), out.c_str());
            }
        } else if (a[i] == "tune" && i + 1 < a.size()) {                      // free bytes -> the MI355X sizing advice (replaces Tune, 1_9_7File.pb:324-431)
            const TuneAdvice t = tune_advice(strtoull(a[++i].c_str(), nullptr, 10));
            printf("tune -w %.2f -htsz %u ext %d -w %u -htsz %u\n", t.w_log2, t.htsz, t.ext ? 1 : 0, t.ext_w_log2, t.ext_htsz);
        } else if (a[i] == "plan" && i + 3 < a.size()) {                      // free bytes, range bits, GPUs -> the table Tune picks for that range
            const uint64_t fr = strtoull(a[i + 1].c_str(), nullptr, 10);
            const TunePlan pl = tune_plan(fr, atof(a[i + 2].c_str()), atoi(a[i + 3].c_str()), 1ull << 24);
            i += 3;
            printf("plan %s | w %.2f htsz %u ext %d build %.3f search %.3f total %.3f\n", plan_flags(pl).c_str(), pl.w_log2, pl.htsz_arg, pl.ext ? 1 : 0, pl.build_s, pl.search_s, pl.total_s);
        } else if (a[i] == "htlookup" && i + 3 < a.size()) {                 // htCPU file, htsz, then hex 64-bit keys: positions found in RAM and by the two reads of -sf 1
            const std::string path = a[i + 1];
            const uint64_t items = 1ull << atoi(a[i + 2].c_str());
            struct stat st; if (stat(path.c_str(), &st) != 0) return 2;
            HostBuf img; if (!read_file(path, img, (uint64_t)st.st_size)) return 2;
            const int fd = open(path.c_str(), O_RDONLY); if (fd < 0) return 2;
            for (i += 3; i < a.size(); i++) {
                const uint64_t k = strtoull(a[i].c_str(), nullptr, 16);
                uint32_t p1[64], p2[64];
                const int n1 = htcpu_lookup(img, items, k, p1, 64), n2 = htcpu_lookup_file(fd, items, k, p2, 64);
                std::string o1, o2;
                for (int q = 0; q < std::min(n1, 64); q++) o1 += " " + std::to_string(p1[q]);
                for (int q = 0; q < std::min(n2, 64); q++) o2 += " " + std::to_string(p2[q]);
                printf("htlookup %s ram%s | file%s\n", a[i].c_str(), o1.c_str(), o2.c_str());
            }
            close(fd);
        } else if (a[i] == "limits" && i + 2 < a.size()) {                    // w (decimal), htsz: the reference's -w / -htsz limits and UNSAFE question (answer on stdin)
            const std::string m = table_limits(strtoull(a[i + 1].c_str(), nullptr, 10), (uint32_t)atoi(a[i + 2].c_str()), stdin);
            i += 2;
            printf("limits %s\n", m.empty() ? "ok" : m == " " ? "exit" : m.c_str());
        } else if (a[i] == "checkpoint" && i + 1 < a.size()) {                // next counter, then in-flight counters ("-" = idle GPU): the saved one
            Run R;
            R.cfg.dir = "/tmp";
            Scalar next;
            if (!hs::fe_from_hex(next, a[++i])) return 2;
            Job J(R, 1, hs::G, hs::G, next, 0, stdout);
            for (++i; i < a.size(); i++) {
                Scalar v = hs::fe_from_u64(0);
                const bool valid = a[i] != "-";
                if (valid && !hs::fe_from_hex(v, a[i])) return 2;
                J.inflight.push_back(v); J.inflight_valid.push_back(valid);
            }
            save_checkpoint(R.cfg, J.listpos, "selftest", J.checkpoint_counter());
        } else if (a[i] == "kangaroo-work") {                               // the header of a work file (host_kangaroo_work.cpp)
            return kangaroo_work_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-table-roundtrip") {                    // the table through a work file in the middle of a record stream
            return kangaroo_roundtrip_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-dpkeys-plan") {                        // the plan of -kdpkeys from the range width and the list's length (no GPU)
            return kangaroo_dpkeys_plan_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-dpkeys") {                             // the hand-back rule of -kdpkeys on scripted records and pairs (no GPU)
            return kangaroo_dpkeys_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-barrier") {                            // -kdpshard's barrier before a save on scripted events (no GPU, no threads)
            return kangaroo_barrier_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-dpshard-plan") {                       // the plan of -kdpshard for E engines (no GPU)
            return kangaroo_dpshard_plan_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-dpshard") {                            // the hand-back rule of -kdpshard on scripted records with global ids (no GPU)
            return kangaroo_dpshard_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-dpdev-plan") {                         // the plan of -kdpdev from the range width (no GPU)
            return kangaroo_dpdev_plan_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-dpdev") {                              // the hand-back rule of -kdpdev on scripted records and pairs (no GPU)
            return kangaroo_dpdev_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-sym") {                                // the same through the symmetric walk's table
            return kangaroo_sym_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-sym-roundtrip") {
            return kangaroo_sym_roundtrip_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-symlist-roundtrip") {                  // the table of -infile -kwalk sym through a version-4 work file
            return kangaroo_symlist_roundtrip_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-symlist") {                            // the same table on a scripted record stream (host_kangaroo_symlist.cpp)
            return kangaroo_symlist_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-tames-gen") {                          // the rule of -ktamesgen -ktamesdev on scripted hand-backs (no GPU)
            return kangaroo_tames_gen_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-tames-image") {                        // the device image of a tame table (host_kangaroo_tames.cpp; no GPU)
            return kangaroo_tames_image_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-tames-search") {                       // the search rule of -ktames on scripted records
            return kangaroo_tames_search_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-tames") {                              // the header of a tame table file
            return kangaroo_tames_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-multi-roundtrip") {                    // the same through a version-3 work file in the middle of the stream
            return kangaroo_multi_roundtrip_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo-multi") {                              // the table for a list of keys on a scripted record stream (host_kangaroo_multi.cpp)
            return kangaroo_multi_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "kangaroo") {                                    // the rest of the command line: range, public key, record stream (host_kangaroo.cpp)
            return kangaroo_selftest(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else if (a[i] == "joblist" && i + 1 < a.size()) {                  // the rest of the command line is the script
            return selftest_joblist(std::vector<std::string>(a.begin() + (long)i + 1, a.end()));
        } else { fprintf(stderr, "selftest: unknown item %s\n", a[i].c_str()); return 2; }
    }
    return 0;
}
