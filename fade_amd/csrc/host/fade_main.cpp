// fade_main.cpp — the `fade` host driver: `annotate` over the fadehip C ABI, plus the host-only consumers
// `extract` (source/remap.d) and `out` (source/filter.d).
//
// Mirrors the CLI surface of the reference:
//   source/app.d:64-101   main, getopt(annotate): -t/--threads, --min-length, -w/--window-size, -b/--bam, -u/--ubam,
//                         -h/--help; `-b -u` together is an error (exit 1); < 3 args or -h prints help (exit 0)
//   source/anno.d:16-52   annotate(): warning line, open BAM/SAM + FASTA, @PG header line, per-record
//                         annotateTask, write to stdout as SAM / uBAM / BAM (source/util.d:65-76)
//   source/anno.d:94-107  tag order rs, am, as, ar, ab;  analysis.d:84-92,108-118 string contents
// The loop at anno.d:44-50 becomes read-chunk -> pack (pointers into the BAM bytes) -> fadehip_annotate_*
// -> format tags -> write: three threaded stages (reader / device+tags / writer) over two device slots.
// Additive flags: --gpus N, --batch N, --stats, --timing.
// There is no CPU alignment path in this program.
#include <memory>
#include "hts_lite.hpp"
#include "recstore_host.hpp"
#include "bed_lite.hpp"
#include "bgzf_feed.hpp"
#include "../../../include/fadehip.h"

#include <atomic>
#include <cerrno>
#include <cmath>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <deque>
#include <functional>
#include <future>
#include <sched.h>
#include <fcntl.h>
#include <spawn.h>
#include <sys/stat.h>
#include <unordered_map>
#include <sys/wait.h>
#include <unistd.h>

extern char **environ;

#ifndef FADE_VERSION
#define FADE_VERSION "v0.5.0-mi355x"
#endif

using namespace htsl;

// the driver double-buffers: two of the ctx's slots per device (one batch computes while the previous one is collected)
static size_t kSlotsInUse = 1;  // batches in flight per device: one, a second when the device falls behind (annotate_main)
static const char *kHeader = "Fragmentase Artifact Detection and Elimination\nversion: " FADE_VERSION "\n";

static void print_full_help() {
    fprintf(stderr,
            "%s\nusage: fade [subcommand]\n"
            "    annotate: marks artifact reads in bam tags (must be done first)\n"
            "    out: eliminates artifact from reads(may require queryname sorted bam)\n"
            "    stats: reports extended information about artifact reads\n"
            "    stats-clip: reports extended information about all soft-clipped reads\n"
            "    extract: extracts artifacts into a mapped bam\n\n"
            "-h --help This help information.\n\n",
            kHeader);
}

static void print_anno_help() {
    fprintf(stderr,
            "%s\nannotate: performs re-alignment of soft-clips and annotates bam records with bitflag (rs) and "
            "realignment tags (am)\nusage: fade annotate [options] <input BAM/SAM> <Indexed fasta reference>\n\n"
            "-t     --threads extra threads for parsing the bam file\n"
            "    --min-length Minimum number of bases for a soft-clip to be considered for artifact detection\n"
            "-w --window-size Number of bases considered outside of read or mate region for re-alignment\n"
            "-b         --bam output bam\n"
            "-u        --ubam output uncompressed bam\n"
            "-c        --clip hard-clip the artifacts in the same pass (what `fade out -c` makes of the annotated file)\n"
            "        --extract PATH: also write what `fade extract` makes of the annotated file (one mapped record per artifact side), in the same pass\n"
            " --extract-sorted with --extract PATH, BAM file in, -b or -u out, one MI355X: PATH is written in coordinate order (@HD SO:coordinate), and its index PATH.bai beside it\n"
            "          --eject drop the artifact reads in the same pass, and on name-sorted input every read that shares their name (what `fade out` makes of the annotated file)\n"
            "    --keep-sorted with -c, coordinate-sorted BAM file in, -b or -u out, one MI355X: clipped records are written at their new coordinates, so the output stays coordinate-sorted\n"
            "           --sort BAM file in, in any order, -b or -u out, one MI355X: the output is written in coordinate order (@HD SO:coordinate), sorted on the device (a file too large for it: sort in the fade out step)\n"
            "    --write-index PATH: also write the BAM index (.bai) of the output, made in the same pass (coordinate-sorted output, BAM file in, -b or -u out, one MI355X)\n"
            "            --csi with --write-index or --extract-sorted: the index is a CSI (min_shift 14, depth 5, or 6 for contigs longer than 2^29; PATH.csi beside --extract PATH)\n"
            "          --gpus number of MI355X devices, one process each on its own range of the input (default 1)\n"
            "    --out-shards with --gpus N: every device writes a complete file PREFIX.<k>.bam (.sam), nothing is merged\n"
            "         --batch records per device batch (default 262144)\n"
            "         --stats print the stats.d summary of this run to stderr\n"
            "     --stats-tsv PATH: write what `fade stats` prints for this run's output to PATH (one device)\n"
            "      --clip-tsv PATH: write what `fade stats-clip` prints for this run's output to PATH (one device)\n"
            "-h        --help This help information.\n\n",
            kHeader);
}

struct Opts {
    int threads = 0, floor_len = 5, window = 300, gpus = 1, batch = 262144;
    bool bam = false, ubam = false, help = false, stats = false, timing = false, clip = false;
    bool eject = false;  // --eject: plain `fade out` (filter.d:209-265) in the same pass
    bool fragments = false;  // `fade out --fragments`: whole fragments leave, input in any order (a set of names on the device, two passes)
    bool fix_mates = false;  // `fade out -c --fix-mates`: mate fields follow the clip (names, placements, write: three passes on the device)
    bool keep_sorted = false;  // --keep-sorted: with -c, the clipped output of coordinate-sorted input stays coordinate-sorted (a tail held on the device)
    std::vector<std::string> pos;
    std::string out_shards;  // --out-shards PREFIX (with --gpus N)
    std::string stats_tsv, clip_tsv;  // --stats-tsv PATH, --clip-tsv PATH: the stats.d / noclip.d reports of this run
    std::string write_index;  // --write-index PATH: the .bai of the BAM on stdout, made on the device in the same pass
    bool csi = false;  // --csi: the index --write-index (and --extract-sorted) writes is a CSI, min_shift 14 and the depth the longest contig needs, not a BAI
    std::string extract;  // --extract PATH: `fade extract`'s records of this run's artifact calls, in the output's format
    bool sorted = false;  // `fade extract --sorted`: the records leave in coordinate order (a store of records on the device, sorted once at the end)
    bool extract_sorted = false;  // `fade annotate --extract PATH --extract-sorted`: PATH is written in coordinate order, PATH.bai beside it
    std::string calmd;  // `fade out -c --calmd REF.fa`: NM and MD of the clipped records follow the clip, against the genome on the device
    bool sort = false;  // `fade out --sort`: the output leaves in coordinate order whatever the input's (its records in a store on the device, in windows when they do not fit)
    std::string repeats;  // `fade stats --gpus 1 --repeats PATH`: a BED of repeats; every row gains read_rpm and art_rpm (a set of intervals on the device)
    std::string seen;  // N (--calmd); R (--repeats); one letter per option met: t m w b u c h g(pus) B(atch) s(tats) T(iming) S(hards) X (--extract) E (--eject) F (--fragments) K (--keep-sorted) O (--sorted) Y (--extract-sorted)
};

// std.getopt with config.bundling: short flags bundle (-bu), values attach (-w100, -w 100, --window-size=100)
static bool parse_opts(int argc, char **argv, Opts &o, std::string &err) {
    auto need_int = [&](const std::string &name, const char *v, int &dst) {
        char *e = nullptr;
        long x = strtol(v, &e, 10);
        if (!v[0] || *e) { err = "Invalid value for option " + name + ": " + v; return false; }
        dst = (int)x;
        return true;
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "--") { for (int k = i + 1; k < argc; k++) o.pos.push_back(argv[k]); break; }
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
            std::string name = a.substr(2), val;
            bool has_val = false;
            size_t eq = name.find('=');
            if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
            auto take = [&](int &dst) {
                if (!has_val) {
                    if (i + 1 >= argc) { err = "Missing value for argument --" + name; return false; }
                    val = argv[++i];
                }
                return need_int("--" + name, val.c_str(), dst);
            };
            if (name == "threads") { o.seen += 't'; if (!take(o.threads)) return false; }
            else if (name == "min-length") { o.seen += 'm'; if (!take(o.floor_len)) return false; }
            else if (name == "window-size") { o.seen += 'w'; if (!take(o.window)) return false; }
            else if (name == "gpus") { o.seen += 'g'; if (!take(o.gpus)) return false; }
            else if (name == "batch") { o.seen += 'B'; if (!take(o.batch)) return false; }
            else if (name == "out-shards") {
                o.seen += 'S';
                if (!has_val) {
                    if (i + 1 >= argc) { err = "Missing value for argument --" + name; return false; }
                    val = argv[++i];
                }
                if (val.empty()) { err = "Invalid value for option --out-shards: (empty)"; return false; }
                o.out_shards = val;
            }
            else if (name == "stats-tsv" || name == "clip-tsv") {
                o.seen += name == "stats-tsv" ? 'P' : 'Q';
                if (!has_val) {
                    if (i + 1 >= argc) { err = "Missing value for argument --" + name; return false; }
                    val = argv[++i];
                }
                if (val.empty()) { err = "Invalid value for option --" + name + ": (empty)"; return false; }
                (name == "stats-tsv" ? o.stats_tsv : o.clip_tsv) = val;
            }
            else if (name == "extract") {
                o.seen += 'X';
                if (!has_val) {
                    if (i + 1 >= argc) { err = "Missing value for argument --" + name; return false; }
                    val = argv[++i];
                }
                if (val.empty()) { err = "Invalid value for option --extract: (empty)"; return false; }
                o.extract = val;
            }
            else if (name == "repeats") {
                o.seen += 'R';
                if (!has_val) {
                    if (i + 1 >= argc) { err = "Missing value for argument --" + name; return false; }
                    val = argv[++i];
                }
                if (val.empty()) { err = "Invalid value for option --repeats: (empty)"; return false; }
                o.repeats = val;
            }
            else if (name == "calmd") {
                o.seen += 'N';
                if (!has_val) {
                    if (i + 1 >= argc) { err = "Missing value for argument --" + name; return false; }
                    val = argv[++i];
                }
                if (val.empty()) { err = "Invalid value for option --calmd: (empty)"; return false; }
                o.calmd = val;
            }
            else if (name == "write-index") {
                o.seen += 'I';
                if (!has_val) {
                    if (i + 1 >= argc) { err = "Missing value for argument --" + name; return false; }
                    val = argv[++i];
                }
                if (val.empty()) { err = "Invalid value for option --write-index: (empty)"; return false; }
                o.write_index = val;
            }
            else if (name == "bam") { o.seen += 'b'; o.bam = true; }
            else if (name == "ubam") { o.seen += 'u'; o.ubam = true; }
            else if (name == "stats") { o.seen += 's'; o.stats = true; }
            else if (name == "timing") { o.seen += 'T'; o.timing = true; }
            else if (name == "clip") { o.seen += 'c'; o.clip = true; }
            else if (name == "eject") {  // (a flag: std.getopt also takes --eject=true / --eject=false)
                o.seen += 'E';
                if (has_val && val != "true" && val != "false") { err = "Invalid value for option --eject: " + val; return false; }
                o.eject = !has_val || val == "true";
            }
            else if (name == "fragments") {  // (a flag, as --eject)
                o.seen += 'F';
                if (has_val && val != "true" && val != "false") { err = "Invalid value for option --fragments: " + val; return false; }
                o.fragments = !has_val || val == "true";
            }
            else if (name == "fix-mates") {  // (a flag, as --eject)
                o.seen += 'M';
                if (has_val && val != "true" && val != "false") { err = "Invalid value for option --fix-mates: " + val; return false; }
                o.fix_mates = !has_val || val == "true";
            }
            else if (name == "keep-sorted") {  // (a flag, as --eject)
                o.seen += 'K';
                if (has_val && val != "true" && val != "false") { err = "Invalid value for option --keep-sorted: " + val; return false; }
                o.keep_sorted = !has_val || val == "true";
            }
            else if (name == "sorted" || name == "extract-sorted") {  // (flags, as --eject)
                o.seen += name == "sorted" ? 'O' : 'Y';
                if (has_val && val != "true" && val != "false") { err = "Invalid value for option --" + name + ": " + val; return false; }
                (name == "sorted" ? o.sorted : o.extract_sorted) = !has_val || val == "true";
            }
            else if (name == "csi") {  // (a flag, as --eject)
                o.seen += 'J';
                if (has_val && val != "true" && val != "false") { err = "Invalid value for option --csi: " + val; return false; }
                o.csi = !has_val || val == "true";
            }
            else if (name == "sort") {  // (a flag, as --eject)
                o.seen += 'Z';
                if (has_val && val != "true" && val != "false") { err = "Invalid value for option --sort: " + val; return false; }
                o.sort = !has_val || val == "true";
            }
            else if (name == "help") o.help = true;
            else { err = "Unrecognized option --" + name; return false; }
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            for (size_t k = 1; k < a.size(); k++) {
                const char c = a[k];
                if (c != 'h') o.seen += c;
                if (c == 'b') o.bam = true;
                else if (c == 'u') o.ubam = true;
                else if (c == 'h') o.help = true;
                else if (c == 'c') o.clip = true;
                else if (c == 't' || c == 'w') {
                    std::string val = a.substr(k + 1);
                    if (!val.empty() && val[0] == '=') val = val.substr(1);
                    if (val.empty()) {
                        if (i + 1 >= argc) { err = std::string("Missing value for argument -") + c; return false; }
                        val = argv[++i];
                    }
                    if (!need_int(std::string("-") + c, val.c_str(), c == 't' ? o.threads : o.window)) return false;
                    break;
                } else { err = std::string("Unrecognized option -") + c; return false; }
            }
        } else o.pos.push_back(a);
    }
    return true;
}

// --keep-sorted --timing: the largest tail a call left on the device (fadehip_bam_held behind every back call)
static int64_t g_held_max_recs = 0, g_held_max_bytes = 0;
static void note_held(const Opts &o, fadehip_bam_stream *st) {
    int64_t r = 0, b = 0;
    if (!o.keep_sorted || !o.timing || fadehip_bam_held(st, &r, &b)) return;
    if (r > g_held_max_recs) g_held_max_recs = r;
    if (b > g_held_max_bytes) g_held_max_bytes = b;
}
static void report_held(const Opts &o) {
    if (o.keep_sorted && o.timing) fprintf(stderr, "[timing] --keep-sorted: at most %lld records (%lld bytes) held on the device between calls\n", (long long)g_held_max_recs, (long long)g_held_max_bytes);
}

// The index file --write-index and --extract-sorted make: a .bai (fadehip_bai_*), or with --csi a .csi (fadehip_csi_*): min_shift
// 14 and the smallest depth >= 5 whose limit 2^(14 + 3 depth) holds the longest @SQ LN — 5 for every genome a BAI can hold, 6
// beyond, since pos has 32 bits.  A driver sets the depth once its header is read (0: a BAI); the streams and the store that
// make the entries get the same geometry (index_geometry below).
static const int32_t kCsiMinShift = 14;
static int32_t g_csi_depth = 0;
static const char *g_csi_who = "fade";  // whose [I::...] line reports the depth chosen
static int32_t csi_depth_for(const Header &hdr) {
    int64_t longest = 0;
    for (const int64_t len : hdr.lens) longest = std::max(longest, len);
    int32_t depth = 5;
    while (depth < 6 && longest > ((int64_t)1 << (kCsiMinShift + 3 * depth))) depth++;
    return depth;
}
struct IndexFile {
    fadehip_bai *bai = nullptr;
    fadehip_csi *csi = nullptr;
    ~IndexFile() {
        if (bai) fadehip_bai_destroy(bai);
        if (csi) fadehip_csi_destroy(csi);
    }
    bool on() const { return bai || csi; }
    void create(size_t n_ref) {
        if (g_csi_depth) csi = fadehip_csi_create((int32_t)n_ref, kCsiMinShift, g_csi_depth);
        else bai = fadehip_bai_create((int32_t)n_ref);
        if (!on()) throw std::runtime_error("out of memory");
    }
    void add(uint64_t at, const fadehip_index_call *c) {
        if (csi ? fadehip_csi_add(csi, at, c) : fadehip_bai_add(bai, at, c)) throw std::runtime_error(csi ? fadehip_csi_error(csi) : fadehip_bai_error(bai));
    }
    // the .bai's bytes as they are; the .csi's payload in BGZF members of the driver's own writer, then the end-of-file marker
    void write(const std::string &path) {
        const uint8_t *p = nullptr;
        size_t n = 0;
        if (csi ? fadehip_csi_finish(csi, &p, &n) : fadehip_bai_finish(bai, &p, &n)) throw std::runtime_error(csi ? fadehip_csi_error(csi) : fadehip_bai_error(bai));
        std::vector<uint8_t> members;
        if (csi) {
            for (size_t at = 0; at < n; at += 0xff00) bgzf_compress_block(p + at, std::min<size_t>(n - at, 0xff00), 6, members);
            members.insert(members.end(), BGZF_EOF, BGZF_EOF + sizeof BGZF_EOF);
            p = members.data();
            n = members.size();
        }
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot write " + path + ": " + strerror(errno));
        const bool ok = fwrite(p, 1, n, f) == n;
        if (fclose(f) != 0 || !ok) throw std::runtime_error("write error on " + path);
        if (csi)  // (a BAI is written without a word, as it always was)
            fprintf(stderr, "[I::%s] --csi: %s is a CSI index of min_shift %d and depth %d (coordinates up to 2^%d)\n", g_csi_who, path.c_str(), (int)kCsiMinShift, (int)g_csi_depth,
                    (int)(kCsiMinShift + 3 * g_csi_depth));
    }
    static int stream_geometry(fadehip_bam_stream *st) { return g_csi_depth ? fadehip_bam_index_geometry(st, kCsiMinShift, g_csi_depth) : 0; }
};
// --write-index PATH: the .bai of the BAM that goes to stdout.  Every call of the file path leaves its index entries at
// offsets relative to its first member (fadehip_bam_back_index); the driver knows where that member lies in the output — the
// header members it wrote, then the bytes of the calls before — so stdout may be a pipe.  PATH is written behind the
// end-of-file marker.
struct IndexSink {
    IndexFile b;
    uint64_t at = 0;  // file offset of the next call's first member
    std::string path;
    bool on() const { return b.on(); }
    void open(const std::string &p, size_t n_ref) {
        path = p;
        b.create(n_ref);
    }
    // the header's members through `write` into memory first, so that their size is known whatever stdout is
    template <class WriteHeader>
    void header(WriteHeader write) {
        char *mp = nullptr;
        size_t mn = 0;
        FILE *mf = open_memstream(&mp, &mn);
        if (!mf) throw std::runtime_error("out of memory");
        try {
            write(mf);
        } catch (...) {
            fclose(mf);
            free(mp);
            throw;
        }
        fclose(mf);
        const bool ok = fwrite(mp, 1, mn, stdout) == mn;
        free(mp);
        if (!ok) throw std::runtime_error("write error on the output stream");
        at = mn;
    }
    // behind a back call that gave n bytes of members
    void call(fadehip_bam_stream *st, fadehip_ctx *ctx, size_t n) {
        fadehip_index_call c;
        if (fadehip_bam_back_index(st, &c)) throw std::runtime_error(fadehip_last_error(ctx));
        b.add(at, &c);
        at += n;
    }
    void write() { b.write(path); }
};

// `fade extract --sorted`, `fade annotate --extract-sorted`: the run's extract records are in a record store on the device
// (fadehip_recstore_*).  Written here to `out`: the header's members — @HD with SO:coordinate, otherwise the header the
// unsorted file gets —, then the store's drains in coordinate order, members straight from the device compressor, then the
// end-of-file marker; with bai_path the .bai of it, from the header's size and every drain's entries, as IndexSink makes one.
// `out` may be a pipe.  Returns the records written.
// In three steps, so that `fade out --sort` can write a file whose records do not fit the device at once: begin (the header),
// window (one sort of the store and its drains; the windows of the key space come in ascending order, and the one builder of
// the index checks the order between drains), finish (the marker and the .bai).
struct SortedWriter {
    fadehip_ctx *ctx;
    FILE *out;
    bool stored;
    std::string bai_path;
    IndexFile bai;
    bool geometry_set = false;  // --csi: the store has the geometry (set once, in front of its first drain)
    uint64_t at = 0;  // file offset of the next drain's first member
    int64_t total = 0;
    SortedWriter(fadehip_ctx *c, FILE *o, bool st, const std::string &bp) : ctx(c), out(o), stored(st), bai_path(bp) {}
    void begin(Header hdr, Pool *pool) {
        hdr.text = fadehip::recstore::header_sorted(hdr.text);
        char *mp = nullptr;
        size_t mn = 0;
        FILE *mf = open_memstream(&mp, &mn);
        if (!mf) throw std::runtime_error("out of memory");
        try {
            Writer hw(mf, stored ? OutFmt::UBAM : OutFmt::BAM, hdr, pool, nullptr, true, false);
            hw.close();
        } catch (...) {
            fclose(mf);
            free(mp);
            throw;
        }
        fclose(mf);
        const bool ok = fwrite(mp, 1, mn, out) == mn;
        free(mp);
        if (!ok) throw std::runtime_error("write error on the sorted output");
        at = mn;
        if (!bai_path.empty()) bai.create(hdr.names.size());
    }
    void window(fadehip_recstore *rs) {
        if (fadehip_recstore_sort(rs)) throw std::runtime_error(fadehip_last_error(ctx));
        const int32_t flags = (stored ? FADEHIP_RECSTORE_STORED : 0) | (bai.on() ? FADEHIP_RECSTORE_INDEX : 0);
        if (bai.csi && !geometry_set) {
            if (fadehip_recstore_index_geometry(rs, kCsiMinShift, g_csi_depth)) throw std::runtime_error(fadehip_last_error(ctx));
            geometry_set = true;
        }
        for (;;) {
            const uint8_t *p = nullptr;
            size_t n = 0;
            int64_t n_rec = 0;
            fadehip_index_call c;
            if (fadehip_recstore_drain(rs, flags, (uint64_t)64 << 20, &p, &n, &n_rec, bai.on() ? &c : nullptr)) throw std::runtime_error(fadehip_last_error(ctx));
            if (!n_rec) break;
            if (fwrite(p, 1, n, out) != n) throw std::runtime_error("write error on the sorted output");
            if (bai.on()) bai.add(at, &c);
            at += n;
            total += n_rec;
        }
    }
    void finish() {
        if (fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, out) != sizeof BGZF_EOF || fflush(out) != 0 || ferror(out)) throw std::runtime_error("write error on the sorted output");
        if (bai.on()) bai.write(bai_path);
    }
};
static int64_t write_sorted_store(fadehip_ctx *ctx, fadehip_recstore *rs, FILE *out, bool stored, Header hdr, Pool *pool, const std::string &bai_path) {
    SortedWriter w(ctx, out, stored, bai_path);
    w.begin(hdr, pool);
    w.window(rs);
    w.finish();
    return w.total;
}

// What `fade out -c` and `fade annotate -c` say about their output (filter.d:184-185); with --keep-sorted, what holds instead
static const char *const kFixMatesLine =
    "[W::fade-out] --fix-mates: mate fields (next position, template length, mate strand and unmapped flags, MC) follow the clip: three passes over the file "
    "(names of the artifact reads, placements of their fragments, write)\n";
static void clip_warnings(const Opts &o) {
    if (o.sort)
        fprintf(stderr, "[W::fade-out] --sort: the output is written in coordinate order, clipped records at their new coordinates; reads clipped to nothing go to the end as unmapped records\n");
    else if (o.keep_sorted)
        fprintf(stderr, "[W::fade-out] --keep-sorted: clipped records are written at their new coordinates, so coordinate-sorted input stays sorted; reads clipped to nothing go to the end as unmapped records\n");
    else
        fprintf(stderr, "[W::fade-out] Using the -c flag means the output SAM/BAM will not be sorted (regardless of prior sorting)\n");
    if (o.fix_mates) fputs(kFixMatesLine, stderr);
    else fprintf(stderr, "[W::fade-out] You also may need to fix mate information with a tool like Picard FixMateInformation\n");
}


// ------------------------------------------------------------------ one batch in flight
// Pinned batch blocks (fadehip_batch_bytes / fadehip_batch_bind) are recycled: upload is one hipMemcpyAsync from them.
struct BlockPool {
    struct Block { void *p; size_t cap; };
    fadehip_ctx *ctx = nullptr;
    std::mutex m;
    std::vector<Block> free_;
    void *acquire(size_t bytes, size_t *cap) {
        {
            std::lock_guard<std::mutex> l(m);
            for (size_t k = 0; k < free_.size(); k++)
                if (free_[k].cap >= bytes) {
                    Block b = free_[k];
                    free_.erase(free_.begin() + (long)k);
                    *cap = b.cap;
                    return b.p;
                }
        }
        void *p = nullptr;
        const size_t want = bytes + bytes / 4 + 4096;
        if (fadehip_host_alloc(ctx, want, &p)) throw std::runtime_error(std::string("pinned allocation: ") + fadehip_last_error(ctx));
        *cap = want;
        return p;
    }
    void release(void *p, size_t cap) {
        if (!p) return;
        std::lock_guard<std::mutex> l(m);
        free_.push_back({p, cap});
    }
    void drain() {
        for (auto &b : free_) fadehip_host_free(ctx, b.p);
        free_.clear();
    }
};

// the writer's BGZF blocks compressed on the device (fadehip_bgzf_deflate_*): two lanes, each with a pinned staging buffer
struct DeviceBgzf : BgzfDevice {
    fadehip_ctx *ctx;
    struct Lane { void *p = nullptr; size_t cap = 0; } lane_[FADEHIP_BGZF_LANES];
    explicit DeviceBgzf(fadehip_ctx *c) : ctx(c) {}
    ~DeviceBgzf() override {
        for (auto &l : lane_)
            if (l.p) fadehip_host_free(ctx, l.p);
    }
    int lanes() const override { return FADEHIP_BGZF_LANES; }
    uint8_t *stage(int lane, size_t bytes) override {
        Lane &l = lane_[lane];
        if (bytes > l.cap) {
            if (l.p) fadehip_host_free(ctx, l.p);
            l.p = nullptr;
            l.cap = bytes + bytes / 4 + (1u << 20);
            if (fadehip_host_alloc(ctx, l.cap, &l.p)) throw std::runtime_error(std::string("pinned allocation: ") + fadehip_last_error(ctx));
        }
        return (uint8_t *)l.p;
    }
    void submit(int lane, size_t bytes) override {
        if (fadehip_bgzf_deflate_submit(ctx, lane, lane_[lane].p, bytes)) throw std::runtime_error(std::string("device BGZF: ") + fadehip_last_error(ctx));
    }
    void wait(int lane, const uint8_t **out, size_t *n) override {
        if (fadehip_bgzf_deflate_wait(ctx, lane, out, n)) throw std::runtime_error(std::string("device BGZF: ") + fadehip_last_error(ctx));
    }
};

struct Chunk {
    RecordBlock blk;             // the records, framed in place (BAM: in the inflated bytes; SAM: parsed into the same layout)
    Writer::BlockOut bout;       // ... and what annotate adds to them
    size_t n_records() const { return blk.size(); }
    // anno.d:61-65: an unmapped record, or one without an S op, gets rs = 0 and nothing else: such records are not sent.
    std::vector<uint32_t> sent;  // indices (into recs) of the records that are
    fadehip_read_batch b;        // bound into `block`
    void *block = nullptr;
    size_t block_cap = 0;
    // what the writer stage needs of the results, copied out of the slot's pinned result block
    std::vector<uint8_t> rs_sent;
    std::vector<fadehip_aln> art;  // the artifact calls (art != 0); read_idx indexes `sent`
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int n_oversize = 0;
    int dev = 0, slot = 0;
};

template <class R>
static inline bool needs_device(const R &r) {
    if (r.flag() & 4) return false;
    for (int k = 0; k < r.n_cigar(); k++)
        if ((r.cigar_op(k) & 15u) == 4u) return true;
    return false;
}

// records -> the batch block, in parallel: count per range, prefix, fill
template <class Get>
static void pack_chunk_t(Chunk &c, Pool &pool, BlockPool &blocks, const Get &get) {
    const size_t n = c.n_records();
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)pool.size(), n / 4096 + 1));
    struct Range { size_t n_sent = 0, n_cig = 0, n_seq = 0; int64_t span = 0; };
    std::vector<Range> rg(nt + 1);
    std::vector<uint8_t> need(n);
    pool.parallel_for(nt, [&](size_t t) {
        Range r;
        for (size_t i = n * t / nt; i < n * (t + 1) / nt; i++) {
            const auto &rec = get(i);
            need[i] = needs_device(rec) ? 1 : 0;
            if (!need[i]) continue;
            r.n_sent++;
            r.n_cig += (size_t)rec.n_cigar();
            r.n_seq += ((size_t)rec.l_seq() + 1) / 2;
            r.span = std::max(r.span, cigar_ref_len(rec));
        }
        rg[t + 1] = r;
    }, CPU_PACK);
    int64_t span = 1;
    for (size_t t = 1; t <= nt; t++) {
        span = std::max(span, rg[t].span);
        rg[t].n_sent += rg[t - 1].n_sent;
        rg[t].n_cig += rg[t - 1].n_cig;
        rg[t].n_seq += rg[t - 1].n_seq;
    }
    const size_t ns = rg[nt].n_sent, ncig = rg[nt].n_cig, nseq = rg[nt].n_seq;
    if (nseq >= ((size_t)1 << 31)) throw std::runtime_error("batch too large: lower --batch");
    c.block = blocks.acquire(fadehip_batch_bytes((int32_t)ns, (int64_t)ncig, (int64_t)nseq), &c.block_cap);
    if (fadehip_batch_bind(c.block, (int32_t)ns, (int64_t)ncig, (int64_t)nseq, &c.b)) throw std::runtime_error(fadehip_last_error(nullptr));
    c.sent.resize(ns);
    int32_t *tid = const_cast<int32_t *>(c.b.tid), *pos = const_cast<int32_t *>(c.b.pos), *lseq = const_cast<int32_t *>(c.b.l_seq);
    uint16_t *flag = const_cast<uint16_t *>(c.b.flag);
    uint8_t *has_sa = const_cast<uint8_t *>(c.b.has_sa), *seq = const_cast<uint8_t *>(c.b.seq_packed);
    uint32_t *coff = const_cast<uint32_t *>(c.b.cigar_off), *soff = const_cast<uint32_t *>(c.b.seq_off), *cops = const_cast<uint32_t *>(c.b.cigar_ops);
    pool.parallel_for(nt, [&](size_t t) {
        size_t k = rg[t].n_sent, nc = rg[t].n_cig, nq = rg[t].n_seq;
        for (size_t i = n * t / nt; i < n * (t + 1) / nt; i++) {
            if (!need[i]) continue;
            const auto &r = get(i);
            c.sent[k] = (uint32_t)i;
            tid[k] = r.tid();
            pos[k] = r.pos();
            lseq[k] = r.l_seq();
            flag[k] = (uint16_t)r.flag();
            has_sa[k] = r.aux_exists("SA") ? 1 : 0;  // anno.d:73
            coff[k] = (uint32_t)nc;
            soff[k] = (uint32_t)nq;
            const size_t cb = 4 * (size_t)r.n_cigar(), sb = ((size_t)r.l_seq() + 1) / 2;
            if (cb) memcpy(cops + nc, r.cigar_bytes(), cb);
            if (sb) memcpy(seq + nq, r.seq(), sb);
            nc += (size_t)r.n_cigar();
            nq += sb;
            k++;
        }
    }, CPU_PACK);
    coff[ns] = (uint32_t)ncig;
    soff[ns] = (uint32_t)nseq;
    c.b.n_skipped = (int32_t)(n - ns);
    c.b.ref_span_bound = (int32_t)std::min<int64_t>(span, INT32_MAX);
}
static void pack_chunk(Chunk &c, Pool &pool, BlockPool &blocks) {
    pack_chunk_t(c, pool, blocks, [&](size_t i) { return c.blk.view(i); });
}

static std::string cigar_string(const uint32_t *ops, int n) {
    std::string s;
    for (int k = 0; k < n; k++) {
        append_int(s, ops[k] >> 4);
        s += CIGAR_STR[std::min<uint32_t>(ops[k] & 15, 9)];
    }
    return s;
}

// The four strings of an artifact call: analysis.d:84-92 / 108-118 + anno.d:98-107 (am, as, ar, ab; "left;right").
template <class R>
static void artifact_strings(const R &r, const fadehip_aln &a, const Header &h, std::string out[4]) {
    static const uint8_t comp[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};  // util.d:18-20
    const int lq = r.l_seq();
    std::string seq((size_t)lq, 'N'), qrc((size_t)lq, 'N'), bq((size_t)lq, '!');
    const uint8_t *sq = r.seq(), *ql = r.qual();
    for (int j = 0; j < lq; j++) {
        const int code = (sq[j >> 1] >> ((~j & 1) << 2)) & 15;
        seq[(size_t)j] = NT16_STR[code];
        qrc[(size_t)(lq - 1 - j)] = NT16_STR[comp[code]];  // util.d:23-34
        bq[(size_t)j] = (char)(ql[j] + 33);
    }
    const int nops = std::min(a.sw.n_ops, FADEHIP_MAX_OPS);
    const std::string cig = cigar_string(a.sw.ops, nops);
    const int64_t apos = a.win_start + a.sw.beg_ref;
    const int64_t pos = r.pos();
    std::string am = (r.tid() >= 0 && r.tid() < (int)h.names.size() ? h.names[(size_t)r.tid()] : std::string("*"));
    am += ',';
    append_int(am, apos);
    am += ',';
    am += cig;
    std::string l[4], rr[4];
    if (a.art & 1) {  // analysis.d:84-92
        const int64_t clip = a.clip_left;
        const int64_t overlap = apos >= pos - clip ? apos - (pos - clip) : 0;
        const int64_t lead = (a.sw.ops[0] & 15) == 4 ? (a.sw.ops[0] >> 4) : 0;
        const int64_t plen = std::min<int64_t>(lq, (lq - lead) + overlap);
        l[0] = am; l[1] = seq.substr(0, (size_t)plen); l[2] = qrc.substr((size_t)(lq - plen)); l[3] = bq.substr(0, (size_t)plen);
    }
    if (a.art & 2) {  // analysis.d:108-118
        const int64_t clip = a.clip_right;
        int64_t res_al = 0;
        for (int q = 0; q < nops; q++) {
            const uint32_t op = a.sw.ops[q] & 15;
            if (FADEHIP_OP_CONSUMES_REF(op)) res_al += a.sw.ops[q] >> 4;
        }
        const int64_t lhs = pos + a.aligned_len + clip, rhs = apos + res_al;
        const int64_t overlap = lhs >= rhs ? lhs - rhs : 0;
        const int64_t trail = (a.sw.ops[nops - 1] & 15) == 4 ? (a.sw.ops[nops - 1] >> 4) : 0;
        const int64_t plen = std::min<int64_t>(lq, (lq - trail) + overlap);
        rr[0] = am; rr[1] = seq.substr((size_t)(lq - plen)); rr[2] = qrc.substr(0, (size_t)plen); rr[3] = bq.substr((size_t)(lq - plen));
    }
    for (int k = 0; k < 4; k++) out[k] = l[k] + ";" + rr[k];  // anno.d:100-106
}

static void clip_read(Rec &rec, uint32_t rsv, const int64_t *ref_len = nullptr);

// remap.d:46-61 / 67-82: the record `fade extract` makes of one artifact side — a new mapped record on contig tid at the
// 0-based pos with the alignment's CIGAR, carrying the read's name, its bases reverse-complemented and its qualities
// reversed; everything else is what a zero-filled bam1_t holds (mapq 0, mate tid 0, mate pos 0, tlen 0), and no aux area
template <class R>
static Rec build_extract_rec(const R &r, int tid, int64_t pos, const uint32_t *cig, size_t n_cig) {
    static const uint8_t comp[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};
    const int lq = r.l_seq();
    const size_t lqn = (size_t)r.l_qname();
    Rec n;
    n.d.assign(32 + lqn + 4 * n_cig + ((size_t)lq + 1) / 2 + (size_t)lq, 0);
    int64_t reflen = 0;
    for (size_t k = 0; k < n_cig; k++) {
        const uint32_t op = cig[k] & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += cig[k] >> 4;
    }
    n.template wr<int32_t>(0, tid);                       // remap.d:49
    n.template wr<int32_t>(4, (int32_t)pos);              // remap.d:50 (ZB: am holds a 0-based position)
    n.d[8] = (uint8_t)lqn;
    n.d[9] = 0;                                  // a fresh bam1_t: mapq 0
    n.template wr<uint16_t>(10, (uint16_t)reg2bin(pos < 0 ? 0 : pos, (pos < 0 ? 0 : pos) + (reflen > 0 ? reflen : 1)));
    n.template wr<uint16_t>(12, (uint16_t)n_cig);
    n.template wr<uint16_t>(14, (uint16_t)((r.flag() & 0x10) ? 0 : 0x10));  // remap.d:51-58
    n.template wr<int32_t>(16, lq);
    n.template wr<int32_t>(20, 0);                        // bam_init1 zero-fills: mtid 0, mpos 0, isize 0
    n.template wr<int32_t>(24, 0);
    n.template wr<int32_t>(28, 0);
    memcpy(n.d.data() + 32, r.qname(), lqn);     // remap.d:48
    size_t off = 32 + lqn;
    if (n_cig) memcpy(n.d.data() + off, cig, 4 * n_cig);  // remap.d:61
    off += 4 * n_cig;
    const uint8_t *sq = r.seq(), *ql = r.qual();
    for (int j = 0; j < lq; j++) {               // remap.d:59 reverse_complement_sam_record
        const int code = (sq[j >> 1] >> ((~j & 1) << 2)) & 15;
        const int k = lq - 1 - j;
        n.d[off + (size_t)(k >> 1)] |= (uint8_t)(comp[code] << ((~k & 1) << 2));
    }
    off += ((size_t)lq + 1) / 2;
    for (int j = 0; j < lq; j++) n.d[off + (size_t)j] = ql[lq - 1 - j];  // remap.d:60
    return n;
}

static void tag_owned_record(Rec &r, uint8_t rs, const fadehip_aln *a, const Header &h) {
    r.aux_update_uint("rs", rs);  // anno.d:63,94
    if (!a) return;
    std::string t[4];
    artifact_strings(r, *a, h, t);
    r.aux_update_str("am", t[0]);  // anno.d:100
    r.aux_update_str("as", t[1]);  // anno.d:102
    r.aux_update_str("ar", t[2]);  // anno.d:104
    r.aux_update_str("ab", t[3]);  // anno.d:106
}

// anno.d:94-107 over a chunk: rs for every record (0 for the ones anno.d:61-65 settles without the device), the artifact
// strings for the few that have them, keeping the reference's tag order rs, am, as, ar, ab
// clip (`fade annotate -c`): an artifact call is rebuilt as a whole too, tagged, and then hard-clipped by clip_read — with the
// lengths of the batch's alignment, not of the am text (a record that came in with am:i keeps that tag and is clipped all the same)
// extract (`fade annotate --extract`): `fade extract`'s records of the chunk's artifact calls, in record order, left before
// right — from the record as it came in and the batch's alignment, likewise never from tags read back
static void apply_tags(Chunk &c, const Header &h, Pool &pool, bool clip = false, std::vector<Rec> *extract = nullptr) {
    const size_t n = c.n_records();
    std::vector<uint8_t> rs(n, 0);
    for (size_t k = 0; k < c.sent.size(); k++) rs[c.sent[k]] = c.rs_sent[k];
    std::vector<int> art_of(n, -1);
    for (size_t k = 0; k < c.art.size(); k++) {
        const int32_t si = c.art[k].read_idx;  // an index into the records that were sent
        if (si < 0 || (size_t)si >= c.sent.size()) throw std::runtime_error("device returned an alignment for a record that was not sent");
        art_of[c.sent[(size_t)si]] = (int)k;
    }
    const size_t nt = (size_t)pool.size();
    // Records framed in place: the new tags become a suffix behind the record's bytes (htslib appends an absent tag).
    // A record that already carries one of the five tags (annotating an annotated file) is rebuilt as a whole instead,
    // with htslib's update-in-place semantics.
    Writer::BlockOut &o = c.bout;
    o.sfx_off.assign(n + 1, 0);
    o.owned.clear();
    std::vector<std::string> art_str(c.art.size() * 4);
    std::vector<std::vector<std::pair<uint32_t, Rec>>> owned_t(nt);
    std::vector<std::vector<Rec>> extract_t(extract ? nt : 0);
    pool.parallel_for(nt, [&](size_t t) {
        for (size_t i = n * t / nt; i < n * (t + 1) / nt; i++) {
            const RecView v = c.blk.view(i);
            if (extract && art_of[i] >= 0 && (rs[i] & 6)) {
                const fadehip_aln &al = c.art[(size_t)art_of[i]];
                const size_t n_ops = (size_t)std::min<int>(std::max(al.sw.n_ops, 0), FADEHIP_MAX_OPS);
                for (int side = 0; side < 2; side++)  // (am names the one alignment on both sides)
                    if (rs[i] & (2u << side)) extract_t[t].push_back(build_extract_rec(v, v.tid(), al.win_start + al.sw.beg_ref, al.sw.ops, n_ops));
            }
            bool has_ours = false;
            for (size_t p = v.aux_off(); p + 3 <= v.nbytes();) {
                const size_t fs = v.aux_field_size(p + 2);
                if (!fs) break;
                const uint8_t a0 = v.bytes()[p], a1 = v.bytes()[p + 1];
                has_ours |= (a0 == 'r' && a1 == 's') || (a0 == 'a' && (a1 == 'm' || a1 == 's' || a1 == 'r' || a1 == 'b'));
                p += 2 + fs;
            }
            const fadehip_aln *a = art_of[i] >= 0 ? &c.art[(size_t)art_of[i]] : nullptr;
            const bool clip_it = clip && a && (rs[i] & 6);
            if (has_ours || clip_it) {
                Rec r;
                r.d.assign(v.bytes(), v.bytes() + v.nbytes());
                tag_owned_record(r, rs[i], a, h);
                if (clip_it) {
                    int64_t n_ref = 0;
                    for (int q = 0; q < std::min<int>(a->sw.n_ops, FADEHIP_MAX_OPS); q++)
                        if (FADEHIP_OP_CONSUMES_REF(a->sw.ops[q] & 15u)) n_ref += a->sw.ops[q] >> 4;
                    const int64_t lens[2] = {n_ref, n_ref};  // (am names the one alignment on both sides)
                    clip_read(r, rs[i], lens);
                }
                owned_t[t].emplace_back((uint32_t)i, std::move(r));
                continue;
            }
            size_t len = 4;  // "rs" 'C' value
            if (a) {
                std::string *st = &art_str[(size_t)art_of[i] * 4];
                artifact_strings(v, *a, h, st);
                for (int k = 0; k < 4; k++) len += 3 + st[k].size() + 1;
            }
            o.sfx_off[i + 1] = (uint32_t)len;
        }
    }, CPU_TAGS);
    for (auto &v : owned_t)
        for (auto &e : v) o.owned.push_back(std::move(e));
    if (extract) {
        extract->clear();
        for (auto &v : extract_t)  // (the threads' ranges follow one another)
            for (auto &e : v) extract->push_back(std::move(e));
    }
    for (size_t i = 0; i < n; i++) o.sfx_off[i + 1] += o.sfx_off[i];
    o.sfx.resize(o.sfx_off[n]);
    pool.parallel_for(nt, [&](size_t t) {
        static const char names[4][2] = {{'a', 'm'}, {'a', 's'}, {'a', 'r'}, {'a', 'b'}};
        for (size_t i = n * t / nt; i < n * (t + 1) / nt; i++) {
            if (o.sfx_off[i + 1] == o.sfx_off[i]) continue;
            uint8_t *d = o.sfx.data() + o.sfx_off[i];
            d[0] = 'r'; d[1] = 's'; d[2] = 'C'; d[3] = rs[i];  // bam_aux_update_int of a ubyte: the smallest type
            d += 4;
            if (art_of[i] >= 0) {
                const std::string *st = &art_str[(size_t)art_of[i] * 4];
                for (int k = 0; k < 4; k++) {
                    d[0] = (uint8_t)names[k][0]; d[1] = (uint8_t)names[k][1]; d[2] = 'Z';
                    memcpy(d + 3, st[k].c_str(), st[k].size() + 1);
                    d += 3 + st[k].size() + 1;
                }
            }
        }
    }, CPU_TAGS);
}

// `fade stats` (stats.d:75-186) and `fade stats-clip` (noclip.d:17-73) over this run's output, written while the tags are
// applied (`fade annotate --stats-tsv / --clip-tsv`): every value a row needs is here already — the record, its rs and the
// four artifact strings.  The inverted-repeat search of a chunk's artifact sides is one fadehip_sw_stats_batch call.
struct Reports {
    FILE *st = nullptr, *cl = nullptr;
    std::string st_path, cl_path;
    bool on() const { return st || cl; }
    void open(const Opts &o) {
        auto op = [](const std::string &p) {
            FILE *f = fopen(p.c_str(), "wb");
            if (!f) throw std::runtime_error("cannot open " + p + " for writing: " + strerror(errno));
            return f;
        };
        if (!o.stats_tsv.empty()) {
            st_path = o.stats_tsv;
            st = op(st_path);
            fputs("qname\trname\tpos\tcigar\tart_start\tart_end\taln_rname\taln_start\taln_end\tart_cigar\tstemloop\tstemloop_rc\t"
                  "predicted_inverted_repeat\tIR_identity\tavgbq\tart_avgbq\tart_bq\tIR_bq\tflagbinary\tflag\tstrand\n", st);
        }
        if (!o.clip_tsv.empty()) {
            cl_path = o.clip_tsv;
            cl = op(cl_path);
            fputs("qname\tsc_q_scores\tsc_seq\tsc_avg_bq\tavg_bq\tart_status\n", cl);
        }
    }
    void close() {  // throws if a write failed
        std::string bad;
        if (st && (fflush(st) || ferror(st))) bad = st_path;
        if (cl && (fflush(cl) || ferror(cl))) bad = cl_path;
        if (st) fclose(st);
        if (cl) fclose(cl);
        st = cl = nullptr;
        if (!bad.empty()) throw std::runtime_error("writing " + bad + " failed");
    }
    ~Reports() {
        if (st) fclose(st);
        if (cl) fclose(cl);
    }
    void add(const Chunk &c, const Header &h, fadehip_ctx *ctx);
};

// D's to!string of a float quotient, as OutStats::ratio prints it: %g, nan, inf
static void append_ratio(std::string &s, uint64_t num, uint64_t den) {
    const float v = (float)num / (float)den;
    char b[64];
    if (std::isnan(v)) snprintf(b, sizeof b, "nan");
    else if (std::isinf(v)) snprintf(b, sizeof b, "inf");
    else snprintf(b, sizeof b, "%g", (double)v);
    s += b;
}

static int64_t cigar_string_aligned_length(const std::string &cig, bool &ok) {  // dhtslib cigarFromString(..).alignedLength
    int64_t n = 0, len = 0;
    bool digits = false;
    ok = !cig.empty();
    for (char ch : cig) {
        if (ch >= '0' && ch <= '9') { len = len * 10 + (ch - '0'); digits = true; continue; }
        const char *o = strchr(CIGAR_STR, ch);
        if (!o || !*o || !digits) { ok = false; return 0; }
        if (FADEHIP_OP_CONSUMES_REF((uint32_t)(o - CIGAR_STR))) n += len;
        len = 0;
        digits = false;
    }
    if (digits) ok = false;
    return n;
}

static std::vector<std::string> split_on(const std::string &s, char sep) {
    std::vector<std::string> v;
    size_t b = 0;
    for (;;) {
        const size_t e = s.find(sep, b);
        v.push_back(s.substr(b, e == std::string::npos ? std::string::npos : e - b));
        if (e == std::string::npos) return v;
        b = e + 1;
    }
}

void Reports::add(const Chunk &c, const Header &h, fadehip_ctx *ctx) {
    const size_t n = c.n_records();
    std::vector<uint8_t> rs(n, 0);
    for (size_t k = 0; k < c.sent.size(); k++) rs[c.sent[k]] = c.rs_sent[k];
    std::vector<int> art_of(n, -1);
    for (size_t k = 0; k < c.art.size(); k++) art_of[c.sent[(size_t)c.art[k].read_idx]] = (int)k;
    auto fail = [](const RecView &v, const char *what) {
        throw std::runtime_error(std::string("record ") + v.qname() + ": " + what);
    };
    std::string clip_out;
    struct Side {
        size_t rec;
        std::string head, stemloop, ab_slice;  // columns qname .. stemloop_rc, the stem loop, art_bq
        std::string tail;                      // flagbinary, flag, strand
        uint64_t qsum;
        int l_seq;
    };
    std::vector<Side> sides;
    std::string q, r;
    std::vector<int64_t> q_off(1, 0), r_off(1, 0);
    for (size_t i = 0; i < n; i++) {
        const uint8_t rsv = rs[i];
        if (!(rsv & 1)) continue;  // neither report looks at a record without a soft clip (rs bit 0)
        const RecView v = c.blk.view(i);
        const int ls = v.l_seq();
        const uint8_t *ql = v.qual();
        uint64_t qsum = 0;
        for (int j = 0; j < ls; j++) qsum += ql[j];
        auto base = [&](int j) { return NT16_STR[(v.seq()[j >> 1] >> ((~j & 1) << 2)) & 15]; };
        if (cl) {  // noclip.d:22-71 with parse_clips' quirk (util.d:37-62)
            uint32_t clips[2] = {0, 0};
            bool first = true;
            for (int k = 0; k < v.n_cigar(); k++) {
                const uint32_t op = v.cigar_op(k);
                if ((op & 15) == 5) continue;
                const bool sc = (op & 15) == 4;
                if (first && !sc) first = false;
                else if (first && sc) clips[0] = op;
                else if (sc) clips[1] = op;
            }
            for (int side = 0; side < 2; side++) {
                if (!clips[side]) continue;
                const int len = (int)(clips[side] >> 4);
                if (ls == 0) fail(v, "a soft-clipped record without bases (SEQ *): stats-clip has no clip to report");
                if (len > ls) fail(v, "soft clip longer than the read");
                const int b0 = side == 0 ? 0 : ls - len;
                uint64_t ssum = 0;
                clip_out.append(v.qname());
                clip_out += '\t';
                for (int j = b0; j < b0 + len; j++) {
                    ssum += ql[j];
                    clip_out += (char)(uint8_t)(ql[j] + 33);  // ubyte arithmetic: 0xff wraps to ' '
                }
                clip_out += '\t';
                for (int j = b0; j < b0 + len; j++) clip_out += base(j);
                clip_out += '\t';
                append_ratio(clip_out, ssum, (uint64_t)len);
                clip_out += '\t';
                append_ratio(clip_out, qsum, (uint64_t)ls);
                clip_out += '\t';
                clip_out += (rsv & (side == 0 ? 2 : 4)) ? "true" : "false";
                clip_out += '\n';
            }
        }
        if (!st || !(rsv & 6)) continue;
        if (art_of[i] < 0) fail(v, "artifact record without its alignment");
        std::string t[4];
        artifact_strings(v, c.art[(size_t)art_of[i]], h, t);
        if (v.tid() < 0 || v.tid() >= (int)h.names.size()) fail(v, "artifact record without a reference");
        std::string cig;
        int64_t al = 0;
        int first_s = -1, last_s = -1;
        for (int k = 0; k < v.n_cigar(); k++) {
            const uint32_t op = v.cigar_op(k);
            append_int(cig, op >> 4);
            cig += CIGAR_STR[std::min<uint32_t>(op & 15, 9)];
            if (FADEHIP_OP_CONSUMES_REF(op & 15)) al += op >> 4;
            if ((op & 15) == 4) {
                if (first_s < 0) first_s = (int)(op >> 4);
                last_s = (int)(op >> 4);
            }
        }
        if (first_s < 0) fail(v, "artifact record without a soft clip");
        const std::vector<std::string> am = split_on(t[0], ';'), as = split_on(t[1], ';'), ar = split_on(t[2], ';');
        if (am.size() < 2 || as.size() < 2 || ar.size() < 2) fail(v, "malformed am / as / ar tag");
        const int64_t pos = v.pos();
        for (int side = 0; side < 2; side++) {
            if (!(rsv & (side == 0 ? 2 : 4))) continue;
            const std::vector<std::string> f = split_on(am[(size_t)side], ',');
            if (f.size() < 3) fail(v, "malformed am tag");
            char *e = nullptr;
            const long aln_start = strtol(f[1].c_str(), &e, 10);
            bool ok = !f[1].empty() && !*e;
            const int64_t aln_len = cigar_string_aligned_length(f[2], ok);
            const std::string &sl = as[(size_t)side], &slrc = ar[(size_t)side];
            if (!ok || sl.empty() || t[3].size() < sl.size()) fail(v, "malformed am / as / ab tag");
            Side s;
            s.rec = i;
            s.head = v.qname();
            s.head += '\t'; s.head += h.names[(size_t)v.tid()];
            s.head += '\t'; append_int(s.head, pos);
            s.head += '\t'; s.head += cig;
            s.head += '\t'; append_int(s.head, side == 0 ? pos - first_s : pos + al);
            s.head += '\t'; append_int(s.head, side == 0 ? pos : pos + al + last_s);
            s.head += '\t'; s.head += f[0];
            s.head += '\t'; s.head += f[1];
            s.head += '\t'; append_int(s.head, (int64_t)aln_start + aln_len);
            s.head += '\t'; s.head += f[2];
            s.head += '\t'; s.head += sl;
            s.head += '\t'; s.head += slrc;
            s.stemloop = sl;
            s.ab_slice = side == 0 ? t[3].substr(0, sl.size()) : t[3].substr(t[3].size() - sl.size());
            char fb[16];
            for (int b = 0; b < 8; b++) fb[b] = (rsv >> (7 - b)) & 1 ? '1' : '0';
            fb[8] = 0;
            s.tail = fb;
            s.tail += '\t'; append_int(s.tail, rsv);
            s.tail += '\t'; s.tail += (v.flag() & 16) ? "+" : "-";
            s.qsum = qsum;
            s.l_seq = ls;
            const size_t end = (3 * sl.size() + 2) / 4;  // round(0.75 * length): half away from zero
            q.append(sl, 0, end);
            r += slrc;
            q_off.push_back((int64_t)q.size());
            r_off.push_back((int64_t)r.size());
            sides.push_back(std::move(s));
        }
    }
    if (!sides.empty()) {
        std::vector<fadehip_sw_stats_result> res(sides.size());
        static const int32_t scoring[4] = {3, 8, 10, -5};  // stats.d:87
        if (fadehip_sw_stats_batch(ctx, scoring, (int32_t)sides.size(), (const uint8_t *)q.data(), q_off.data(),
                                   (const uint8_t *)r.data(), r_off.data(), res.data()))
            throw std::runtime_error(std::string("stats alignment: ") + fadehip_last_error(ctx));
        std::string out;
        for (size_t k = 0; k < sides.size(); k++) {
            const Side &s = sides[k];
            const size_t ir = (size_t)res[k].end_query + 1;
            if (ir > s.stemloop.size()) throw std::runtime_error("stats alignment ended beyond the stem loop");
            uint64_t bsum = 0;
            for (unsigned char ch : s.ab_slice) bsum += ch;
            out += s.head;
            out += '\t'; out.append(s.stemloop, 0, ir);
            out += '\t'; append_ratio(out, (uint64_t)res[k].matches, (uint64_t)res[k].length);
            out += '\t'; append_ratio(out, s.qsum, (uint64_t)s.l_seq);
            out += '\t'; append_ratio(out, bsum, s.stemloop.size());
            out += '\t'; out += s.ab_slice;
            out += '\t'; out.append(s.ab_slice, 0, ir);
            out += '\t'; out += s.tail;
            out += '\n';
        }
        if (!out.empty()) fwrite(out.data(), 1, out.size(), st);
    }
    if (!clip_out.empty()) fwrite(clip_out.data(), 1, clip_out.size(), cl);
}


// FADE_TRACE=1: every start / stop pair of a named stage clock as a line on stderr at the end (ms since the first one)
struct StageTrace {
    bool on = getenv("FADE_TRACE") != nullptr;
    std::mutex m;
    std::chrono::steady_clock::time_point origin = std::chrono::steady_clock::now();
    struct Ev { const char *name; double t0, t1; };
    std::vector<Ev> ev;
    void add(const char *name, std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        std::lock_guard<std::mutex> l(m);
        ev.push_back(Ev{name, std::chrono::duration<double>(a - origin).count(), std::chrono::duration<double>(b - origin).count()});
    }
    void dump() {
        if (!on) return;
        std::lock_guard<std::mutex> l(m);
        std::sort(ev.begin(), ev.end(), [](const Ev &a, const Ev &b) { return a.t0 < b.t0; });
        for (auto &e : ev) fprintf(stderr, "[trace] %-8s %9.3f ms  +%8.3f ms\n", e.name, e.t0 * 1e3, (e.t1 - e.t0) * 1e3);
    }
};
static StageTrace g_trace;

struct StageClock {
    double t = 0;
    const char *name = nullptr;
    std::chrono::steady_clock::time_point t0;
    void start() { t0 = std::chrono::steady_clock::now(); }
    void stop() {
        const auto t1 = std::chrono::steady_clock::now();
        t += std::chrono::duration<double>(t1 - t0).count();
        if (g_trace.on && name) g_trace.add(name, t0, t1);
    }
};

// joins the stage threads on every way out of annotate_main (an exception past a joinable std::thread is std::terminate)
struct StageThreads {
    std::vector<std::thread> th;
    std::function<void()> unblock;  // closes the queues so that the stages can finish
    ~StageThreads() {
        if (unblock) unblock();
        for (auto &t : th)
            if (t.joinable()) t.join();
    }
};

// The staging buffers of the file-path drivers: ordinary memory while the ctx is still being made (the reader fills them
// meanwhile), registered with it once it is there.  A driver's Guard gives them back (unpin) before it destroys the ctx;
// the memory itself goes when this does, so it is declared in front of the Guard.
struct Staging {
    std::vector<std::pair<void *, size_t>> raw;  // allocated here
    std::vector<void *> pinned;                  // ... and registered with the ctx
    uint8_t *alloc(size_t bytes) {
        const size_t al = (size_t)1 << 21, n = (bytes + al - 1) & ~(al - 1);
        void *q = aligned_alloc(al, n);
        if (!q) throw std::runtime_error("out of memory");
        raw.emplace_back(q, n);
        return (uint8_t *)q;
    }
    bool pin(fadehip_ctx *c) {  // false: fadehip_last_error(c) says why
        for (auto &rb : raw) {
            if (fadehip_host_register(c, rb.first, rb.second)) return false;
            pinned.push_back(rb.first);
        }
        return true;
    }
    void unpin(fadehip_ctx *c) { for (void *p : pinned) fadehip_host_free(c, p); }
    ~Staging() { for (auto &rb : raw) free(rb.first); }
};

// Threads when -t is not given: the CPUs this process may actually use — its affinity mask and, in a container, the
// cgroup's CPU quota (a 16-CPU share of a 256-thread host must not get 255 threads) — at most 64.
static int default_threads(int cap = 64) {
    int n = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min(n > 0 ? n : CPU_COUNT(&set), CPU_COUNT(&set));
    auto quota = [](const char *path, const char *period_path) -> double {
        FILE *f = fopen(path, "r");
        if (!f) return 0;
        char a[64] = "", b[64] = "";
        const int got = fscanf(f, "%63s %63s", a, b);
        fclose(f);
        if (got < 1 || strcmp(a, "max") == 0 || atof(a) <= 0) return 0;
        double period = got == 2 ? atof(b) : 0;
        if (period_path) {
            period = 0;
            if (FILE *g = fopen(period_path, "r")) {
                if (fscanf(g, "%lf", &period) != 1) period = 0;
                fclose(g);
            }
        }
        return period > 0 ? atof(a) / period : 0;
    };
    double q = quota("/sys/fs/cgroup/cpu.max", nullptr);  // cgroup v2: "<quota|max> <period>"
    if (q <= 0) q = quota("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us");  // v1
    if (q > 0) n = std::min(n, (int)(q + 0.999));
    return std::max(1, std::min(n, cap));
}

// seconds since the kernel started this process (/proc/self/stat field 22 against /proc/uptime), for -T only
static double since_process_start() {
    FILE *f = fopen("/proc/self/stat", "r");
    if (!f) return 0;
    char buf[2048];
    const size_t n = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[n] = 0;
    const char *p = strrchr(buf, ')');  // comm may contain spaces
    unsigned long long start = 0;
    if (!p) return 0;
    p += 2;
    for (int field = 3; field < 22 && p; field++) { p = strchr(p, ' '); if (p) p++; }
    if (!p || sscanf(p, "%llu", &start) != 1) return 0;
    double up = 0;
    f = fopen("/proc/uptime", "r");
    if (!f) return 0;
    if (fscanf(f, "%lf", &up) != 1) up = 0;
    fclose(f);
    return up - (double)start / (double)sysconf(_SC_CLK_TCK);
}

// The genome of an annotate run (anno.d:23 opens an IndexedFastaFile).  With <fasta>.fai beside the file — unless
// FADE_FASTA_INDEX=0, or the file is gzip without BGZF framing — prepare() only parses the index and upload() hands the file to
// the library, which reads it through the index while the device packs it (fadehip_genome_upload_fasta): no residue passes
// through this program.  In every other case the whole file is read into strings and uploaded from them, as before.  Either
// way the @SQ names and lengths are held against the FASTA first.
struct GenomeSource {
    bool indexed = false;
    std::string fasta, fai_path;
    Fasta fa;
    std::vector<fadehip_fai_entry> entries;
    std::vector<int64_t> lens;
    std::vector<int64_t> have;  // bases the FASTA holds of each contig of the header (`fade out -c --calmd` holds LN against it)
    std::vector<const uint8_t *> ptrs;
    const char *who = "fade annotate";
    double prepare_s = 0, upload_s = 0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

    // 0, or 1 with the reason on stderr (a file that cannot be read throws, as load_fasta does)
    int prepare(const std::string &path, const std::vector<std::string> &sq_names, const std::vector<int64_t> &sq_lens) {
        const double t0 = now();
        fasta = path;
        fai_path = path + ".fai";
        Fai fai;
        const char *sw = getenv("FADE_FASTA_INDEX");
        indexed = !(sw && strcmp(sw, "0") == 0) && !is_plain_gzip(path) && load_fai(fai_path, fai);
        if (!indexed) fa = load_fasta(path);  // anno.d:23
        const std::vector<std::string> &names = indexed ? fai.names : fa.names;
        lens.resize(sq_names.size());
        have.assign(sq_names.size(), 0);
        ptrs.assign(sq_names.size(), nullptr);
        entries.resize(indexed ? sq_names.size() : 0);
        std::unordered_map<std::string, size_t> by_name;
        for (size_t q = names.size(); q-- > 0;) by_name[names[q]] = q;  // (the first of equal names, as a linear search finds it)
        // contigs of the BAM header, in tid order, must be present in the FASTA (fetchSequence by name, analysis.d:63)
        for (size_t k = 0; k < sq_names.size(); k++) {
            auto it = by_name.find(sq_names[k]);
            if (it == by_name.end()) {
                fprintf(stderr, "[E::%s] reference %s of the BAM header is not in %s\n", who, sq_names[k].c_str(), path.c_str());
                return 1;
            }
            const size_t q = it->second;
            // analysis.d:55-59 clamps the window at the header's targetLength; the FASTA may be longer, never shorter
            const size_t have = indexed ? (size_t)fai.length[q] : fa.seqs[q].size();
            this->have[k] = (int64_t)have;
            if ((int64_t)have < sq_lens[k]) {
                fprintf(stderr, "[E::%s] %s is shorter in the FASTA (%zu) than in the header (%lld)\n", who, sq_names[k].c_str(), have, (long long)sq_lens[k]);
                return 1;
            }
            lens[k] = sq_lens[k];
            if (indexed) entries[k] = fadehip_fai_entry{sq_lens[k], fai.offset[q], fai.line_bases[q], fai.line_width[q]};
            else ptrs[k] = (const uint8_t *)fa.seqs[q].data();
        }
        prepare_s += now() - t0;
        return 0;
    }
    int upload(fadehip_ctx *ctx) {
        const double t0 = now();
        if (indexed) {
            if (fadehip_genome_upload_fasta(ctx, fasta.c_str(), (int32_t)entries.size(), entries.data())) {
                fprintf(stderr, "[E::%s] genome upload through the index %s: %s\n", who, fai_path.c_str(), fadehip_last_error(ctx));
                return 1;
            }
        } else if (fadehip_genome_upload(ctx, (int)lens.size(), lens.data(), ptrs.data())) {
            fprintf(stderr, "[E::%s] genome upload: %s\n", who, fadehip_last_error(ctx));
            return 1;
        }
        upload_s += now() - t0;
        return 0;
    }
    void report() const {
        long hwm_kb = 0;  // what the host has held at the most so far: the text of the FASTA, or the library's two chunks
        if (FILE *f = fopen("/proc/self/status", "r")) {
            char line[256];
            while (fgets(line, sizeof line, f)) sscanf(line, "VmHWM: %ld", &hwm_kb);
            fclose(f);
        }
        fprintf(stderr, "[timing] genome: %s, %.3f s to read and match, %.3f s to upload; since process start %.3f s (genome resident), host peak %ld MB so far\n",
                indexed ? "indexed FASTA path (.fai; the library reads the file, the device packs it)" : "whole-file FASTA loader (no index used)", prepare_s,
                upload_s, since_process_start(), hwm_kb / 1024);
    }
};

// ------------------------------------------------------------------ lanes: one process per GPU
// `fade annotate --gpus N` on a BAM file: N lanes, each a process of its own with its own reader, device and writer, on
// disjoint BGZF virtual-offset ranges of the input; no lane sees another's records, the only exchange
// is the final sum of the stats.d counters (RCCL when the lanes sit on distinct devices).  The parent never touches the
// GPU: it cuts the file, starts the lanes, and puts their outputs together — BGZF blocks concatenate.
struct LaneEnv {
    bool on = false;
    int k = 0, n = 1, device = 0, rccl = 0;
    bool shard = false;  // --out-shards: this lane writes a complete file (header and end-of-file block of its own)
    LaneRange range;
    std::string cl, status_path, id_path;
};
static LaneEnv lane_env() {
    LaneEnv e;
    const char *l = getenv("FADE_LANE");
    if (!l) return e;
    unsigned long long a = 0, b = 0, c = 0, d = 0;
    if (sscanf(l, "%d/%d:%d:%d:%llu:%llu:%llu:%llu", &e.k, &e.n, &e.device, &e.rccl, &a, &b, &c, &d) != 8) return e;
    e.on = true;
    e.range.on = true;
    e.range.coff_start = a;
    e.range.first_rec = b;
    e.range.coff_end = c;
    e.range.end_rec = d;
    if (const char *v = getenv("FADE_LANE_CL")) e.cl = v;
    if (const char *v = getenv("FADE_LANE_STATUS")) e.status_path = v;
    if (const char *v = getenv("FADE_LANE_NCCL_ID")) e.id_path = v;
    if (const char *v = getenv("FADE_LANE_SHARD")) e.shard = atoi(v) != 0;
    return e;
}

// a plausible BAM record at buf[o ..): the checks a splitter can make without the chain from the start of the file
static bool plausible_record(const uint8_t *buf, size_t n, size_t o, int n_ref, size_t *next) {
    if (o + 36 > n) return false;
    uint32_t bs;
    memcpy(&bs, buf + o, 4);
    if (bs < 32 || bs > (1u << 24)) return false;
    const RecView v(buf + o + 4, std::min<size_t>(bs, n - o - 4));
    if (v.tid() < -1 || v.tid() >= n_ref || v.mtid() < -1 || v.mtid() >= n_ref || v.pos() < -1 || v.mpos() < -1) return false;
    const size_t lq = (size_t)v.l_qname();
    if (lq < 1 || v.l_seq() < 0) return false;
    const size_t need = 32 + lq + 4 * (size_t)v.n_cigar() + ((size_t)v.l_seq() + 1) / 2 + (size_t)v.l_seq();
    if (need > bs) return false;
    if (o + 4 + 32 + lq <= n) {
        const uint8_t *q = buf + o + 4 + 32;
        if (q[lq - 1] != 0) return false;
        for (size_t k = 0; k + 1 < lq; k++)
            if (q[k] < 33 || q[k] > 126) return false;
    }
    *next = o + 4 + bs;
    return true;
}

static int annotate_lanes_main(const std::string &cl, const Opts &o, bool *fall_back) {
    *fall_back = true;  // until the lanes have been started, a single-lane run can still take over
    const int n_lanes = o.gpus;
    const std::string &path = o.pos[1];
    struct stat sb;
    if (path == "-" || stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return 1;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return 1;
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    // the BGZF blocks of the file
    std::vector<uint64_t> boff;
    std::vector<uint32_t> bsz;
    {
        uint64_t at = 0;
        uint32_t bs;
        for (MemberAt r; (r = bgzf_member_at(fileno(f), at, &bs, nullptr)) != MemberAt::NO_HEADER; at += bs) {
            if (r == MemberAt::NOT_BGZF) return 1;  // not BGZF: one lane reads it
            boff.push_back(at);
            bsz.push_back(bs);
        }
    }
    if (boff.size() < (size_t)(8 * n_lanes)) return 1;  // too small to be worth cutting
    auto isize_of = [&](size_t b) -> uint32_t {
        uint32_t bs, isz = 0;  // (0 where the trailer cannot be read)
        bgzf_member_at(fileno(f), boff[b], &bs, &isz);
        return isz;
    };
    auto inflate_blocks = [&](size_t b0, size_t nb, std::vector<uint8_t> &out, std::vector<size_t> &start) -> bool {
        out.clear();
        start.clear();
        for (size_t b = b0; b < std::min(b0 + nb, boff.size()); b++) {
            std::vector<uint8_t> comp(bsz[b]);
            if (pread(fileno(f), comp.data(), comp.size(), (off_t)boff[b]) != (ssize_t)comp.size()) return false;
            const size_t xlen = (size_t)comp[10] | ((size_t)comp[11] << 8), hl = 12 + xlen;
            if (comp.size() < hl + 8) return false;
            const uint32_t isz = isize_of(b);
            if (isz > 65536) return false;
            start.push_back(out.size());
            const size_t base = out.size();
            out.resize(base + isz);
            z_stream zs;
            memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -15) != Z_OK) return false;
            zs.next_in = comp.data() + hl;
            zs.avail_in = (uInt)(comp.size() - hl - 8);
            zs.next_out = out.data() + base;
            zs.avail_out = isz;
            const int rc = inflate(&zs, Z_FINISH);
            inflateEnd(&zs);
            if (rc != Z_STREAM_END || zs.total_out != isz) return false;
        }
        start.push_back(out.size());
        return true;
    };
    // header, number of references
    int n_ref = 0;
    size_t hdr_bytes = 0;
    {
        Pool small(1);
        Reader rd(path, &small);
        if (!rd.is_bam()) return 1;
        n_ref = (int)rd.header().names.size();
        hdr_bytes = rd.bam_header_bytes();
    }
    // lane starts: lane 0 behind the header; lane k at the first offset of block k * nblk / N from which a chain of
    // plausible records runs through the next blocks.  The guess is checked for real by the lane before, whose own chain
    // must end exactly there.
    std::vector<LaneRange> lr((size_t)n_lanes);
    {
        uint64_t coff = 0;
        uint32_t first_rec = 0, bs, isz;
        if (!locate_first_record(fileno(f), (uint64_t)sb.st_size, hdr_bytes, &coff, &first_rec)) return 1;
        // (where the header fills every member the single-lane drivers start at the last one; here no member is left for a lane)
        if (bgzf_member_at(fileno(f), coff, &bs, &isz) != MemberAt::OK || first_rec >= isz) return 1;
        lr[0].on = true;
        lr[0].coff_start = coff;
        lr[0].first_rec = first_rec;
    }
    for (int k = 1; k < n_lanes; k++) {
        bool found = false;
        for (size_t b = boff.size() * (size_t)k / (size_t)n_lanes; b + 4 < boff.size() && !found; b++) {
            std::vector<uint8_t> buf;
            std::vector<size_t> st;
            if (!inflate_blocks(b, 4, buf, st)) return 1;
            for (size_t o0 = 0; o0 < st[1] && !found; o0++) {
                size_t o = o0, nx = 0;
                int cnt = 0;
                while (plausible_record(buf.data(), buf.size(), o, n_ref, &nx) && nx <= buf.size()) { o = nx; cnt++; }
                // the chain must run to the end of what was inflated (the last record may stick out) through at least 4 records
                if (cnt >= 4 && (o == buf.size() || (o + 4 <= buf.size() && plausible_record(buf.data(), buf.size(), o, n_ref, &nx)) || buf.size() - o < 36)) {
                    lr[(size_t)k].on = true;
                    lr[(size_t)k].coff_start = boff[b];
                    lr[(size_t)k].first_rec = o0;
                    found = true;
                }
            }
        }
        if (!found) return 1;
        lr[(size_t)k - 1].coff_end = lr[(size_t)k].coff_start;
        lr[(size_t)k - 1].end_rec = lr[(size_t)k].first_rec;
    }
    // devices: 0 .. N-1, or FADE_DEVICE_MAP (tests put two lanes on one device; RCCL wants distinct devices)
    std::vector<int> devmap((size_t)n_lanes);
    for (int d = 0; d < n_lanes; d++) devmap[(size_t)d] = d;
    bool distinct = true;
    if (const char *dm = getenv("FADE_DEVICE_MAP")) {
        int d = 0;
        for (const char *q = dm; *q && d < n_lanes; d++) {
            devmap[(size_t)d] = atoi(q);
            q = strchr(q, ',');
            if (!q) break;
            q++;
        }
        for (int a = 0; a < n_lanes; a++)
            for (int b2 = a + 1; b2 < n_lanes; b2++)
                if (devmap[(size_t)a] == devmap[(size_t)b2]) distinct = false;
    }
    // (a lane is a whole `fade annotate` of its own: its share of the cores, up to the 64 a single run takes — an 8-GPU node
    // has them)
    const int threads_each = std::max(1, std::min(64, (o.threads > 0 ? o.threads : default_threads(64 * n_lanes)) / n_lanes));
    const bool shards = !o.out_shards.empty();
    // Where the lanes write.  --out-shards: every lane a complete file of its own (header, its records, end-of-file block),
    // nothing is merged (BASELINE config 4: "sharded per GPU").  Otherwise ONE stream on stdout: lane 0 writes straight into
    // it (header first), lanes 1 .. N-1 into files of a private directory that this process forwards WHILE the lanes run —
    // into their final place at once when stdout is a file that can be written at an offset (a lane's place is known as soon
    // as the lanes before it have ended, and the copies of all lanes proceed side by side), one lane after the other when it
    // is a pipe.
    char dir[512] = "";
    {
        const char *tmpd = getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp";
        snprintf(dir, sizeof dir, "%s/fade_lanes_XXXXXX", tmpd);
        if (!mkdtemp(dir)) { fprintf(stderr, "[E::fade annotate] cannot make a directory under %s: %s\n", tmpd, strerror(errno)); return 1; }  // (0700, a name nobody can guess)
    }
    std::vector<std::string> outp((size_t)n_lanes), stp((size_t)n_lanes);
    std::vector<int> ofd((size_t)n_lanes, -1);  // lanes 1 ..: this process's read side of the lane's file
    std::vector<pid_t> pids((size_t)n_lanes, -1);
    const std::string idp = std::string(dir) + "/ncclid";
    auto cleanup = [&] {
        for (int k = 0; k < n_lanes; k++) {
            if (ofd[(size_t)k] >= 0) close(ofd[(size_t)k]);
            if (!shards && !outp[(size_t)k].empty()) unlink(outp[(size_t)k].c_str());
            unlink(stp[(size_t)k].c_str());
        }
        unlink(idp.c_str());
        unlink((idp + ".tmp").c_str());
        rmdir(dir);
    };
    *fall_back = false;  // from here on the lanes own the run: a failure is reported, nothing is run twice
    if (o.timing)
        for (int k = 0; k < n_lanes; k++)
            fprintf(stderr, "[timing] lane %d of %d: device %d, blocks from file offset %llu (first record at +%llu) to %llu (+%llu)\n", k, n_lanes, devmap[(size_t)k],
                    (unsigned long long)lr[(size_t)k].coff_start, (unsigned long long)lr[(size_t)k].first_rec, (unsigned long long)lr[(size_t)k].coff_end,
                    (unsigned long long)lr[(size_t)k].end_rec);
    fprintf(stderr, "[W::fade annotate] Output SAM/BAM will not be sorted (regardless of prior sorting)\n");
    fflush(stdout);
    const auto t_spawn = std::chrono::steady_clock::now();
    auto secs = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_spawn).count(); };
    bool ok = true;
    for (int k = 0; k < n_lanes; k++) stp[(size_t)k] = std::string(dir) + "/" + std::to_string(k) + ".status";
    // (FADE_LANES_LIVE=m: at most m lanes at a time, the next one starts when one ends — for boxes that allow few processes
    // on a device, i.e. tests that put eight lanes on one GPU)
    const int live_cap = std::max(1, std::min(n_lanes, getenv("FADE_LANES_LIVE") ? atoi(getenv("FADE_LANES_LIVE")) : n_lanes));
    int next_lane = 0;
    // the lanes sum their counters among themselves over RCCL when each has a device of its own and all of them run at once
    // (FADE_LANES_RCCL=1 asks for it regardless: a test of what RCCL says to two ranks on one device; =0 leaves the sum to
    // this process, which adds up the lanes' reports either way)
    const char *rccl_env = getenv("FADE_LANES_RCCL");
    const bool lanes_rccl = live_cap == n_lanes && (rccl_env ? atoi(rccl_env) != 0 : distinct);
    auto start_lane = [&](int k) -> bool {
        int wfd = -1;  // the lane's stdout (lane 0 of a merged run: this process's own)
        if (shards) {
            outp[(size_t)k] = o.out_shards + "." + std::to_string(k) + ((o.bam || o.ubam) ? ".bam" : ".sam");
            wfd = open(outp[(size_t)k].c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        } else if (k > 0) {
            outp[(size_t)k] = std::string(dir) + "/" + std::to_string(k) + ".out";
            wfd = open(outp[(size_t)k].c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
            if (wfd >= 0) ofd[(size_t)k] = open(outp[(size_t)k].c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
        }
        if ((shards || k > 0) && (wfd < 0 || (!shards && ofd[(size_t)k] < 0))) {
            fprintf(stderr, "[E::fade annotate] cannot create %s: %s\n", outp[(size_t)k].c_str(), strerror(errno));
            if (wfd >= 0) close(wfd);
            return false;
        }
        char lane[256];
        snprintf(lane, sizeof lane, "%d/%d:%d:%d:%llu:%llu:%llu:%llu", k, n_lanes, devmap[(size_t)k], lanes_rccl ? 1 : 0, (unsigned long long)lr[(size_t)k].coff_start,
                 (unsigned long long)lr[(size_t)k].first_rec, (unsigned long long)lr[(size_t)k].coff_end, (unsigned long long)lr[(size_t)k].end_rec);
        std::vector<std::string> envs;
        for (char **e = environ; *e; e++)
            if (strncmp(*e, "FADE_LANE", 9) != 0) envs.push_back(*e);
        envs.push_back(std::string("FADE_LANE=") + lane);
        envs.push_back("FADE_LANE_CL=" + cl);
        envs.push_back("FADE_LANE_STATUS=" + stp[(size_t)k]);
        envs.push_back("FADE_LANE_NCCL_ID=" + idp);
        if (shards) envs.push_back("FADE_LANE_SHARD=1");
        // (a lane whose file this process reads while it grows must write it front to back: side-by-side pwrites would leave
        // holes that read as zeros for a moment)
        if (!shards && k > 0) {
            for (auto &e : envs)
                if (e.rfind("FADE_BAM_WRITERS=", 0) == 0) e = "FADE_BAM_WRITERS=0";
            envs.push_back("FADE_BAM_WRITERS=0");
        }
        std::vector<char *> envp;
        for (auto &e : envs) envp.push_back(const_cast<char *>(e.c_str()));
        envp.push_back(nullptr);
        std::vector<std::string> args = {"/proc/self/exe", "annotate", "-t", std::to_string(threads_each), "--min-length", std::to_string(o.floor_len),
                                         "-w", std::to_string(o.window), "--batch", std::to_string(o.batch)};
        if (o.bam) args.push_back("-b");
        if (o.ubam) args.push_back("-u");
        if (o.clip) args.push_back("-c");
        if (o.timing) args.push_back("--timing");
        args.push_back(o.pos[1]);
        args.push_back(o.pos[2]);
        std::vector<char *> argv;
        for (auto &a : args) argv.push_back(const_cast<char *>(a.c_str()));
        argv.push_back(nullptr);
        posix_spawn_file_actions_t fa;
        posix_spawn_file_actions_init(&fa);
        if (wfd >= 0) posix_spawn_file_actions_adddup2(&fa, wfd, 1);
        const int rc = posix_spawn(&pids[(size_t)k], "/proc/self/exe", &fa, nullptr, argv.data(), envp.data());
        posix_spawn_file_actions_destroy(&fa);
        if (wfd >= 0) close(wfd);
        if (rc != 0) {
            fprintf(stderr, "[E::fade annotate] cannot start lane %d: %s\n", k, strerror(rc));
            pids[(size_t)k] = -1;
            return false;
        }
        return true;
    };
    while (ok && next_lane < live_cap) ok = start_lane(next_lane++);
    // ---- the lanes run; their outputs are put together meanwhile
    struct Merge {
        std::mutex m;
        std::condition_variable cv;
        std::vector<char> ended;      // lane k has ended well: its file has its final size
        std::vector<uint64_t> size;   // ... which is this
        std::vector<char> copied;     // lane k's bytes are all in the output
        bool abort = false;
        std::string err;
    } mg;
    mg.ended.assign((size_t)n_lanes, 0);
    mg.size.assign((size_t)n_lanes, 0);
    mg.copied.assign((size_t)n_lanes, 0);
    struct stat so;
    const int oflags = fcntl(1, F_GETFL);
    const off_t base = lseek(1, 0, SEEK_CUR);
    // (FADE_LANES_MERGE=stream: one lane after the other even into a file — what a pipe gets; tests compare the two)
    const bool placed = !shards && fstat(1, &so) == 0 && S_ISREG(so.st_mode) && base >= 0 && oflags >= 0 && !(oflags & O_APPEND) &&
                        !(getenv("FADE_LANES_MERGE") && strcmp(getenv("FADE_LANES_MERGE"), "stream") == 0);
    std::vector<double> t_end((size_t)n_lanes, 0), t_copied((size_t)n_lanes, 0);
    std::vector<std::thread> copiers;
    if (!shards && ok)
        for (int k = 1; k < n_lanes; k++)
            copiers.emplace_back([&, k] {
                // lane k's bytes may go out once their place is known: behind the FINAL sizes of lanes 0 .. k-1 (placed), or
                // behind the last byte of lane k-1 in the stream
                uint64_t at = 0;
                {
                    std::unique_lock<std::mutex> l(mg.m);
                    mg.cv.wait(l, [&] {
                        if (mg.abort) return true;
                        for (int j = 0; j < k; j++)
                            if (!mg.ended[(size_t)j] || (!placed && !mg.copied[(size_t)j])) return false;
                        return true;
                    });
                    if (mg.abort) return;
                    for (int j = 0; j < k; j++) at += mg.size[(size_t)j];
                }
                std::vector<char> buf((size_t)4 << 20);
                uint64_t pos = 0;
                for (;;) {
                    const ssize_t got = pread(ofd[(size_t)k], buf.data(), buf.size(), (off_t)pos);
                    if (got < 0 && errno == EINTR) continue;
                    if (got < 0) { std::lock_guard<std::mutex> l(mg.m); mg.abort = true; mg.err = std::string("read error on a lane's output: ") + strerror(errno); mg.cv.notify_all(); return; }
                    if (got == 0) {
                        std::unique_lock<std::mutex> l(mg.m);
                        if (mg.abort) return;
                        if (mg.ended[(size_t)k] && pos >= mg.size[(size_t)k]) break;
                        mg.cv.wait_for(l, std::chrono::microseconds(300));  // (the lane is still writing)
                        continue;
                    }
                    size_t done = 0;
                    while (done < (size_t)got) {
                        const ssize_t w = placed ? pwrite(1, buf.data() + done, (size_t)got - done, (off_t)((uint64_t)base + at + pos + done))
                                                 : write(1, buf.data() + done, (size_t)got - done);
                        if (w < 0 && errno == EINTR) continue;
                        if (w <= 0) { std::lock_guard<std::mutex> l(mg.m); mg.abort = true; mg.err = "write error on the output stream"; mg.cv.notify_all(); return; }
                        done += (size_t)w;
                    }
                    pos += (uint64_t)got;
                }
                std::lock_guard<std::mutex> l(mg.m);
                mg.copied[(size_t)k] = 1;
                t_copied[(size_t)k] = secs();
                mg.cv.notify_all();
            });
    // reap whichever lane ends next; one that fails takes the others with it (a lane waiting in ncclCommInitRank for a dead
    // peer would wait for ever)
    int live = 0;
    for (int k = 0; k < n_lanes; k++) live += pids[(size_t)k] > 0;
    auto kill_all = [&] {
        for (int k = 0; k < n_lanes; k++)
            if (pids[(size_t)k] > 0) kill(pids[(size_t)k], SIGKILL);
    };
    if (!ok) kill_all();
    while (live > 0) {
        int st = 0;
        const pid_t p = waitpid(-1, &st, 0);
        if (p < 0) { if (errno == EINTR) continue; break; }
        int k = 0;
        while (k < n_lanes && pids[(size_t)k] != p) k++;
        if (k == n_lanes) continue;
        pids[(size_t)k] = -1;
        live--;
        const bool good = WIFEXITED(st) && WEXITSTATUS(st) == 0;
        bool aborted;
        {
            std::lock_guard<std::mutex> l(mg.m);
            aborted = mg.abort;
        }
        if (!good || aborted) {
            if (ok && !good) fprintf(stderr, "[E::fade annotate] lane %d of %d failed\n", k, n_lanes);
            if (ok) {
                ok = false;
                kill_all();
                std::lock_guard<std::mutex> l(mg.m);
                mg.abort = true;
                mg.cv.notify_all();
            }
            continue;
        }
        uint64_t sz = 0;
        if (!shards) {
            if (k == 0) {
                const off_t e = lseek(1, 0, SEEK_CUR);  // (lane 0 wrote through this very file description)
                sz = placed && e >= base ? (uint64_t)(e - base) : 0;
            } else {
                struct stat sb2;
                if (fstat(ofd[(size_t)k], &sb2) == 0) sz = (uint64_t)sb2.st_size;
            }
        }
        {
            std::lock_guard<std::mutex> l(mg.m);
            mg.ended[(size_t)k] = 1;
            mg.size[(size_t)k] = sz;
            if (k == 0) { mg.copied[0] = 1; t_copied[0] = secs(); }
            t_end[(size_t)k] = secs();
            mg.cv.notify_all();
        }
        if (ok && next_lane < n_lanes) {
            if (start_lane(next_lane++)) live++;
            else {
                ok = false;
                kill_all();
                std::lock_guard<std::mutex> l(mg.m);
                mg.abort = true;
                mg.cv.notify_all();
            }
        }
    }
    for (auto &t : copiers) t.join();
    if (!mg.err.empty()) { fprintf(stderr, "[E::fade annotate] %s\n", mg.err.c_str()); ok = false; }
    int64_t totals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t n_oversize = 0;
    for (int k = 0; k < n_lanes && ok; k++) {
        FILE *s = fopen(stp[(size_t)k].c_str(), "r");
        long long v[9], red[8];
        if (!s || fscanf(s, "%lld %lld %lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8]) != 9) {
            fprintf(stderr, "[E::fade annotate] lane %d left no report\n", k);
            ok = false;
        } else {
            for (int q = 0; q < 8; q++) totals[q] += v[q];
            n_oversize += v[8];
            // lanes on distinct devices have summed the counters among themselves (RCCL): every lane then holds the totals
            if (lanes_rccl && fscanf(s, "%lld %lld %lld %lld %lld %lld %lld %lld", &red[0], &red[1], &red[2], &red[3], &red[4], &red[5], &red[6], &red[7]) == 8 && k == n_lanes - 1)
                for (int q = 0; q < 8; q++)
                    if (red[q] != totals[q]) { fprintf(stderr, "[E::fade annotate] the lanes' RCCL sum differs from the sum of their reports\n"); ok = false; break; }
        }
        if (s) fclose(s);
    }
    if (!ok) { cleanup(); return 1; }
    if (!shards) {
        if (placed) {
            uint64_t all = 0;
            for (int k = 0; k < n_lanes; k++) all += mg.size[(size_t)k];
            if (lseek(1, (off_t)((uint64_t)base + all), SEEK_SET) < 0) { fprintf(stderr, "[E::fade annotate] cannot seek the output: %s\n", strerror(errno)); cleanup(); return 1; }
        }
        if (o.bam || o.ubam) {
            size_t done = 0;
            while (done < sizeof BGZF_EOF) {
                const ssize_t w = write(1, BGZF_EOF + done, sizeof BGZF_EOF - done);
                if (w < 0 && errno == EINTR) continue;
                if (w <= 0) { fprintf(stderr, "[E::fade annotate] write error on the output stream\n"); cleanup(); return 1; }
                done += (size_t)w;
            }
        }
    }
    if (o.timing) {
        double last_end = 0, last_copy = 0;
        for (int k = 0; k < n_lanes; k++) { last_end = std::max(last_end, t_end[(size_t)k]); last_copy = std::max(last_copy, t_copied[(size_t)k]); }
        fprintf(stderr, "[timing] lanes: %s; the last lane ended after %.3f s, the last byte was in place after %.3f s (merge behind the lanes: %.3f s);",
                shards ? "a complete file per lane, nothing merged" : placed ? "lanes 1.. copied into their final place while the lanes ran" : "lanes forwarded in order while the lanes ran",
                last_end, shards ? last_end : last_copy, shards ? 0.0 : std::max(0.0, last_copy - last_end));
        for (int k = 0; k < n_lanes; k++) fprintf(stderr, " lane %d ended %.3f%s", k, t_end[(size_t)k], k + 1 < n_lanes ? "," : "\n");
    }
    cleanup();
    if (n_oversize)
        fprintf(stderr, "[W::fade annotate] %lld soft-clipped reads were not re-aligned: read or window beyond the kernels' limits\n", (long long)n_oversize);
    if (o.stats) {
        const double rc = (double)std::max<int64_t>(totals[0], 1);
        fprintf(stderr, "read count:\t%lld\nClipped %%:\t%g\n%% With Supplementary alns:\t%g\nArtifact rate:\t%g\n"
                        "%% With Supplementary alns and artifacts:\t%g\nArtifact rate left only:\t%g\nArtifact rate right only:\t%g\n",
                (long long)totals[0], totals[1] / rc, totals[2] / rc, totals[4] / rc, totals[3] / rc, totals[6] / rc, totals[7] / rc);
    }
    return 0;
}

static int numerically_aware_cmp(std::string a, std::string b);

// `fade annotate --eject`: filter.d:216-220 — the first ten records decide whether the input looks name-sorted (annotate keeps
// names and order, so these are the names `fade out` would see); the matching line of filter.d:218 / 248 is printed once
static bool eject_mode_grouped(const std::vector<std::string> &first_names) {
    bool sorted = true;
    for (size_t k = 1; k < std::min<size_t>(first_names.size(), 10); k++)
        if (numerically_aware_cmp(first_names[k], first_names[k - 1]) < 0) sorted = false;
    if (sorted) fprintf(stderr, "[W::fade-out] Output looks name-sorted, ejecting all reads with same readname if any have an artifact\n");
    else fprintf(stderr, "[W::fade-out] Output doesn't look name-sorted, ejecting by only reads with an artifact\n");
    return sorted;
}

// filter.d:221-265 on the host pipeline's writer side, by the batches' rs (this run's, never an rs tag a record brought):
// the records of a chunk come in with their tags on, the ones that stay go to `out`.  The mode is decided when ten records
// have been seen (or the input has ended); in grouped mode the last open group is held across chunks and flushed at the end.
struct Ejector {
    int mode = -1;  // -1: not decided yet, 0: record by record, 1: name groups
    std::vector<std::pair<Rec, bool>> waiting;  // records seen before the decision
    std::vector<Rec> group;
    bool group_art = false;
    void flush_group(std::vector<Rec> &out) {
        if (!group_art)
            for (Rec &r : group) out.push_back(std::move(r));
        group.clear();
        group_art = false;
    }
    void take(Rec &&r, bool art, std::vector<Rec> &out) {
        if (mode == 0) {
            if (!art) out.push_back(std::move(r));
            return;
        }
        if (!group.empty() && strcmp(group.back().qname(), r.qname()) != 0) flush_group(out);
        group.push_back(std::move(r));
        group_art |= art;
    }
    void decide(std::vector<Rec> &out) {
        std::vector<std::string> names;
        for (size_t k = 0; k < std::min<size_t>(waiting.size(), 10); k++) names.push_back(waiting[k].first.qname());
        mode = eject_mode_grouped(names) ? 1 : 0;
        for (auto &w : waiting) take(std::move(w.first), w.second, out);
        waiting.clear();
    }
    void add(Rec &&r, bool art, std::vector<Rec> &out) {
        if (mode >= 0) { take(std::move(r), art, out); return; }
        waiting.emplace_back(std::move(r), art);
        if (waiting.size() >= 10) decide(out);
    }
    void finish(std::vector<Rec> &out) {
        if (mode < 0) decide(out);
        flush_group(out);
    }
};

// `fade annotate -b in.bam ref.fa` with the whole file path on the device (fadehip_bam_*): this process reads compressed
// bytes and writes compressed bytes; inflate, framing, annotateTask, the tags and deflate are kernels.  Three threads
// around the library's two halves: [reader: file -> pinned buffers, cut at BGZF member boundaries] -> [this thread:
// front] -> [back thread: back] -> [writer thread: fwrite].  FADE_BAM_DEVICE=0 (or any input that is not a BAM file, any
// output that is not BAM, --gpus N) takes the host pipeline of annotate_main instead.
static int annotate_stream_main(const std::string &cl, const Opts &o, bool *fall_back) {
    *fall_back = true;
    const LaneEnv lane = lane_env();  // set when this process is one lane of a `--gpus N` run (annotate_lanes_main): a range of the file
    const std::string &path = o.pos[1];
    struct stat sb;
    if (!(o.bam || o.ubam) || path == "-" || stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return 1;
    StageClock ck_total, ck_fasta, ck_upload, ck_front, ck_back, ck_fwrite, ck_fread, ck_inflate;
    ck_fasta.name = "fasta"; ck_upload.name = "upload"; ck_front.name = "front"; ck_back.name = "back"; ck_fwrite.name = "fwrite"; ck_fread.name = "fread"; ck_inflate.name = "inflate";
    ck_total.start();
    const int nthreads = o.threads > 0 ? o.threads : default_threads();
    // Who inflates: the device (FADE_BAM_INFLATE=device: only compressed bytes cross PCIe, the host cores stay free) or this
    // process's pool (host, the default with 8 threads or more: the cores have nothing else to do here, and the device then
    // spends its time on the compressor, which is its slowest kernel).
    const char *inf_env = getenv("FADE_BAM_INFLATE");
    const bool host_inflate = inf_env ? strcmp(inf_env, "host") == 0 : nthreads >= 8;
    Pool pool(host_inflate ? nthreads : std::min(nthreads, 4));
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return 1;
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    // header; the member that holds the first record and the record's offset in its payload
    Header hdr;
    uint64_t coff = 0;
    uint32_t first_rec = 0;
    std::vector<std::string> eject_names;  // --eject: the names of the first ten records
    try {
        Reader rd(path, &pool);
        if (!rd.is_bam()) return 1;
        hdr = rd.header();
        const size_t hdr_bytes = rd.bam_header_bytes();
        if (o.eject) {  // the front of the file is inflated here anyway: on to the tenth record
            std::vector<Rec> first;
            rd.read_chunk(first, 10);
            for (const Rec &r : first) eject_names.push_back(r.qname());
        }
        if (lane.on) {
            coff = lane.range.coff_start;
            first_rec = (uint32_t)lane.range.first_rec;
            if (first_rec > 65536) return 1;
        } else if (!locate_first_record(fileno(f), (uint64_t)sb.st_size, hdr_bytes, &coff, &first_rec)) {
            return 1;  // (other gzip subfields first, say: the host path reads it)
        }
    } catch (const std::exception &e) {
        return 1;  // the host path reports what is wrong with the file
    }
    *fall_back = false;
    g_csi_depth = o.csi ? csi_depth_for(hdr) : 0;
    g_csi_who = "fade-annotate";
    if (o.timing) fprintf(stderr, "[timing] since process start %.3f s (annotate begins; file path on the device)\n", since_process_start());
    if (!lane.on && !o.sort) fprintf(stderr, "[W::fade annotate] Output SAM/BAM will not be sorted (regardless of prior sorting)\n");
    const bool eject_grouped = o.eject && eject_mode_grouped(eject_names);
    // a lane reads the members in front of coff_end whole and, of the member AT coff_end, the end_rec bytes in front of the next
    // lane's first record
    uint64_t read_end = (uint64_t)sb.st_size;
    uint32_t tail_trim = 0;
    const bool limited = lane.on && lane.range.coff_end != 0;
    if (limited) {
        read_end = lane.range.coff_end;
        if (lane.range.end_rec > 0) {
            uint32_t bsz, isz;
            const MemberAt r = bgzf_member_at(fileno(f), lane.range.coff_end, &bsz, &isz);
            if (r == MemberAt::NO_HEADER || r == MemberAt::NOT_BGZF) fprintf(stderr, "[E::fade annotate] lane range ends at no BGZF member\n");
            if (r != MemberAt::OK) return 1;
            read_end += bsz;
            // a lane's last member is cut where the next lane's first record starts: by this process when it inflates, by the
            // library (tail_trim) when the device does
            if (lane.range.end_rec > isz) { fprintf(stderr, "[E::fade annotate] lane range ends beyond its last block\n"); return 1; }
            tail_trim = isz - (uint32_t)lane.range.end_rec;
        }
    }
    fadehip_ctx *ctx = nullptr;
    fadehip_bam_stream *st = nullptr;
    fadehip_recstore *store = nullptr;  // --extract-sorted: the run's extract records, on the device
    Staging staging;
    struct Guard {
        fadehip_ctx *&c;
        fadehip_bam_stream *&s;
        fadehip_recstore *&rs;
        Staging &stg;
        ~Guard() {
            if (s) fadehip_bam_close(s);
            if (rs) fadehip_recstore_destroy(rs);
            stg.unpin(c);
            fadehip_destroy(c);
        }
    } guard{ctx, st, store, staging};
    try {
        fadehip_params prm;
        fadehip_params_default(&prm);
        setenv("FADEHIP_TAIL_CUS", "0", 0);  // one batch at a time: no CU-masked stream, fewer queues
        setenv("FADEHIP_BLOCKING_SYNC", "1", 0);  // the threads that wait for the device sleep: the cores are the inflater's
        int device = 0;
        if (lane.on) device = lane.device;
        else if (const char *dm = getenv("FADE_DEVICE_MAP")) device = atoi(dm);
        if (hdr.names.empty()) { fprintf(stderr, "[E::fade annotate] input has no @SQ lines\n"); return 1; }
        // FADE_BAM_CHUNK_MB: bytes per front call — compressed when the device inflates (default 128), inflated when the
        // host does (default 32: the first call starts earlier and the last one drains sooner; 64 and 128 measured slower).
        const size_t chunk = (size_t)std::max(1, getenv("FADE_BAM_CHUNK_MB") ? atoi(getenv("FADE_BAM_CHUNK_MB")) : host_inflate ? 32 : 128) << 20;
        // The device is brought up on a thread of its own, beside everything the host can do without it (the FASTA, the input's
        // first members read and inflated): the ctx (the HIP runtime's own start is most of it), then the stream and what its
        // first calls would otherwise make one by one (fadehip_bam_prepare).  The genome goes up as soon as the ctx is there.
        std::string create_err;
        std::promise<int> ctx_made;
        std::future<int> ctx_ready = ctx_made.get_future();
        std::future<int> creating = std::async(std::launch::async, [&]() -> int {
            if (fadehip_create(&ctx, device, &prm)) { create_err = fadehip_last_error(nullptr); ctx_made.set_value(1); return 1; }
            ctx_made.set_value(0);
            std::vector<const char *> names;
            for (auto &n : hdr.names) names.push_back(n.c_str());
            fadehip_bam_config cfg;
            memset(&cfg, 0, sizeof cfg);
            cfg.floor_len = o.floor_len;
            cfg.window = o.window;
            cfg.n_ref = (int32_t)names.size();
            cfg.ref_names = names.data();
            cfg.first_record = first_rec;
            cfg.tail_trim = host_inflate ? 0 : tail_trim;
            cfg.flags = o.ubam ? FADEHIP_BAM_STORED : 0;  // -u: uncompressed BGZF (util.d:65-76, SAMWriterTypes.UBAM)
            if (o.clip) cfg.flags |= FADEHIP_BAM_CLIP;    // -c: the artifact calls leave hard-clipped
            if (o.keep_sorted) cfg.flags |= FADEHIP_BAM_KEEP_SORTED;  // --keep-sorted: ... at their new coordinates
            if (!o.extract.empty()) cfg.flags |= FADEHIP_BAM_EXTRACT;  // --extract: every call leaves its extract records too
            if (o.eject) cfg.flags |= eject_grouped ? FADEHIP_BAM_EJECT | FADEHIP_BAM_EJECT_GROUPS : FADEHIP_BAM_EJECT;  // --eject
            if (!o.write_index.empty()) cfg.flags |= FADEHIP_BAM_INDEX;  // --write-index: every call leaves its .bai entries too
            if (o.extract_sorted) {  // --extract-sorted: ... and they stay on the device, in a store, until the main output is finished
                cfg.flags |= FADEHIP_BAM_STORE_EXTRACT;
                if (fadehip_recstore_create(ctx, &store)) { create_err = fadehip_last_error(ctx); return 1; }
            }
            if (o.sort) {  // --sort: the MAIN output stays on the device, in a store that measures it under the budget the device allows; the drains compress and index it
                cfg.flags = (cfg.flags & ~(FADEHIP_BAM_STORED | FADEHIP_BAM_INDEX)) | FADEHIP_BAM_STORE_OUTPUT;
                if (fadehip_recstore_create(ctx, &store) || fadehip_recstore_set_budget(store, 0) || fadehip_recstore_measure(store, (int32_t)hdr.lens.size(), hdr.lens.data())) {
                    create_err = fadehip_last_error(ctx);
                    return 1;
                }
            }
            if (fadehip_bam_open(ctx, &cfg, &st)) { create_err = fadehip_last_error(ctx); return 1; }
            if ((cfg.flags & FADEHIP_BAM_INDEX) && IndexFile::stream_geometry(st)) { create_err = fadehip_last_error(ctx); return 1; }  // --csi
            if (store && fadehip_bam_use_recstore(st, store)) { create_err = fadehip_last_error(ctx); return 1; }
            const size_t call_bytes = host_inflate ? chunk : std::min<size_t>(chunk * 3, (size_t)1 << 30);
            if (!(getenv("FADE_BAM_PREPARE") && atoi(getenv("FADE_BAM_PREPARE")) == 0) && fadehip_bam_prepare(st, call_bytes)) { create_err = fadehip_last_error(ctx); return 1; }
            return 0;
        });
        // ---- the stages
        // Compressed bytes are read by a thread of their own, HEAD bytes into a buffer, so that a member cut by the end of one
        // read is completed by copying its beginning in front of the next.
        const size_t ccap = host_inflate ? std::max<size_t>(chunk / 2, 1 << 20) : chunk, HEAD = 65536 + 64;
        constexpr int NBUF = 3;
        struct CBuf { uint8_t *p = nullptr; size_t n = 0; uint64_t off = 0; bool eof = false; std::vector<uint8_t> own; };
        struct In { uint8_t *p = nullptr, *pin = nullptr; size_t n = 0; bool last = false, compressed = false; int cbuf = -1; };
        CBuf cbufs[NBUF];
        In bufs[NBUF];
        // FADE_BAM_DEVICE_SHARE=n: with the pool inflating, every n-th call's members go to the device as they are (inflated by
        // the kernel of FADE_BAM_INFLATE=device): the cores are the bottleneck of a file-to-file run once the device's half is
        // fast, and the device has time to spare for a share of the inflating.  0: none.
        const int dev_share = host_inflate ? std::max(0, getenv("FADE_BAM_DEVICE_SHARE") ? atoi(getenv("FADE_BAM_DEVICE_SHARE")) : 0) : 0;
        std::atomic<int> cbuf_refs[NBUF];
        for (auto &r : cbuf_refs) r = 0;
        // (Reading the members where the page cache has them — the file mapped, its pages entered by MADV_POPULATE_READ —
        // was measured and is slower than pread into a buffer: the pool inflates 20-30 % slower out of the mapping.)
        for (int k = 0; k < NBUF; k++) {
            if (host_inflate) {
                if (dev_share) cbufs[k].p = staging.alloc(HEAD + ccap + 64);  // (some of its members cross PCIe as they are)
                else {
                    cbufs[k].own.resize(HEAD + ccap + 64);
                    cbufs[k].p = cbufs[k].own.data();
                }
                bufs[k].pin = bufs[k].p = staging.alloc(chunk + 65536 + 64);
            } else {
                cbufs[k].p = staging.alloc(HEAD + ccap + 64);  // (handed to front as they are: pinned)
            }
        }
        BoundedQueue<int> q_cfree(NBUF + 1), q_cfull(NBUF + 1), q_free(NBUF + 1), q_full(NBUF + 1), q_done(FADEHIP_BAM_CHUNKS + 1);
        struct OutRef { const uint8_t *p; size_t n; const uint8_t *xp = nullptr; size_t xn = 0; };  // (xp, xn: --extract)
        // A call's bytes stay valid during the next back call only (include/fadehip.h: two staging buffers in turn), so the
        // back thread may run at most one call ahead of the call whose bytes the writer still holds: two credits, one taken
        // before each back call and given back when its bytes have been written.
        BoundedQueue<OutRef> q_write(2);
        BoundedQueue<int> q_credit(2);
        q_credit.push(0);
        q_credit.push(0);
        for (int k = 0; k < NBUF; k++) { q_cfree.push(k); q_free.push(k); }
        std::string stage_err;
        std::mutex err_m;
        auto set_err = [&](const std::string &e) {
            std::lock_guard<std::mutex> l(err_m);
            if (stage_err.empty()) stage_err = e;
        };
        std::atomic<bool> abort_all{false};
        // --extract PATH: the extract file, its writer (made once the device is there) and the writer thread's records
        struct FileCloser { FILE *f = nullptr; ~FileCloser() { if (f) fclose(f); } } xfile;
        std::unique_ptr<Writer> xwriter;
        std::vector<Rec> xrecs;
        IndexSink index;  // --write-index (the back thread adds every call's entries)
        StageThreads stages;
        stages.unblock = [&] {
            abort_all = true;
            q_cfree.close(); q_cfull.close(); q_free.close(); q_full.close(); q_done.close(); q_write.close(); q_credit.close();
        };
        stages.th.emplace_back([&] {  // file reader
            try {
                uint64_t at = coff;
                int k;
                bool eof = false;
                while (!eof && !abort_all && q_cfree.pop(k)) {
                    CBuf &c = cbufs[k];
                    ck_fread.start();
                    c.off = at;
                    c.n = read_fill(fileno(f), c.p + HEAD, ccap, &at, read_end, &eof, path);
                    ck_fread.stop();
                    c.eof = eof;
                    q_cfull.push(k);
                }
            } catch (const std::exception &e) {
                set_err(e.what());
            }
            q_cfull.close();
        });
        stages.th.emplace_back([&] {  // members: cut (and, in host mode, inflated on the pool) into the calls' buffers
            try {
                MemberCutter cutter;
                std::vector<Mem> ms;
                int ck;
                bool ended = false;
                unsigned batch_no = 0;
                while (!ended && !abort_all && q_cfull.pop(ck)) {
                    CBuf &c = cbufs[ck];
                    const uint64_t cb_off = c.off - cutter.tail.size();  // file offset of cb[0]
                    const MemberCutter::Cut cut = cutter.cut(c.p, HEAD, c.n, c.eof, ms, path);
                    uint8_t *const cb = cut.cb;
                    ended = c.eof;
                    if (!host_inflate) {
                        // the compressed bytes go to the device as they lie; the buffer comes back when front is done with it
                        In in;
                        in.p = cb; in.n = cut.w; in.last = ended; in.cbuf = ck;
                        int slot;
                        if (!q_free.pop(slot)) break;
                        bufs[slot] = in;
                        q_full.push(slot);
                        continue;
                    }
                    // host mode: batches of members whose payloads fill a pinned buffer
                    size_t m0 = 0;
                    cbuf_refs[ck] = 1;  // (this thread's own hold on the compressed bytes)
                    do {
                        size_t total = 0;
                        const size_t m1 = take_batch(ms, m0, chunk, &total);
                        int slot;
                        if (!q_free.pop(slot)) { ended = true; break; }
                        In &b = bufs[slot];
                        b.p = b.pin;
                        b.compressed = false;
                        // a call of the device's share: the members as they lie (never the run's last call, whose tail a lane trims here)
                        if (dev_share && m1 > m0 && ++batch_no % (unsigned)dev_share == 0 && !(ended && m1 == ms.size())) {
                            b.p = cb + ms[m0].off;
                            b.n = ms[m1 - 1].off + ms[m1 - 1].size - ms[m0].off;
                            b.last = false;
                            b.compressed = true;
                            b.cbuf = ck;
                            cbuf_refs[ck]++;
                            q_full.push(slot);
                            m0 = m1;
                            continue;
                        }
                        ck_inflate.start();
                        const bool inflated = inflate_batch(pool, cb, ms, m0, m1, b.p);
                        ck_inflate.stop();
                        if (!inflated) throw std::runtime_error("BGZF block does not inflate to its ISIZE / CRC32 (corrupt input)");
                        // a lane's last member: only the bytes in front of the next lane's first record are this lane's
                        if (limited && m1 == ms.size() && m1 > m0 && cb_off + ms[m1 - 1].off == lane.range.coff_end) {
                            if (lane.range.end_rec > ms[m1 - 1].isz) throw std::runtime_error("lane range ends beyond its last block");
                            total -= ms[m1 - 1].isz - (size_t)lane.range.end_rec;
                        }
                        b.n = total;
                        b.last = ended && m1 == ms.size();
                        b.cbuf = -1;
                        q_full.push(slot);
                        m0 = m1;
                    } while (m0 < ms.size());
                    if (--cbuf_refs[ck] == 0) q_cfree.push(ck);  // (inflated: the compressed bytes are done with, unless a call of the device's share still reads them)
                }
            } catch (const std::exception &e) {
                set_err(e.what());
                abort_all = true;
                q_cfree.close();
            }
            q_full.close();
        });
        ck_fasta.start();
        GenomeSource genome;
        if (genome.prepare(o.pos[2], hdr.names, hdr.lens)) return 1;
        ck_fasta.stop();
        Header out_hdr = hdr;
        out_hdr.add_pg("fade-annotate", "fade", FADE_VERSION, lane.on ? lane.cl : cl);  // anno.d:25-32
        ck_upload.start();
        if (ctx_ready.get()) { fprintf(stderr, "[E::fade annotate] cannot open the GPU path: %s\n", create_err.c_str()); return 1; }
        // the buffers the reader has been filling become staging memory now
        if (!staging.pin(ctx)) { fprintf(stderr, "[E::fade annotate] %s\n", fadehip_last_error(ctx)); return 1; }
        if (genome.upload(ctx)) return 1;
        if (o.timing) genome.report();
        // the header goes out through the CPU writer (its members only: no end-of-file block yet; not a byte without a device)
        if (o.sort) {
            // (--sort: nothing reaches stdout while the input streams through; header, records and marker follow the sort)
        } else if (!o.write_index.empty()) {
            index.open(o.write_index, hdr.names.size());
            index.header([&](FILE *to) {
                Writer hw(to, o.ubam ? OutFmt::UBAM : OutFmt::BAM, out_hdr, &pool, nullptr, true, false);
                hw.close();
            });
        } else {
            Writer hw(stdout, o.ubam ? OutFmt::UBAM : OutFmt::BAM, out_hdr, &pool, nullptr, !lane.on || lane.k == 0 || lane.shard, false);
            hw.close();
        }
        if (creating.get()) { fprintf(stderr, "[E::fade annotate] cannot open the GPU path: %s\n", create_err.c_str()); return 1; }
        if (!o.extract.empty()) {  // --extract PATH: the output's format and header, written by the CPU writer
            xfile.f = fopen(o.extract.c_str(), "wb");
            if (!xfile.f) { fprintf(stderr, "[E::fade annotate] cannot write %s: %s\n", o.extract.c_str(), strerror(errno)); return 1; }
            if (!store) xwriter.reset(new Writer(xfile.f, o.ubam ? OutFmt::UBAM : OutFmt::BAM, out_hdr, &pool));  // (--extract-sorted: written once the main output is finished)
        }
        ck_upload.stop();
        // (the FASTA's text is on the device now; giving a genome's worth of pages back takes milliseconds, and the first call
        // is waiting: on a thread of its own)
        std::thread([seqs = std::move(genome.fa.seqs)]() mutable { seqs.clear(); seqs.shrink_to_fit(); }).detach();
        stages.th.emplace_back([&] {  // back: compress, hand to the writer
            int tok;
            try {
                while (q_done.pop(tok)) {
                    const uint8_t *p = nullptr;
                    size_t n = 0;
                    int credit;
                    if (!q_credit.pop(credit)) break;  // (the run is being given up)
                    ck_back.start();
                    const int rc = fadehip_bam_back(st, &p, &n);
                    ck_back.stop();
                    if (rc) throw std::runtime_error(std::string("device: ") + fadehip_last_error(ctx));
                    note_held(o, st);
                    if (index.on()) index.call(st, ctx, n);  // (the entries live as long as the call's members: taken here)
                    OutRef ref{p, n};
                    if (xwriter) {  // (the call's extract records live as long as its members: the writer takes both)
                        int64_t n_x = 0;
                        if (fadehip_bam_back_extract(st, &ref.xp, &ref.xn, &n_x)) throw std::runtime_error(std::string("device: ") + fadehip_last_error(ctx));
                    }
                    q_write.push(ref);
                }
            } catch (const std::exception &e) {
                set_err(e.what());
                abort_all = true;
                while (q_done.pop(tok)) {}
            }
            q_write.close();
        });
        // The writer.  Into a file that can be written at an offset (a regular file, not opened for appending) a call's members
        // go out as a few pwrites side by side — one thread copies into the page cache at 8-10 GB/s, and 1.6 GB per 10 M reads
        // is then a stage as long as the device's; into a pipe they go out through stdout in order.  `placed_base` is where the
        // records start (the header has been flushed by then); the file offset is set behind the last byte at the end.
        std::atomic<long long> placed_base{-1};
        std::atomic<uint64_t> placed_bytes{0};
        // (FADE_BAM_WRITERS=n: off by default — measured on the GPU box, four pwrites side by side into one file took 0.21-0.23 s
        // per 1.6 GB against 0.18 s front to back: buffered writes to one inode serialise in the kernel)
        const int n_wr = std::max(1, std::min(8, getenv("FADE_BAM_WRITERS") ? atoi(getenv("FADE_BAM_WRITERS")) : 1));
        stages.th.emplace_back([&] {  // writer
            OutRef r;
            bool ok = true;
            uint64_t at = 0;
            std::vector<std::thread> helpers;
            while (q_write.pop(r)) {
                if (ok && r.xn) {
                    // the call's extract records (a few per cent of its bytes): framed here, compressed by the extract file's
                    // own writer on the pool — on this side of the pipeline, so that the front half never waits for it
                    try {
                        split_extract_records(r.xp, r.xn, xrecs);
                        xwriter->write(xrecs);
                    } catch (const std::exception &e) { set_err(e.what()); ok = false; abort_all = true; }
                }
                if (ok && r.n) {
                    ck_fwrite.start();
                    const long long base = placed_base.load();
                    if (base < 0) {
                        if (fwrite(r.p, 1, r.n, stdout) != r.n) { set_err("write error on the output stream"); ok = false; abort_all = true; }
                    } else {
                        std::atomic<bool> bad{false};
                        auto put = [&](size_t lo, size_t hi) {
                            while (lo < hi) {
                                const ssize_t w = pwrite(1, r.p + lo, hi - lo, (off_t)((uint64_t)base + at + lo));
                                if (w < 0 && errno == EINTR) continue;
                                if (w <= 0) { bad = true; return; }
                                lo += (size_t)w;
                            }
                        };
                        const size_t parts = r.n >= ((size_t)1 << 20) ? (size_t)n_wr : 1;
                        helpers.clear();
                        for (size_t q = 1; q < parts; q++) helpers.emplace_back(put, r.n * q / parts, r.n * (q + 1) / parts);
                        put(0, r.n / parts);
                        for (auto &h : helpers) h.join();
                        if (bad) { set_err("write error on the output stream"); ok = false; abort_all = true; }
                        at += r.n;
                        placed_bytes = at;
                    }
                    ck_fwrite.stop();
                }
                q_credit.push(0);
            }
        });
        {
            struct stat so;
            const int fl = fcntl(1, F_GETFL);
            if (fflush(stdout) == 0 && fstat(1, &so) == 0 && S_ISREG(so.st_mode) && fl >= 0 && !(fl & O_APPEND) &&
                getenv("FADE_BAM_WRITERS") && atoi(getenv("FADE_BAM_WRITERS")) > 1) {
                const off_t b = lseek(1, 0, SEEK_CUR);
                if (b >= 0) placed_base = (long long)b;
            }
        }
        int k;
        bool failed = false;
        while (!failed && !abort_all && q_full.pop(k)) {
            ck_front.start();
            const int rc = (host_inflate && !bufs[k].compressed) ? fadehip_bam_front_raw(st, bufs[k].p, bufs[k].n, bufs[k].last ? 1 : 0)
                                                                 : fadehip_bam_front(st, bufs[k].p, bufs[k].n, bufs[k].last ? 1 : 0);
            ck_front.stop();
            if (rc) { set_err(std::string("device: ") + fadehip_last_error(ctx)); failed = true; break; }
            if (bufs[k].cbuf >= 0) {  // (the compressed bytes have been copied up)
                if (!host_inflate) q_cfree.push(bufs[k].cbuf);
                else if (--cbuf_refs[bufs[k].cbuf] == 0) q_cfree.push(bufs[k].cbuf);
            }
            q_free.push(k);
            q_done.push(0);
        }
        q_done.close();
        // a stage gave up (a write error, a back call that failed) or front did: the stages in front of this loop may sit in
        // q_free / q_cfree, which nobody serves any more — closed here, BEFORE the join, so that they see the end
        if (failed || abort_all) { abort_all = true; q_free.close(); q_cfree.close(); while (q_full.pop(k)) {} }
        for (auto &t : stages.th) t.join();
        stages.unblock = nullptr;
        if (!stage_err.empty()) { fprintf(stderr, "[E::fade annotate] %s\n", stage_err.c_str()); return 1; }
        if (xwriter) {
            xwriter->close();
            xwriter.reset();
            if (fflush(xfile.f) != 0 || ferror(xfile.f)) { fprintf(stderr, "[E::fade annotate] write error on %s\n", o.extract.c_str()); return 1; }
        }
        if (placed_base.load() >= 0 && lseek(1, (off_t)((uint64_t)placed_base.load() + placed_bytes.load()), SEEK_SET) < 0) {
            fprintf(stderr, "[E::fade annotate] cannot seek the output: %s\n", strerror(errno));
            return 1;
        }
        if (o.sort) {  // one window only: re-aligning the input once per window is not built
            int32_t over = 0;
            int64_t n_reset = 0;
            uint64_t budget = 0;
            if (fadehip_recstore_over(store, &over) || fadehip_recstore_resets(store, &n_reset) || fadehip_recstore_budget(store, &budget)) throw std::runtime_error(fadehip_last_error(ctx));
            if (over) {
                fprintf(stderr, "[E::fade-annotate] --sort: the output's records do not fit the budget of %llu bytes on the device, and annotate sorts in one piece: annotate without --sort and "
                                "sort in the fade out step (fade out --gpus 1 --sort), which takes files of any size\n", (unsigned long long)budget);
                return 1;
            }
            if (n_reset && !o.write_index.empty()) {
                fprintf(stderr, "[E::fade-annotate] --sort --write-index: %lld reads are clipped to nothing; they are written zero-filled (refID 0, pos 0) at the end of the file, and a file that "
                                "ends in them is not in coordinate order by its own bytes, so no index can be made of it (samtools index refuses it too): run without --write-index\n", (long long)n_reset);
                return 1;
            }
            StageClock ck_sorted;
            ck_sorted.start();
            const int64_t n_sorted = write_sorted_store(ctx, store, stdout, o.ubam, out_hdr, &pool, o.write_index);
            ck_sorted.stop();
            if (o.timing) fprintf(stderr, "[timing] --sort: %lld records sorted on the device and written in coordinate order in %.3f s\n", (long long)n_sorted, ck_sorted.t);
        } else if ((!lane.on || lane.shard) && fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, stdout) != sizeof BGZF_EOF) { fprintf(stderr, "[E::fade annotate] write error on the output stream\n"); return 1; }
        if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "[E::fade annotate] write error on the output stream\n"); return 1; }
        if (index.on()) index.write();
        if (store && !o.sort) {  // --extract-sorted: PATH in coordinate order and PATH.bai beside it, behind the finished main output
            StageClock ck_sorted;
            ck_sorted.start();
            const int64_t n_sorted = write_sorted_store(ctx, store, xfile.f, o.ubam, out_hdr, &pool, o.extract + (o.csi ? ".csi" : ".bai"));
            ck_sorted.stop();
            if (o.timing) fprintf(stderr, "[timing] --extract-sorted: %lld records sorted on the device and written in coordinate order in %.3f s\n", (long long)n_sorted, ck_sorted.t);
        }
        int64_t totals[8], n_rec = 0, n_over = 0;
        fadehip_bam_totals(st, totals, &n_rec, &n_over);
        report_held(o);
        if (lane.on) {
            // the lane's report for the parent; lanes on distinct devices first sum their counters among themselves (the one
            // collective of the path: ncclAllReduce over xGMI, one rank per process)
            long long red[8];
            bool have_red = false;
            if (lane.rccl && lane.n > 1) {
                int64_t t[8];
                std::copy(totals, totals + 8, t);
                if (fadehip_stats_allreduce_rank(ctx, lane.k, lane.n, lane.id_path.c_str(), t, 8)) { fprintf(stderr, "[E::fade annotate] stats all-reduce (lanes): %s\n", fadehip_last_error(ctx)); return 1; }
                for (int q = 0; q < 8; q++) red[q] = (long long)t[q];
                have_red = true;
            }
            FILE *sf = fopen(lane.status_path.c_str(), "w");
            if (!sf) { fprintf(stderr, "[E::fade annotate] cannot write %s\n", lane.status_path.c_str()); return 1; }
            for (int q = 0; q < 8; q++) fprintf(sf, "%lld ", (long long)totals[q]);
            fprintf(sf, "%lld\n", (long long)n_over);
            if (have_red) {
                for (int q = 0; q < 8; q++) fprintf(sf, "%lld ", red[q]);
                fprintf(sf, "\n");
            }
            fclose(sf);
        }
        if (n_over && !lane.on) fprintf(stderr, "[W::fade annotate] %lld soft-clipped reads were not re-aligned: read longer than %d bases or window longer than %d\n",
                            (long long)n_over, FADEHIP_MAX_LONG_QUERY, prm.max_ref_len);
        if (o.stats && !lane.on) {  // stats.d:56-72 layout
            const double rc = (double)std::max<int64_t>(totals[0], 1);
            fprintf(stderr, "read count:\t%lld\nClipped %%:\t%g\n%% With Supplementary alns:\t%g\nArtifact rate:\t%g\n"
                            "%% With Supplementary alns and artifacts:\t%g\nArtifact rate left only:\t%g\nArtifact rate right only:\t%g\n",
                    (long long)totals[0], totals[1] / rc, totals[2] / rc, totals[4] / rc, totals[3] / rc, totals[6] / rc, totals[7] / rc);
        }
        ck_total.stop();
        if (o.timing) {
            fprintf(stderr, "[timing] total %.3f s: fasta %.3f, create+genome upload %.3f | reader: file reads %.3f, inflate on %d host threads %.3f | front (%sframe, annotate, tags) %.3f | "
                            "back (deflate, copy out) %.3f | fwrite %.3f (stages overlap); %lld records\n",
                    ck_total.t, ck_fasta.t, ck_upload.t, ck_fread.t, host_inflate ? pool.size() : 0, ck_inflate.t, host_inflate ? "" : "inflate, ", ck_front.t, ck_back.t, ck_fwrite.t, (long long)n_rec);
        }
        g_trace.dump();
        if (getenv("FADEHIP_BAM_PROF")) { fadehip_bam_close(st); st = nullptr; }  // (prints the library's own clocks)
        if (!(getenv("FADE_FAST_EXIT") && atoi(getenv("FADE_FAST_EXIT")) == 0)) {
            if (o.timing) fprintf(stderr, "[timing] since process start %.3f s (leaving by _exit)\n", since_process_start());
            fflush(stdout);
            fflush(stderr);
            _exit(0);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "[E::fade annotate] %s\n", e.what());
        return 1;
    }
    return 0;
}

static int annotate_main(const std::string &cl, const Opts &o) {
    StageClock ck_total, ck_fasta, ck_upload, ck_read, ck_pack, ck_submit, ck_collect, ck_tags, ck_write;
    ck_total.start();
    if (o.timing) fprintf(stderr, "[timing] since process start %.3f s (annotate begins)\n", since_process_start());
    if (o.timing) fprintf(stderr, "[timing] %d threads%s\n", o.threads > 0 ? o.threads : default_threads(), o.threads > 0 ? "" : " (default: affinity and cgroup quota)");
    const LaneEnv lane = lane_env();  // set when this process is one lane of a `--gpus N` run (annotate_lanes_main)
    // anno.d:18-19 (htslib log format)
    if (!lane.on) fprintf(stderr, "[W::fade annotate] Output SAM/BAM will not be sorted (regardless of prior sorting)\n");
    const int nthreads = o.threads > 0 ? o.threads : default_threads();
    const int ngpu = lane.on ? 1 : std::max(1, o.gpus);
    std::vector<fadehip_ctx *> ctxs((size_t)ngpu, nullptr);
    std::vector<BlockPool> blocks((size_t)ngpu);
    struct CtxGuard {
        std::vector<fadehip_ctx *> &c;
        std::vector<BlockPool> &b;
        ~CtxGuard() {
            for (size_t k = 0; k < c.size(); k++) {
                if (c[k]) b[k].drain();
                fadehip_destroy(c[k]);
            }
        }
    } ctx_guard{ctxs, blocks};
    Pool pool(nthreads);
    try {
        Reports reports;  // --stats-tsv / --clip-tsv: filled by the writer stage, chunk after chunk
        reports.open(o);
        Reader reader(o.pos[1], &pool);   // anno.d:22 (every stage's parallel work runs on the one pool)
        if (lane.on) reader.restrict_to(lane.range);  // this lane's records only
        // (the reader starts at once: the first batches inflate while the FASTA loads and the genome goes to HBM)
        // Stages: [reader: BGZF inflate / SAM parse] -> [this thread: pack into a pinned block, upload + run (both return
        // at once), fetch the oldest batch's results] -> [writer: tags, format, BGZF deflate].  Each stage has its own
        // pool; chunks keep their input order.  The device calls are asynchronous, so this one thread keeps every slot
        // of every device busy: batch k goes to device k % N, the device's slots in turn.
        // the reader may run ahead by about two million records (0.6 GB inflated) while the GPU path comes up
        const size_t ahead = (size_t)std::max(2, std::min(8, (2 << 20) / std::max(o.batch, 1)));
        BoundedQueue<std::unique_ptr<Chunk>> q_in(ahead), q_out(3);
        std::string stage_err;
        std::mutex err_m;
        auto set_stage_err = [&](const std::string &e) {
            std::lock_guard<std::mutex> l(err_m);
            if (stage_err.empty()) stage_err = e;
        };
        std::atomic<bool> abort_stages{false};
        StageThreads stages;
        stages.unblock = [&] {
            abort_stages = true;
            q_in.close();
            q_out.close();
        };
        stages.th.emplace_back([&] {
            try {
                while (!abort_stages) {
                    std::unique_ptr<Chunk> c(new Chunk());
                    ck_read.start();
                    const size_t got = reader.read_block(c->blk, (size_t)std::max(o.batch, 1));  // (SAM lines are parsed into the same layout)
                    ck_read.stop();
                    if (got == 0) break;
                    q_in.push(std::move(c));
                }
            } catch (const std::exception &e) {
                set_stage_err(e.what());
            }
            q_in.close();
        });
        // --gpus N uses devices 0..N-1; FADE_DEVICE_MAP="0,0" (tests on a one-GPU box) maps the N contexts elsewhere
        std::vector<int> devmap((size_t)ngpu);
        for (int d = 0; d < ngpu; d++) devmap[(size_t)d] = d;
        bool distinct_devices = true;
        if (lane.on) devmap[0] = lane.device;
        else if (const char *dm = getenv("FADE_DEVICE_MAP")) {
            int d = 0;
            for (const char *q = dm; *q && d < ngpu; d++) {
                devmap[(size_t)d] = atoi(q);
                q = strchr(q, ',');
                if (!q) break;
                q++;
            }
            for (int a = 0; a < ngpu; a++)
                for (int b2 = a + 1; b2 < ngpu; b2++)
                    if (devmap[(size_t)a] == devmap[(size_t)b2]) distinct_devices = false;
        }
        fadehip_params prm;
        fadehip_params_default(&prm);  // max_ref_len 2^20: any window the kernels can serve, whatever -w is
        prm.max_batch_reads = std::max(o.batch, 1);
        // Batches in flight per device.  A device annotates a batch in about a millisecond and the host needs thirty for
        // it, so one slot is enough here, and with one batch at a time nothing competes with the score pass for CUs: the
        // run then needs three HSA queues fewer (a slot's two streams and the CU-masked one; each is a 173 MB context-save
        // area to set up and to give back: ~80 ms per run in all).  FADE_SLOTS=2 restores the double-buffered form.
        // If the host ever waits for the device (more than 15 % of the time since the first batch went out), the second slot
        // is taken into use for the rest of the run: upload and run of a batch then overlap the one before.
        const bool slots_fixed = getenv("FADE_SLOTS") != nullptr;
        const double wait_frac = getenv("FADE_SLOT_WAIT") ? atof(getenv("FADE_SLOT_WAIT")) : 0.15;  // (tests: 0 forces the switch)
        if (const char *sl = getenv("FADE_SLOTS")) kSlotsInUse = (size_t)std::max(1, std::min(atoi(sl), FADEHIP_NUM_SLOTS));
        if (kSlotsInUse == 1) setenv("FADEHIP_TAIL_CUS", "0", 0);
        // the HIP runtime and the contexts come up on a helper thread while this one reads the FASTA
        std::string create_err;
        std::future<int> creating = std::async(std::launch::async, [&]() -> int {
            for (int d = 0; d < ngpu; d++)
                if (fadehip_create(&ctxs[(size_t)d], devmap[(size_t)d], &prm)) {
                    create_err = fadehip_last_error(nullptr);  // (the library keeps it per thread)
                    return 1;
                }
            return 0;
        });
        ck_fasta.start();
        GenomeSource genome;
        if (genome.prepare(o.pos[2], reader.header().names, reader.header().lens)) return 1;
        ck_fasta.stop();
        Header hdr = reader.header();     // anno.d:24
        hdr.add_pg("fade-annotate", "fade", FADE_VERSION, lane.on ? lane.cl : cl);  // anno.d:25-32

        const Header &h = reader.header();
        if (h.names.empty()) {
            fprintf(stderr, "[E::fade annotate] input has no @SQ lines\n");
            return 1;
        }
        auto die = [&](fadehip_ctx *c, const char *what) {
            fprintf(stderr, "[E::fade annotate] %s: %s\n", what, fadehip_last_error(c));
            return 1;
        };
        ck_upload.start();
        if (creating.get()) {
            fprintf(stderr, "[E::fade annotate] cannot open the GPU path: %s\n", create_err.c_str());
            return 1;
        }
        for (int d = 0; d < ngpu; d++) {
            blocks[(size_t)d].ctx = ctxs[(size_t)d];
            if (genome.upload(ctxs[(size_t)d])) return 1;
        }
        ck_upload.stop();
        if (o.timing) genome.report();
        genome.fa.seqs.clear();
        genome.fa.seqs.shrink_to_fit();
        // nothing is written to stdout before the GPU path is known to be usable
        const OutFmt fmt = o.bam ? OutFmt::BAM : o.ubam ? OutFmt::UBAM : OutFmt::SAM;  // util.d:65-76
        // BAM output: the BGZF blocks are compressed on the device (FADE_BGZF_DEVICE=0 keeps them on the host pool)
        std::unique_ptr<DeviceBgzf> dev_codec;
        if (fmt == OutFmt::BAM && !(getenv("FADE_BGZF_DEVICE") && atoi(getenv("FADE_BGZF_DEVICE")) == 0)) dev_codec.reset(new DeviceBgzf(ctxs[0]));
        Writer writer(stdout, fmt, hdr, &pool, dev_codec.get(), !lane.on || lane.k == 0 || lane.shard, !lane.on || lane.shard);
        // --extract PATH: the extract records in the output's format, under the output's header (compressed on the host pool)
        struct FileCloser { FILE *f = nullptr; ~FileCloser() { if (f) fclose(f); } } xfile;
        std::unique_ptr<Writer> xwriter;
        std::vector<Rec> xrecs;
        if (!o.extract.empty()) {
            xfile.f = fopen(o.extract.c_str(), "wb");
            if (!xfile.f) { fprintf(stderr, "[E::fade annotate] cannot write %s: %s\n", o.extract.c_str(), strerror(errno)); return 1; }
            xwriter.reset(new Writer(xfile.f, fmt, hdr, &pool));
        }

        Ejector ejector;  // --eject: the writer stage's
        std::vector<Rec> kept;
        StageThreads wstage;  // declared after the writer it uses: joined before the writer goes away
        wstage.unblock = [&] {
            abort_stages = true;
            q_in.close();
            q_out.close();
        };
        wstage.th.emplace_back([&] {
            std::unique_ptr<Chunk> c;
            try {
                while (q_out.pop(c)) {
                    ck_tags.start();
                    apply_tags(*c, hdr, pool, o.clip, xwriter ? &xrecs : nullptr);
                    if (reports.on()) reports.add(*c, hdr, ctxs[(size_t)c->dev]);
                    ck_tags.stop();
                    ck_write.start();
                    if (xwriter && !xrecs.empty()) xwriter->write(xrecs);
                    if (o.eject) {
                        // the chunk's records with their tags on, then filter.d:221-265 by the batch's rs
                        const size_t n = c->n_records();
                        std::vector<uint8_t> art(n, 0);
                        for (size_t k = 0; k < c->sent.size(); k++) art[c->sent[k]] = (c->rs_sent[k] & 6) != 0;
                        std::vector<int32_t> own(n, -1);
                        for (size_t k = 0; k < c->bout.owned.size(); k++) own[c->bout.owned[k].first] = (int32_t)k;
                        kept.clear();
                        for (size_t i = 0; i < n; i++) {
                            Rec r;
                            if (own[i] >= 0) r = std::move(c->bout.owned[(size_t)own[i]].second);
                            else {
                                const uint8_t *b = c->blk.buf.data() + c->blk.off[i], *sx = c->bout.sfx.data() + c->bout.sfx_off[i];
                                r.d.assign(b, b + c->blk.len[i]);
                                r.d.insert(r.d.end(), sx, sx + (c->bout.sfx_off[i + 1] - c->bout.sfx_off[i]));
                            }
                            ejector.add(std::move(r), art[i] != 0, kept);
                        }
                        writer.write(kept);
                    } else writer.write_block(c->blk, c->bout);
                    ck_write.stop();
                }
                if (o.eject) {  // the group still open, or an input of fewer than ten records
                    kept.clear();
                    ejector.finish(kept);
                    writer.write(kept);
                }
            } catch (const std::exception &e) {
                set_stage_err(e.what());
                while (q_out.pop(c)) {}
            }
        });
        std::deque<std::unique_ptr<Chunk>> inflight;
        int64_t totals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<std::vector<int64_t>> per_dev((size_t)ngpu, std::vector<int64_t>(8, 0));
        int64_t n_oversize = 0;
        bool failed = false;
        auto finish = [&](std::unique_ptr<Chunk> c) -> int {
            fadehip_anno_view v;
            ck_collect.start();
            const int crc = fadehip_annotate_results(ctxs[(size_t)c->dev], c->slot, &v);
            if (!crc) {
                // the slot's result block is reused by its next batch: keep what the writer stage needs
                c->rs_sent.assign(v.rs, v.rs + v.n_reads);
                c->art.clear();
                for (int k = 0; k < v.n_aln; k++)
                    if (v.aln[k].art) c->art.push_back(v.aln[k]);
                for (int k = 0; k < 8; k++) per_dev[(size_t)c->dev][(size_t)k] += v.stats[k];
                n_oversize += v.n_oversize;
            }
            ck_collect.stop();
            blocks[(size_t)c->dev].release(c->block, c->block_cap);
            c->block = nullptr;
            if (crc) {
                fprintf(stderr, "[E::fade annotate] results: %s\n", fadehip_last_error(ctxs[(size_t)c->dev]));
                return 1;
            }
            q_out.push(std::move(c));
            return 0;
        };
        size_t seq_no = 0;
        std::vector<int> next_slot((size_t)ngpu, 0);
        std::chrono::steady_clock::time_point t_first;
        std::unique_ptr<Chunk> c;
        // a failed stage (reader or writer) ends the run here: no further batch is packed or sent to a device
        auto stage_failed = [&] {
            std::lock_guard<std::mutex> l(err_m);
            return !stage_err.empty();
        };
        while (!failed && !stage_failed() && q_in.pop(c)) {
            c->dev = (int)(seq_no % (size_t)ngpu);
            c->slot = next_slot[(size_t)c->dev];
            next_slot[(size_t)c->dev] = (c->slot + 1) % (int)kSlotsInUse;
            if (seq_no == 0) t_first = std::chrono::steady_clock::now();
            seq_no++;
            ck_pack.start();
            pack_chunk(*c, pool, blocks[(size_t)c->dev]);  // (while the device works on the batch before)
            ck_pack.stop();
            // one batch per (device, slot): the batch that had this slot is fetched before the slot is handed the next
            while (!failed && inflight.size() >= (size_t)ngpu * kSlotsInUse) {
                if (finish(std::move(inflight.front()))) failed = true;
                inflight.pop_front();
            }
            if (failed) {
                blocks[(size_t)c->dev].release(c->block, c->block_cap);  // (the chunk in hand goes nowhere: its pinned block returns to the pool)
                c->block = nullptr;
                break;
            }
            ck_submit.start();
            const int src = fadehip_annotate_submit(ctxs[(size_t)c->dev], c->slot, &c->b, o.floor_len, o.window);
            ck_submit.stop();
            if (src) {
                fprintf(stderr, "[E::fade annotate] submit: %s\n", fadehip_last_error(ctxs[(size_t)c->dev]));
                blocks[(size_t)c->dev].release(c->block, c->block_cap);
                c->block = nullptr;
                failed = true;
                break;
            }
            inflight.push_back(std::move(c));
            if (!slots_fixed && kSlotsInUse == 1 && seq_no >= 4 * (size_t)ngpu &&
                ck_collect.t > wait_frac * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_first).count()) {
                kSlotsInUse = 2;  // the batches in flight keep slot 0; the next one of every device takes slot 1
                std::fill(next_slot.begin(), next_slot.end(), 1);
                if (o.timing) fprintf(stderr, "[timing] the host waited for the device: two batches in flight per device from batch %zu on\n", seq_no);
            }
        }
        while (!failed && !inflight.empty()) {
            if (finish(std::move(inflight.front()))) failed = true;
            inflight.pop_front();
        }
        if (stage_failed()) failed = true;
        if (failed) {  // the batches still in flight are abandoned (their pinned blocks go back), the reader runs out so that it can exit
            for (auto &f : inflight)
                if (f && f->block) {
                    (void)fadehip_sync(ctxs[(size_t)f->dev]);  // the DMA out of the block has ended before it is reused or freed
                    blocks[(size_t)f->dev].release(f->block, f->block_cap);
                    f->block = nullptr;
                }
            inflight.clear();
            abort_stages = true;
            while (q_in.pop(c)) {}
        }
        q_out.close();
        for (auto &t : wstage.th) t.join();
        for (auto &t : stages.th) t.join();
        wstage.unblock = nullptr;
        stages.unblock = nullptr;
        if (!stage_err.empty()) {
            fprintf(stderr, "[E::fade annotate] %s\n", stage_err.c_str());
            failed = true;
        }
        if (failed) return 1;
        writer.close();
        if (xwriter) {
            xwriter->close();
            xwriter.reset();
            if (fflush(xfile.f) != 0 || ferror(xfile.f)) { fprintf(stderr, "[E::fade annotate] write error on %s\n", o.extract.c_str()); return 1; }
        }
        reports.close();
        if (n_oversize && !lane.on)
            fprintf(stderr, "[W::fade annotate] %lld soft-clipped reads were not re-aligned: read longer than %d bases or window longer than %d\n",
                    (long long)n_oversize, FADEHIP_MAX_LONG_QUERY, prm.max_ref_len);
        // the one collective of the path: sum the stats.d counters over the devices (RCCL over xGMI)
        if (ngpu > 1 && distinct_devices) {
            std::vector<int64_t> flat((size_t)ngpu * 8);
            for (int d = 0; d < ngpu; d++) std::copy(per_dev[(size_t)d].begin(), per_dev[(size_t)d].end(), flat.begin() + d * 8);
            if (fadehip_stats_allreduce(ctxs.data(), ngpu, flat.data(), 8)) return die(ctxs[0], "stats all-reduce");
            std::copy(flat.begin(), flat.begin() + 8, totals);
        } else {
            // (several contexts mapped onto one device by FADE_DEVICE_MAP: RCCL takes one rank per device, sum here)
            for (int d = 0; d < ngpu; d++)
                for (int k = 0; k < 8; k++) totals[k] += per_dev[(size_t)d][(size_t)k];
        }
        if (lane.on) {
            // the lane's report for the parent; lanes on distinct devices first sum their counters among themselves, the one
            // collective of the path: ncclAllReduce over xGMI, one rank per process
            long long red[8];
            bool have_red = false;
            if (lane.rccl && lane.n > 1) {
                int64_t t[8];
                std::copy(totals, totals + 8, t);
                if (fadehip_stats_allreduce_rank(ctxs[0], lane.k, lane.n, lane.id_path.c_str(), t, 8)) return die(ctxs[0], "stats all-reduce (lanes)");
                for (int q = 0; q < 8; q++) red[q] = (long long)t[q];
                have_red = true;
            }
            FILE *sf = fopen(lane.status_path.c_str(), "w");
            if (!sf) { fprintf(stderr, "[E::fade annotate] cannot write %s\n", lane.status_path.c_str()); return 1; }
            for (int q = 0; q < 8; q++) fprintf(sf, "%lld ", (long long)totals[q]);
            fprintf(sf, "%lld\n", (long long)n_oversize);
            if (have_red) {
                for (int q = 0; q < 8; q++) fprintf(sf, "%lld ", red[q]);
                fprintf(sf, "\n");
            }
            fclose(sf);
        }
        if (o.stats && !lane.on) {  // stats.d:56-72 layout
            const double rc = (double)std::max<int64_t>(totals[0], 1);
            fprintf(stderr, "read count:\t%lld\nClipped %%:\t%g\n%% With Supplementary alns:\t%g\nArtifact rate:\t%g\n"
                            "%% With Supplementary alns and artifacts:\t%g\nArtifact rate left only:\t%g\nArtifact rate right only:\t%g\n",
                    (long long)totals[0], totals[1] / rc, totals[2] / rc, totals[4] / rc, totals[3] / rc, totals[6] / rc, totals[7] / rc);
        }
        ck_total.stop();
        if (o.timing)
            fprintf(stderr, "[timing] total %.3f s: fasta %.3f, create+genome upload %.3f | reader stage %.3f | pack %.3f, "
                            "submit %.3f, results %.3f | writer stage: tags %.3f, write %.3f (stages overlap)\n",
                    ck_total.t, ck_fasta.t, ck_upload.t, ck_read.t, ck_pack.t, ck_submit.t, ck_collect.t, ck_tags.t, ck_write.t);
        if (o.timing) {  // core-seconds of the pools' work by kind (thread CPU time)
            std::string line = "[timing] pool core-seconds:";
            double sum = 0;
            for (int k = 0; k < CPU_KINDS; k++) {
                const double sec = (double)cpu_meter()[k].load() * 1e-9;
                if (sec < 0.0005) continue;
                char buf[64];
                snprintf(buf, sizeof buf, " %s %.3f,", cpu_kind_name(k), sec);
                line += buf;
                sum += sec;
            }
            fprintf(stderr, "%s total %.3f\n", line.c_str(), sum);
            fprintf(stderr, "[timing] output thread: %.3f s inside fwrite\n", writer.io_seconds());
            const ReadProf &rp = read_prof();
            if (reader.is_bam())
                fprintf(stderr, "[timing] BAM reader thread: wait for file bytes %.3f, scan %.3f, inflate (parallel) %.3f, frame %.3f, carry %.3f, "
                                "layout check (parallel) %.3f\n", rp.wait_io, rp.scan, rp.inflate, rp.frame, rp.carry, rp.layout);
        }
        // Everything is written and flushed.  What is left would be giving back, piece by piece, what the process exit gives
        // back at once — the contexts' device buffers and streams, a gigabyte of pinned blocks, the pools' threads: 0.1 s of
        // a 0.8 s run.  FADE_FAST_EXIT=0 takes the long way (leak checkers, tests of the destructors).
        if (!(getenv("FADE_FAST_EXIT") && atoi(getenv("FADE_FAST_EXIT")) == 0)) {
            if (o.timing) fprintf(stderr, "[timing] since process start %.3f s (leaving by _exit)\n", since_process_start());
            fflush(stdout);
            fflush(stderr);
            _exit(0);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "[E::fade annotate] %s\n", e.what());
        return 1;
    }
    return 0;
}

// std.getopt rejects an option the subcommand did not declare (app.d:76-83,104-107,132-134)
static bool options_allowed(const Opts &o, const char *allowed) {
    for (char c : o.seen)
        if (!strchr(allowed, c)) {
            if (c == 'R') fprintf(stderr, "std.getopt.GetOptException: Unrecognized option --repeats\n[E::fade] --repeats: the option goes with fade stats --gpus 1 (it adds two columns to that report's rows)\n");
            else if (c == 'Z') fprintf(stderr, "std.getopt.GetOptException: Unrecognized option --sort\n[E::fade] --sort: the option goes with fade out --gpus 1 and fade annotate (the output's records are sorted on the device)\n");
            else if (c == 'N') fprintf(stderr, "std.getopt.GetOptException: Unrecognized option --calmd\n[E::fade] --calmd: the option goes with fade out -c --gpus 1 (NM and MD of the clipped reads follow the clip)\n");
            else if (c == 'J') fprintf(stderr, "std.getopt.GetOptException: Unrecognized option --csi\n[E::fade] --csi: the option goes with --write-index PATH (fade annotate, fade out, fade extract --sorted) and fade annotate --extract-sorted (the index is written as a CSI)\n");
            else fprintf(stderr, "std.getopt.GetOptException: Unrecognized option %s%c\n", "-", c);
            return false;
        }
    return true;
}

static void print_extract_help() {
    fprintf(stderr,
            "%s\nextract: extracts artifacts into a mapped SAM/BAM (used after annotate)\n"
            "usage: fade extract [options] <annotated BAM/SAM> \n\n"
            "-t --threads extra threads for parsing the bam file\n"
            "-b     --bam output bam\n"
            "-u    --ubam output uncompressed bam\n"
            "      --gpus 1: BAM file in, -b or -u out: the records are built on one MI355X (rs and am read back by a kernel)\n"
            "    --sorted with --gpus 1: the records are kept on the MI355X, sorted once by coordinate and written in that order (@HD SO:coordinate)\n"
            "--write-index PATH: with --sorted, also write the BAM index (.bai) of the output, made in the same pass\n"
            "--csi with --write-index: the index is a CSI (min_shift 14, depth 5, or 6 for contigs longer than 2^29), not a BAI\n"
            "    --timing print where the run spent its time to stderr\n"
            "-h    --help This help information.\n\n",
            kHeader);
}

static void print_report_help(bool stats) {
    fprintf(stderr,
            "%s\n%s\n"
            "usage: fade %s --gpus 1 [options] <annotated BAM> [out.tsv]\n\n"
            "-t --threads extra threads for parsing the bam file\n"
            "      --gpus 1: the report's rows are written on one MI355X (the tags read back, the inverted repeats aligned, the text formatted by kernels)\n"
            "%s"
            "    --timing print where the run spent its time to stderr\n"
            "-h    --help This help information.\n\n",
            kHeader, stats ? "stats: reports extended information about artifact reads (used after annotate)" : "stats-clip: reports extended information about all soft-clipped reads (used after annotate)",
            stats ? "stats" : "stats-clip",
            stats ? "   --repeats PATH: a BED file of repeats (plain text), held on the MI355X: every row gains read_rpm and art_rpm, 1 where the read's / the artifact's region overlaps one\n" : "");
}

static bool parse_cigar_string(const std::string &s, std::vector<uint32_t> &ops) {
    uint64_t num = 0;
    bool have = false;
    for (char c : s) {
        if (c >= '0' && c <= '9') { num = num * 10 + (uint64_t)(c - '0'); have = true; }
        else {
            const char *o = strchr(CIGAR_STR, c);
            if (!o || !have) return false;
            ops.push_back((uint32_t)(num << 4) | (uint32_t)(o - CIGAR_STR));
            num = 0;
            have = false;
        }
    }
    return !have;
}

// source/remap.d:11-87 — `fade extract`: one new mapped record per artifact side, built from the am tag
// (contig, 0-based pos, CIGAR), carrying the reverse-complemented read and its reversed qualities.  Pure host
// work: it consumes what the annotate path wrote and so validates the am grammar end to end.
static int extract_main(const std::string &cl, const Opts &o) {
    fprintf(stderr, "[W::fade extract] Output SAM/BAM will not be sorted\n");  // remap.d:13
    const int nthreads = o.threads > 0 ? o.threads : 2;
    Pool pool(nthreads);  // (reader and writer share it)
    try {
        Reader reader(o.pos[1], &pool);  // remap.d:17
        Header hdr = reader.header();
        hdr.add_pg("fade-extract", "fade", FADE_VERSION, cl);  // remap.d:18-26
        const OutFmt fmt = o.bam ? OutFmt::BAM : o.ubam ? OutFmt::UBAM : OutFmt::SAM;
        Writer writer(stdout, fmt, hdr, &pool);
        std::vector<Rec> in, out;
        for (;;) {
            in.clear();
            out.clear();
            if (reader.read_chunk(in, 65536) == 0) break;
            for (const Rec &r : in) {
                const size_t prs = r.aux_find("rs");  // remap.d:31-33
                if (prs == std::string::npos) continue;
                uint32_t rsv = 0;
                const uint8_t ty = r.d[prs + 2];
                if (ty == 'C' || ty == 'c') rsv = r.d[prs + 3];
                else if (ty == 'S' || ty == 's') rsv = r.rd<uint16_t>(prs + 3);
                else if (ty == 'I' || ty == 'i') rsv = r.rd<uint32_t>(prs + 3);
                else continue;
                rsv &= 0xff;
                if (!(rsv & 6)) continue;  // remap.d:36-37
                const size_t pam = r.aux_find("am");  // remap.d:38-40
                if (pam == std::string::npos || r.d[pam + 2] != 'Z') continue;
                const std::string am((const char *)r.d.data() + pam + 3);
                const size_t semi = am.find(';');
                const std::string sides[2] = {am.substr(0, semi), semi == std::string::npos ? std::string() : am.substr(semi + 1)};
                for (int side = 0; side < 2; side++) {
                    if (!(rsv & (side == 0 ? 2u : 4u))) continue;  // remap.d:43,64
                    const std::string &f = sides[side];
                    const size_t c1 = f.find(','), c2 = c1 == std::string::npos ? c1 : f.find(',', c1 + 1);
                    if (c2 == std::string::npos) throw std::runtime_error("malformed am tag: " + am);
                    const int tid = reader.header().tid_of(f.substr(0, c1));
                    const int64_t pos = std::strtoll(f.c_str() + c1 + 1, nullptr, 10);
                    std::vector<uint32_t> cig;
                    if (!parse_cigar_string(f.substr(c2 + 1), cig)) throw std::runtime_error("malformed am CIGAR: " + am);
                    out.push_back(build_extract_rec(r, tid, pos, cig.data(), cig.size()));
                }
            }
            writer.write(out);
        }
        writer.close();
    } catch (const std::exception &e) {
        fprintf(stderr, "[E::fade extract] %s\n", e.what());
        return 1;
    }
    return 0;
}

// ------------------------------------------------------------------ fade out (source/filter.d)
static void print_out_help() {
    fprintf(stderr,
            "%s\nout: removes all read and mates for reads contain the artifact (used after annotate)\n"
            "     or, with the -c flag, hard clips out artifact sequence from reads\n"
            "     it is reccomended that the input SAM/BAM be queryname sorted\n"
            "usage: fade out [options] <input BAM/SAM>\n\n"
            "-c    --clip clip reads instead of filtering them\n"
            "-t --threads extra threads for parsing the bam file\n"
            "-b     --bam output bam\n"
            "-u    --ubam output uncompressed bam\n"
            "      --gpus 1: BAM file in, -b or -u out: filtering or clipping runs on one MI355X (rs and am read back by a kernel)\n"
            " --fragments BAM file in, -b or -u out, on one MI355X: eject every read that shares its name with an artifact read, input in any order (two passes over the file)\n"
            " --fix-mates with -c, BAM file in, -b or -u out, on one MI355X: every read's mate fields (next position, template length, flags 0x8 / 0x20, MC) follow the clip of its mate (three passes over the file)\n"
            "    --calmd REF.fa with -c, BAM file in, -b or -u out, on one MI355X: NM and MD of every hard-clipped read are recomputed against the reference (read through REF.fa.fai when present)\n"
            "--keep-sorted with -c, coordinate-sorted BAM file in, -b or -u out, on one MI355X: clipped records are written at their new coordinates, so the output stays coordinate-sorted\n"
            "      --sort with --gpus 1, BAM file in, in any order, -b or -u out: the output is written in coordinate order (@HD SO:coordinate), sorted on the MI355X; a file too large for it in several passes\n"
            "--write-index PATH: also write the BAM index (.bai) of the output, made in the same pass (coordinate-sorted output, BAM file in, -b or -u out, on one MI355X)\n"
            "--csi with --write-index: the index is a CSI (min_shift 14, depth 5, or 6 for contigs longer than 2^29), not a BAI\n"
            "    --timing print where the run spent its time to stderr\n"
            "-h    --help This help information.\n\n",
            kHeader);
}

// std.conv.parse!long on the front of s: optional sign, digits; consumes what it parsed.  false = ConvException.
static bool d_parse_long(std::string &s, long long &v) {
    size_t k = 0;
    bool neg = false;
    if (k < s.size() && (s[k] == '-' || s[k] == '+')) { neg = s[k] == '-'; k++; }
    if (k >= s.size() || s[k] < '0' || s[k] > '9') return false;
    long long x = 0;
    while (k < s.size() && s[k] >= '0' && s[k] <= '9') { x = x * 10 + (s[k] - '0'); k++; }
    v = neg ? -x : x;
    s.erase(0, k);
    return true;
}

// filter.d:127-167
static int numerically_aware_cmp(std::string a, std::string b) {
    while (!a.empty() && !b.empty()) {
        const bool nda = a[0] > '9' || a[0] < '0', ndb = b[0] > '9' || b[0] < '0';
        if (nda && ndb) {
            if (a[0] == b[0]) { a.erase(0, 1); b.erase(0, 1); continue; }
            return (unsigned char)a[0] < (unsigned char)b[0] ? -1 : 1;
        }
        long long ai = -1, bi = -1;
        const bool pa = d_parse_long(a, ai), pb = d_parse_long(b, bi);
        if (!pa && !pb) return a.size() == b.size() ? 0 : a.size() < b.size() ? -1 : 1;  // cannot happen: one side is a digit
        if (ai == bi) continue;
        return ai < bi ? -1 : 1;
    }
    return a.size() == b.size() ? 0 : a.size() < b.size() ? -1 : 1;
}

static bool rs_of(const Rec &r, uint32_t &rsv) {
    const size_t p = r.aux_find("rs");
    if (p == std::string::npos) return false;
    const uint8_t ty = r.d[p + 2];
    if (ty == 'C' || ty == 'c') rsv = r.d[p + 3];
    else if (ty == 'S' || ty == 's') rsv = r.rd<uint16_t>(p + 3);
    else if (ty == 'I' || ty == 'i') rsv = r.rd<uint32_t>(p + 3);
    else return false;
    rsv &= 0xff;
    return true;
}

struct OutStats {  // stats.d:16-72
    long long read_count = 0, clipped = 0, sup = 0, art_sup = 0, art = 0, art_mate = 0, aln_l = 0, aln_r = 0;
    void parse(uint32_t v) {
        const uint32_t sc = v & 1, al = (v >> 1) & 1, ar = (v >> 2) & 1, ml = (v >> 3) & 1, mr = (v >> 4) & 1, su = (v >> 5) & 1;
        clipped += sc;
        art += (al | ar);
        sup += su;
        art_sup += (al | ar) & su;
        art_mate += ((al & ml) | (ar & mr));
        aln_l += al;
        aln_r += ar;
    }
    static void ratio(const char *label, long long num, long long den) {
        if (den == 0) fprintf(stderr, "%s%s\n", label, num == 0 ? "nan" : "inf");
        else fprintf(stderr, "%s%g\n", label, (double)((float)num / (float)den));
    }
    void print() const {
        fprintf(stderr, "read count:\t%lld\n", read_count);
        ratio("Clipped %:\t", clipped, read_count);
        ratio("% With Supplementary alns:\t", sup, read_count);
        ratio("Artifact rate:\t", art, read_count);
        ratio("% With Supplementary alns and artifacts:\t", art_sup, read_count);
        ratio("Artifact rate left only:\t", aln_l, read_count);
        ratio("Artifact rate right only:\t", aln_r, read_count);
    }
};

static bool q_consuming(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
static bool r_consuming(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

static Rec build_rec(const std::string &qname, int32_t tid, int32_t pos, int mapq, uint16_t flag, int32_t mtid, int32_t mpos,
                     int32_t tlen, const std::vector<uint32_t> &cig, const std::vector<uint8_t> &codes,
                     const std::vector<uint8_t> &qual, const uint8_t *aux, size_t aux_len) {
    Rec n;
    const size_t lqn = qname.size() + 1, lq = codes.size();
    n.d.assign(32 + lqn + 4 * cig.size() + (lq + 1) / 2 + lq + aux_len, 0);
    int64_t reflen = 0;
    for (uint32_t c : cig) if (r_consuming(c & 15)) reflen += c >> 4;
    n.wr<int32_t>(0, tid);
    n.wr<int32_t>(4, pos);
    n.d[8] = (uint8_t)lqn;
    n.d[9] = (uint8_t)mapq;
    n.wr<uint16_t>(10, (uint16_t)reg2bin(pos < 0 ? 0 : pos, (pos < 0 ? 0 : pos) + (reflen > 0 ? reflen : 1)));
    n.wr<uint16_t>(12, (uint16_t)cig.size());
    n.wr<uint16_t>(14, flag);
    n.wr<int32_t>(16, (int32_t)lq);
    n.wr<int32_t>(20, mtid);
    n.wr<int32_t>(24, mpos);
    n.wr<int32_t>(28, tlen);
    memcpy(n.d.data() + 32, qname.c_str(), lqn);
    size_t off = 32 + lqn;
    if (!cig.empty()) memcpy(n.d.data() + off, cig.data(), 4 * cig.size());
    off += 4 * cig.size();
    for (size_t k = 0; k < lq; k++) n.d[off + (k >> 1)] |= (uint8_t)(codes[k] << ((~k & 1) << 2));
    off += (lq + 1) / 2;
    if (lq) memcpy(n.d.data() + off, qual.data(), lq);
    off += lq;
    if (aux_len) memcpy(n.d.data() + off, aux, aux_len);
    return n;
}

// filter.d:15-91 clipRead.  ref_len: the reference bases to take left and right when the caller knows them (`fade annotate -c`:
// the batch's alignment); otherwise they are parsed back from the am tag, as `fade out -c` must.
static void clip_read(Rec &rec, uint32_t rsv, const int64_t *ref_len) {
    std::vector<uint32_t> cig((size_t)rec.n_cigar());
    for (int k = 0; k < rec.n_cigar(); k++) cig[(size_t)k] = rec.cigar_op(k);
    int64_t pos = rec.pos();
    const int lq = rec.l_seq();
    std::vector<uint8_t> codes((size_t)lq), qual((size_t)lq);
    for (int j = 0; j < lq; j++) {
        codes[(size_t)j] = (rec.seq()[j >> 1] >> ((~j & 1) << 2)) & 15;
        qual[(size_t)j] = rec.qual()[j];
    }
    const std::string name = rec.qname();
    size_t sb = 0, se = (size_t)lq;  // surviving [sb, se) of seq / qual
    const size_t pam = rec.aux_find("am");
    const std::string am = pam == std::string::npos ? std::string() : std::string((const char *)rec.d.data() + pam + 3);
    const size_t semi = am.find(';');
    const std::string sides[2] = {am.substr(0, semi), semi == std::string::npos ? std::string() : am.substr(semi + 1)};
    auto art_ref_len = [&](int side) -> int64_t {
        if (ref_len) return ref_len[side];
        const std::string &f = sides[side];
        const size_t c1 = f.find(','), c2 = c1 == std::string::npos ? c1 : f.find(',', c1 + 1);
        std::vector<uint32_t> ac;
        if (c2 == std::string::npos || !parse_cigar_string(f.substr(c2 + 1), ac)) throw std::runtime_error("malformed am tag: " + am);
        int64_t n = 0;
        for (uint32_t c : ac) if (r_consuming(c & 15)) n += c >> 4;
        return n;
    };
    auto aligned_len = [&]() { int64_t n = 0; for (uint32_t c : cig) if (r_consuming(c & 15)) n += c >> 4; return n; };
    auto reset = [&]() {  // filter.d:47-51 / 79-83: a fresh (zero-filled) record keeping name, sequence, qualities
        std::vector<uint8_t> c2(codes.begin() + (long)sb, codes.begin() + (long)se), q2(qual.begin() + (long)sb, qual.begin() + (long)se);
        rec = build_rec(name, 0, 0, 0, 0, 0, 0, 0, {}, c2, q2, nullptr, 0);
    };
    if (rsv & 2) {  // filter.d:22-54
        int64_t to_trim = art_ref_len(0);
        uint32_t hard = 0;
        if (to_trim < aligned_len()) {
            while (to_trim) {
                const uint32_t op = cig[0] & 15;
                if (q_consuming(op)) { if (sb < se) sb++; hard++; }  // (a CIGAR may claim more bases than l_seq holds: none left, none taken)
                if (r_consuming(op)) { pos++; to_trim--; }
                cig[0] -= 16;  // length - 1
                if ((cig[0] >> 4) == 0) cig.erase(cig.begin());
            }
        } else { reset(); return; }
        cig.insert(cig.begin(), (hard << 4) | 5u);
    }
    if (rsv & 4) {  // filter.d:55-86
        int64_t to_trim = art_ref_len(1);
        uint32_t hard = 0;
        if (to_trim < aligned_len()) {
            while (to_trim) {
                const uint32_t op = cig.back() & 15;
                if (q_consuming(op)) { if (se > sb) se--; hard++; }
                if (r_consuming(op)) to_trim--;
                cig.back() -= 16;
                if ((cig.back() >> 4) == 0) cig.pop_back();
            }
        } else { reset(); return; }
        cig.push_back((hard << 4) | 5u);
    }
    // filter.d:87-90: cigar, sequence, qscores, pos; every other field and the aux tags stay
    std::vector<uint8_t> c2(codes.begin() + (long)sb, codes.begin() + (long)se), q2(qual.begin() + (long)sb, qual.begin() + (long)se);
    const size_t ao = rec.aux_off();
    std::vector<uint8_t> aux(rec.d.begin() + (long)ao, rec.d.end());
    rec = build_rec(name, rec.tid(), (int32_t)pos, rec.mapq(), (uint16_t)rec.flag(), rec.mtid(), rec.mpos(), rec.tlen(), cig, c2, q2,
                    aux.data(), aux.size());
}

// filter.d:169-268
static int out_main(const std::string &cl, const Opts &o) {
    const int nthreads = o.threads > 0 ? o.threads : 2;
    Pool pool(nthreads);  // (reader and writer share it)
    try {
        Reader reader(o.pos[1], &pool);
        Header hdr = reader.header();
        hdr.add_pg("fade-extract", "fade", FADE_VERSION, cl);  // filter.d:173-180 (the reference reuses this ID)
        const OutFmt fmt = o.bam ? OutFmt::BAM : o.ubam ? OutFmt::UBAM : OutFmt::SAM;
        Writer writer(stdout, fmt, hdr, &pool);
        OutStats stats;
        std::vector<Rec> in, out;
        auto next_chunk = [&]() { in.clear(); return reader.read_chunk(in, 65536) > 0; };
        if (o.clip) {  // filter.d:184-212
            fprintf(stderr, "[W::fade-out] Using the -c flag means the output SAM/BAM will not be sorted (regardless of prior sorting)\n");
            fprintf(stderr, "[W::fade-out] You also may need to fix mate information with a tool like Picard FixMateInformation\n");
            while (next_chunk()) {
                for (Rec &r : in) {
                    stats.read_count++;
                    uint32_t v;
                    if (rs_of(r, v)) {
                        stats.parse(v);
                        if (v & 6) clip_read(r, v);
                    }
                }
                writer.write(in);
            }
        } else {
            // filter.d:216-220: the first ten records decide whether the input looks name-sorted
            std::vector<Rec> all_first;
            next_chunk();
            bool sorted = true;
            for (size_t k = 1; k < std::min<size_t>(in.size(), 10); k++)
                if (numerically_aware_cmp(in[k].qname(), in[k - 1].qname()) < 0) sorted = false;
            if (sorted) {  // filter.d:221-246
                fprintf(stderr, "[W::fade-out] Output looks name-sorted, ejecting all reads with same readname if any have an artifact\n");
                std::vector<Rec> group;
                auto flush_group = [&]() {
                    bool art_found = false;
                    for (const Rec &r : group) {
                        stats.read_count++;
                        uint32_t v;
                        if (!rs_of(r, v)) continue;
                        stats.parse(v);
                        if (v & 6) art_found = true;
                    }
                    if (!art_found) for (Rec &r : group) out.push_back(std::move(r));
                    group.clear();
                };
                do {
                    out.clear();
                    for (Rec &r : in) {
                        if (!group.empty() && strcmp(group.back().qname(), r.qname()) != 0) flush_group();
                        group.push_back(std::move(r));
                    }
                    writer.write(out);
                } while (next_chunk());
                out.clear();
                if (!group.empty()) flush_group();
                writer.write(out);
            } else {  // filter.d:247-265
                fprintf(stderr, "[W::fade-out] Output doesn't look name-sorted, ejecting by only reads with an artifact\n");
                do {
                    out.clear();
                    for (Rec &r : in) {
                        stats.read_count++;
                        uint32_t v;
                        if (!rs_of(r, v)) continue;  // filter.d:254-257: records without rs are not written here
                        stats.parse(v);
                        if (!(v & 6)) out.push_back(std::move(r));
                    }
                    writer.write(out);
                } while (next_chunk());
            }
        }
        writer.close();
        stats.print();  // filter.d:267
    } catch (const std::exception &e) {
        fprintf(stderr, "[E::fade out] %s\n", e.what());
        return 1;
    }
    return 0;
}

// `fade out [-c] --gpus 1` and `fade extract --gpus 1` on a BAM file with -b or -u: the file path on the device over records
// that were annotated earlier (FADEHIP_BAM_FROM_TAGS) — rs and am are read back out of the records by a kernel, the clip,
// eject and extract kernels are those of `fade annotate -c / --eject / --extract`, and this process moves compressed bytes.
// A reader thread cuts the file at BGZF member boundaries (and, with FADE_BAM_INFLATE=host, inflates the members on the
// pool); this thread alternates front of call k and back of call k - 1, and writes what back hands out.  SAM or piped
// input, SAM output and FADE_BAM_DEVICE=0 take the host loop (*fall_back stays set and nothing has been written).
// `fade out --fragments` (TagsJob::FRAGMENTS) is two runs of that path on one context, the reading loop run twice over the
// file: the first (FADEHIP_BAM_COLLECT_NAMES | NO_OUTPUT) fills a set of names on the device with the artifact calls' names,
// the second (FADEHIP_BAM_EJECT_NAMED) writes every record whose name is not in the set.  It has no host loop behind it:
// where *fall_back stays set, main refuses the run.

// `fade stats --gpus 1` / `fade stats-clip --gpus 1` (TagsJob::STATS / STATS_CLIP) are the same reading loop over a stream
// with FADEHIP_BAM_REPORT_STATS / _CLIP | NO_OUTPUT: the host writes the header line, then what fadehip_bam_back_report hands
// out, to stdout or to the file named behind the input (app.d:168-176).  No host loop behind them either.
// `fade out -c --fix-mates` (TagsJob::FIX_MATES) is three: the names as under --fragments, then (FADEHIP_BAM_COLLECT_MATES |
// CLIP | NO_OUTPUT) the placement of every primary paired-end read of those names into a mate map on the device, then
// (FADEHIP_BAM_FIX_MATES | CLIP, with --keep-sorted and --write-index as asked) the output.  No host loop behind it either.
enum class TagsJob { OUT, EXTRACT, FRAGMENTS, FIX_MATES, STATS, STATS_CLIP };
static int tags_stream_main(const std::string &cl, const Opts &o, TagsJob job, bool *fall_back) {
    *fall_back = true;
    const bool report = job == TagsJob::STATS || job == TagsJob::STATS_CLIP;
    const char *who = job == TagsJob::EXTRACT ? "fade extract" : job == TagsJob::STATS ? "fade stats" : job == TagsJob::STATS_CLIP ? "fade stats-clip" : "fade out";
    const bool fragments = job == TagsJob::FRAGMENTS, fix_mates = job == TagsJob::FIX_MATES;
    const bool sort_out = o.sort && !report && job != TagsJob::EXTRACT;  // `fade out --sort`: the pass that writes keeps its records on the device
    const std::string &path = o.pos[1];
    struct stat sb;
    if (!(o.bam || o.ubam || report) || path == "-" || stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return 1;
    if (getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0) return 1;
    StageClock ck_total, ck_front, ck_back, ck_write;
    ck_total.start();
    const int nthreads = o.threads > 0 ? o.threads : default_threads();
    const char *inf_env = getenv("FADE_BAM_INFLATE");
    const bool host_inflate = inf_env ? strcmp(inf_env, "host") == 0 : nthreads >= 8;
    Pool pool(host_inflate || job == TagsJob::EXTRACT ? nthreads : std::min(nthreads, 4));
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return 1;
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    Header hdr;
    uint64_t coff = 0;
    uint32_t first_rec = 0;
    std::vector<std::string> first_names;  // plain `out`: the names of the first ten records
    try {
        Reader rd(path, &pool);
        if (!rd.is_bam()) return 1;
        hdr = rd.header();
        const size_t hdr_bytes = rd.bam_header_bytes();
        if (job == TagsJob::OUT && !o.clip) {  // the front of the file is inflated here anyway: on to the tenth record
            std::vector<Rec> first;
            rd.read_chunk(first, 10);
            for (const Rec &r : first) first_names.push_back(r.qname());
        }
        // the member that holds the first record, and the record's offset in its payload
        if (!locate_first_record(fileno(f), (uint64_t)sb.st_size, hdr_bytes, &coff, &first_rec)) return 1;  // (other gzip subfields first, say: the host loop reads it)
    } catch (const std::exception &e) {
        return 1;  // the host loop reports what is wrong with the file
    }
    *fall_back = false;
    g_csi_depth = o.csi ? csi_depth_for(hdr) : 0;
    g_csi_who = job == TagsJob::EXTRACT ? "fade extract" : "fade-out";
    if (o.timing) fprintf(stderr, "[timing] since process start %.3f s (%s begins; file path on the device)\n", since_process_start(), who);
    // `fade out -c --calmd REF.fa` (never beside --sort: main refuses that): the @SQ lines held against the FASTA here, before any device is opened and any output
    // written; the genome goes up once the context exists (the loader is `fade annotate`'s, as it stands)
    const bool calmd = !o.calmd.empty() && o.clip && (job == TagsJob::OUT || job == TagsJob::FIX_MATES);
    GenomeSource genome;
    if (calmd) {
        genome.who = "fade-out";
        try {
            if (genome.prepare(o.calmd, hdr.names, hdr.lens)) return 1;
        } catch (const std::exception &e) {
            fprintf(stderr, "[E::fade-out] --calmd: %s\n", e.what());
            return 1;
        }
        for (size_t k = 0; k < hdr.names.size(); k++)
            if (genome.have[k] != hdr.lens[k]) {
                fprintf(stderr, "[E::fade-out] --calmd: %s has LN:%lld in the BAM header and %lld bases in %s: not the reference the reads were aligned to\n", hdr.names[k].c_str(),
                        (long long)hdr.lens[k], (long long)genome.have[k], o.calmd.c_str());
                return 1;
            }
    }
    const int32_t calmd_flag = calmd ? FADEHIP_BAM_CALMD : 0;
    bool grouped = false;
    FILE *rep_out = stdout;  // the report: stdout, or the file named behind the input
    struct RepCloser { FILE *&f; ~RepCloser() { if (f && f != stdout) fclose(f); } } rep_closer{rep_out};
    if (report) {
        if (o.pos.size() > 2 && !(rep_out = fopen(o.pos[2].c_str(), "wb"))) {
            fprintf(stderr, "[E::%s] cannot open %s for writing: %s\n", who, o.pos[2].c_str(), strerror(errno));
            return 1;
        }
    } else if (job == TagsJob::EXTRACT) {
        if (!o.sorted) fprintf(stderr, "[W::fade extract] Output SAM/BAM will not be sorted\n");  // remap.d:13 (--sorted: it will be)
    } else if (fragments) {
        fprintf(stderr, "[W::fade-out] --fragments: ejecting every read that shares its name with an artifact read, input in any order (two passes over the file)\n");
    } else if (o.clip) {  // filter.d:184-185 (--fix-mates: its own line in the place of the second)
        clip_warnings(o);
    } else {
        grouped = eject_mode_grouped(first_names);  // filter.d:216-220, 248
    }
    fadehip_ctx *ctx = nullptr;
    fadehip_bam_stream *st = nullptr;
    fadehip_nameset *names = nullptr;
    fadehip_mateset *mates = nullptr;
    fadehip_recstore *store = nullptr;  // `fade extract --sorted`: the run's extract records, on the device
    fadehip_intervals *repeats = nullptr;  // `fade stats --repeats`: the BED's intervals, on the device
    Staging staging;
    struct Guard {
        fadehip_ctx *&c;
        fadehip_bam_stream *&s;
        fadehip_nameset *&ns;
        fadehip_mateset *&ms;
        fadehip_recstore *&rs;
        fadehip_intervals *&iv;
        Staging &stg;
        ~Guard() {
            if (s) fadehip_bam_close(s);
            if (iv) fadehip_intervals_destroy(iv);
            if (ns) fadehip_nameset_destroy(ns);
            if (ms) fadehip_mateset_destroy(ms);
            if (rs) fadehip_recstore_destroy(rs);
            stg.unpin(c);
            if (c) fadehip_destroy(c);
        }
    } guard{ctx, st, names, mates, store, repeats, staging};
    try {
        fadehip_params prm;
        fadehip_params_default(&prm);
        setenv("FADEHIP_TAIL_CUS", "0", 0);
        setenv("FADEHIP_BLOCKING_SYNC", "1", 0);  // the thread that waits for the device sleeps: the cores are the inflater's
        const int device = getenv("FADE_DEVICE_MAP") ? atoi(getenv("FADE_DEVICE_MAP")) : 0;
        const size_t chunk = (size_t)std::max(1, getenv("FADE_BAM_CHUNK_MB") ? atoi(getenv("FADE_BAM_CHUNK_MB")) : host_inflate ? 32 : 128) << 20;
        // the device is brought up beside the buffers being made and the first members being read
        std::string create_err;
        // a stream of the file path with `mode` beside FROM_TAGS (--fragments: one per pass, on the same set of names)
        auto open_stream = [&](int32_t mode) -> int {
            std::vector<const char *> ref_names;
            for (auto &n : hdr.names) ref_names.push_back(n.c_str());
            fadehip_bam_config cfg;
            memset(&cfg, 0, sizeof cfg);
            cfg.n_ref = (int32_t)ref_names.size();
            cfg.ref_names = ref_names.data();
            cfg.first_record = first_rec;
            cfg.flags = FADEHIP_BAM_FROM_TAGS | mode;
            if (fadehip_bam_open(ctx, &cfg, &st)) { create_err = fadehip_last_error(ctx); return 1; }
            if ((mode & FADEHIP_BAM_INDEX) && IndexFile::stream_geometry(st)) { create_err = fadehip_last_error(ctx); return 1; }  // --csi
            if ((mode & (FADEHIP_BAM_COLLECT_NAMES | FADEHIP_BAM_EJECT_NAMED | FADEHIP_BAM_COLLECT_MATES)) && fadehip_bam_use_nameset(st, names)) { create_err = fadehip_last_error(ctx); return 1; }
            if ((mode & (FADEHIP_BAM_COLLECT_MATES | FADEHIP_BAM_FIX_MATES)) && fadehip_bam_use_mateset(st, mates)) { create_err = fadehip_last_error(ctx); return 1; }
            if ((mode & (FADEHIP_BAM_STORE_EXTRACT | FADEHIP_BAM_STORE_OUTPUT)) && fadehip_bam_use_recstore(st, store)) { create_err = fadehip_last_error(ctx); return 1; }
            if ((mode & FADEHIP_BAM_REPORT_REPEATS) && fadehip_bam_use_intervals(st, repeats)) { create_err = fadehip_last_error(ctx); return 1; }
            const size_t call_bytes = host_inflate ? chunk : std::min<size_t>(chunk * 3, (size_t)1 << 30);
            if (!(getenv("FADE_BAM_PREPARE") && atoi(getenv("FADE_BAM_PREPARE")) == 0) && fadehip_bam_prepare(st, call_bytes)) { create_err = fadehip_last_error(ctx); return 1; }
            return 0;
        };
        // --sort: the stream of the pass that writes, with `mode` as it would be without the option — its records go into a
        // store that measures them under the budget the device allows (fadehip_recstore_set_budget 0), not to the compressor:
        // the drains compress (and index) them once they are in order
        int32_t sorting_mode = 0;
        auto open_sorting = [&](int32_t mode) -> int {
            sorting_mode = mode;
            if (!store) {
                if (fadehip_recstore_create(ctx, &store) || fadehip_recstore_set_budget(store, 0) ||
                    fadehip_recstore_measure(store, (int32_t)hdr.lens.size(), hdr.lens.data())) { create_err = fadehip_last_error(ctx); return 1; }
            }
            return open_stream((mode & ~(FADEHIP_BAM_STORED | FADEHIP_BAM_INDEX)) | FADEHIP_BAM_STORE_OUTPUT);
        };
        std::future<int> creating = std::async(std::launch::async, [&]() -> int {
            if (fadehip_create(&ctx, device, &prm)) { create_err = fadehip_last_error(nullptr); return 1; }
            if (calmd && genome.upload(ctx)) { create_err = "the reference of --calmd did not reach the device"; return 1; }
            if (fragments || fix_mates) {
                if (fadehip_nameset_create(ctx, &names)) { create_err = fadehip_last_error(ctx); return 1; }
                if (fix_mates && fadehip_mateset_create(ctx, &mates)) { create_err = fadehip_last_error(ctx); return 1; }
                return open_stream(FADEHIP_BAM_COLLECT_NAMES | FADEHIP_BAM_NO_OUTPUT);
            }
            if (report && !o.repeats.empty()) {  // the set is loaded and sealed before the first call
                StageClock ck_bed;
                ck_bed.start();
                if (fadehip_intervals_load_bed(ctx, o.repeats.c_str(), &repeats)) { create_err = fadehip_last_error(ctx); return 1; }
                ck_bed.stop();
                int64_t n_iv = 0;
                int32_t n_chrom = 0;
                fadehip_intervals_count(repeats, &n_iv, &n_chrom);
                if (o.timing) fprintf(stderr, "[timing] --repeats: %lld intervals of %d contigs loaded and sealed on the device in %.3f s\n", (long long)n_iv, n_chrom, ck_bed.t);
                return open_stream(FADEHIP_BAM_NO_OUTPUT | FADEHIP_BAM_REPORT_STATS | FADEHIP_BAM_REPORT_REPEATS);
            }
            if (report) return open_stream(FADEHIP_BAM_NO_OUTPUT | (job == TagsJob::STATS ? FADEHIP_BAM_REPORT_STATS : FADEHIP_BAM_REPORT_CLIP));
            int32_t mode = o.ubam ? FADEHIP_BAM_STORED : 0;
            if (job == TagsJob::EXTRACT) mode |= FADEHIP_BAM_EXTRACT | FADEHIP_BAM_NO_OUTPUT;
            if (job == TagsJob::EXTRACT && o.sorted) {  // the records stay on the device until the input is through
                if (fadehip_recstore_create(ctx, &store)) { create_err = fadehip_last_error(ctx); return 1; }
                mode |= FADEHIP_BAM_STORE_EXTRACT;
                return open_stream(mode);  // (--write-index is of the sorted records: the drains make its entries, not the stream)
            }
            else if (o.clip) mode |= FADEHIP_BAM_CLIP | (o.keep_sorted ? FADEHIP_BAM_KEEP_SORTED : 0) | calmd_flag;
            else mode |= grouped ? FADEHIP_BAM_EJECT | FADEHIP_BAM_EJECT_GROUPS : FADEHIP_BAM_EJECT;
            if (sort_out) return open_sorting(mode);
            if (!o.write_index.empty()) mode |= FADEHIP_BAM_INDEX;
            return open_stream(mode);
        });
        struct Joiner { std::future<int> &f; ~Joiner() { if (f.valid()) f.wait(); } } joiner{creating};
        // ---- the reader: compressed bytes cut at member boundaries; HEAD bytes in front of a buffer take the beginning of a
        // member that the previous read cut
        const size_t ccap = host_inflate ? std::max<size_t>(chunk / 2, 1 << 20) : chunk, HEAD = 65536 + 64;
        constexpr int NBUF = 3;
        struct In { uint8_t *p = nullptr; size_t n = 0; bool last = false; int buf = -1; };
        uint8_t *bufs[NBUF];
        std::vector<uint8_t> own_comp;  // host inflate: the compressed bytes never cross PCIe
        for (int k = 0; k < NBUF; k++) bufs[k] = staging.alloc(host_inflate ? chunk + 65536 + 64 : HEAD + ccap + 64);
        if (host_inflate) own_comp.resize(HEAD + ccap + 64);
        // (the queues and the reader thread are made per pass over the file: --fragments makes two)
        std::unique_ptr<BoundedQueue<int>> q_free_p;
        std::unique_ptr<BoundedQueue<In>> q_full_p;
        std::string stage_err;
        std::mutex err_m;
        auto set_err = [&](const std::string &e) {
            std::lock_guard<std::mutex> l(err_m);
            if (stage_err.empty()) stage_err = e;
        };
        std::unique_ptr<StageThreads> stages_p;
        auto start_pass = [&] {
          stages_p.reset();
          q_free_p.reset(new BoundedQueue<int>(NBUF + 1));
          q_full_p.reset(new BoundedQueue<In>(NBUF + 1));
          BoundedQueue<int> &q_free = *q_free_p;
          BoundedQueue<In> &q_full = *q_full_p;
          for (int k = 0; k < NBUF; k++) q_free.push(k);
          stages_p.reset(new StageThreads);
          stages_p->unblock = [&q_free, &q_full] { q_free.close(); q_full.close(); };
          stages_p->th.emplace_back([&, qf = q_free_p.get(), qu = q_full_p.get()] {
            BoundedQueue<int> &q_free = *qf;
            BoundedQueue<In> &q_full = *qu;
            try {
                uint64_t at = coff;
                MemberCutter cutter;
                std::vector<Mem> ms;
                bool eof = false;
                while (!eof) {
                    int k = -1;
                    if (!host_inflate && !q_free.pop(k)) break;
                    uint8_t *base = host_inflate ? own_comp.data() : bufs[k];
                    const size_t got = read_fill(fileno(f), base + HEAD, ccap, &at, UINT64_MAX, &eof, path);
                    const MemberCutter::Cut cut = cutter.cut(base, HEAD, got, eof, ms, path);
                    if (!host_inflate) {
                        In in;
                        in.p = cut.cb; in.n = cut.w; in.last = eof; in.buf = k;
                        q_full.push(in);
                        continue;
                    }
                    size_t m0 = 0;
                    do {  // batches of members whose payloads fill a staging buffer
                        size_t total = 0;
                        const size_t m1 = take_batch(ms, m0, chunk, &total);
                        if (!q_free.pop(k)) return;
                        uint8_t *dst = bufs[k];
                        if (!inflate_batch(pool, cut.cb, ms, m0, m1, dst)) throw std::runtime_error("BGZF block does not inflate to its ISIZE / CRC32 (corrupt input)");
                        In in;
                        in.p = dst; in.n = total; in.last = eof && m1 == ms.size(); in.buf = k;
                        q_full.push(in);
                        m0 = m1;
                    } while (m0 < ms.size());
                }
            } catch (const std::exception &e) {
                set_err(e.what());
            }
            q_full.close();
          });
        };
        start_pass();
        // ---- the header, as the host loop writes it; the records follow from the device (`extract`: through the Writer)
        Header out_hdr = hdr;
        out_hdr.add_pg("fade-extract", "fade", FADE_VERSION, cl);  // filter.d:173-180 / remap.d:18-26 (the reference reuses this ID)
        if (creating.get()) { fprintf(stderr, "[E::%s] cannot open the GPU path: %s\n", who, create_err.c_str()); return 1; }
        if (!staging.pin(ctx)) { fprintf(stderr, "[E::%s] %s\n", who, fadehip_last_error(ctx)); return 1; }
        const OutFmt fmt = o.ubam ? OutFmt::UBAM : OutFmt::BAM;
        std::unique_ptr<Writer> xwriter;
        std::vector<Rec> xrecs;
        IndexSink index;  // --write-index (`fade out`; with --fragments the second pass, which writes the output)
        auto take_back = [&]() {
            const uint8_t *p = nullptr;
            size_t n = 0;
            ck_back.start();
            const int rc = fadehip_bam_back(st, &p, &n);
            ck_back.stop();
            if (rc) throw std::runtime_error(fadehip_last_error(ctx));
            note_held(o, st);
            if (index.on()) index.call(st, ctx, n);
            ck_write.start();
            if (report) {
                const uint8_t *tp = nullptr;
                size_t tn = 0;
                int64_t n_rows = 0;
                if (fadehip_bam_back_report(st, job == TagsJob::STATS ? FADEHIP_BAM_REPORT_STATS : FADEHIP_BAM_REPORT_CLIP, &tp, &tn, &n_rows)) throw std::runtime_error(fadehip_last_error(ctx));
                if (tn && fwrite(tp, 1, tn, rep_out) != tn) throw std::runtime_error("write error on the report");
            } else if (xwriter) {
                const uint8_t *xp = nullptr;
                size_t xn = 0;
                int64_t n_x = 0;
                if (fadehip_bam_back_extract(st, &xp, &xn, &n_x)) throw std::runtime_error(fadehip_last_error(ctx));
                split_extract_records(xp, xn, xrecs);
                if (!xrecs.empty()) xwriter->write(xrecs);
            } else if (n && fwrite(p, 1, n, stdout) != n) throw std::runtime_error("write error on the output stream");
            ck_write.stop();
        };
        // one pass over the file: front of call k, back of call k - 1, until the reader is through
        auto run_calls = [&]() -> int {
        BoundedQueue<int> &q_free = *q_free_p;
        BoundedQueue<In> &q_full = *q_full_p;
        StageThreads &stages = *stages_p;
        In in;
        bool waiting = false, ended = false;
        while (q_full.pop(in)) {
            ck_front.start();
            const int rc = host_inflate ? fadehip_bam_front_raw(st, in.p, in.n, in.last ? 1 : 0) : fadehip_bam_front(st, in.p, in.n, in.last ? 1 : 0);
            ck_front.stop();
            if (rc) throw std::runtime_error(fadehip_last_error(ctx));
            q_free.push(in.buf);
            ended |= in.last;
            if (waiting) take_back();  // (call k - 1, while call k runs on the device)
            waiting = true;
        }
        if (waiting && stage_err.empty()) take_back();
        stages.unblock();
        for (auto &t : stages.th) t.join();
        stages.unblock = nullptr;
        if (!stage_err.empty()) { fprintf(stderr, "[E::%s] %s\n", who, stage_err.c_str()); return 1; }
        if (!ended) { fprintf(stderr, "[E::%s] the input ended before its last call\n", who); return 1; }
        return 0;
        };
        if (fragments || fix_mates) {  // pass 1: the names of the artifact calls; then the stream of pass 2, and the reader again
            StageClock ck_pass;
            ck_pass.start();
            if (run_calls()) return 1;
            int64_t n_names = 0, totals1[8], n_rec1 = 0;
            if (fadehip_nameset_count(names, &n_names)) { fprintf(stderr, "[E::%s] %s\n", who, fadehip_last_error(ctx)); return 1; }
            fadehip_bam_totals(st, totals1, &n_rec1, nullptr);
            fadehip_bam_close(st);
            st = nullptr;
            ck_pass.stop();
            if (o.timing)
                fprintf(stderr, "[timing] pass 1 (names of the artifact calls into the set) %.3f s: front %.3f | back %.3f; %lld records, %lld names collected\n", ck_pass.t, ck_front.t,
                        ck_back.t, (long long)n_rec1, (long long)n_names);
            ck_front = StageClock();
            ck_back = StageClock();
            ck_write = StageClock();
            const int32_t mode2 = fix_mates ? FADEHIP_BAM_COLLECT_MATES | FADEHIP_BAM_CLIP | FADEHIP_BAM_NO_OUTPUT
                                            : FADEHIP_BAM_EJECT_NAMED | (o.ubam ? FADEHIP_BAM_STORED : 0) | (o.write_index.empty() ? 0 : FADEHIP_BAM_INDEX);
            if (fragments && sort_out ? open_sorting(mode2) : open_stream(mode2)) {
                fprintf(stderr, "[E::%s] cannot open the GPU path: %s\n", who, create_err.c_str());
                return 1;
            }
            start_pass();
        }
        if (fix_mates) {  // pass 2: the placements of those names' primary paired-end reads; then the stream of pass 3
            StageClock ck_pass;
            ck_pass.start();
            if (run_calls()) return 1;
            int64_t n_entries = 0, n_amb = 0;
            if (fadehip_mateset_count(mates, &n_entries, &n_amb)) { fprintf(stderr, "[E::%s] %s\n", who, fadehip_last_error(ctx)); return 1; }
            fadehip_bam_close(st);
            st = nullptr;
            ck_pass.stop();
            if (o.timing)
                fprintf(stderr, "[timing] pass 2 (placements of the reads of those names into the mate map) %.3f s: front %.3f | back %.3f; %lld placements stored, %lld of them ambiguous\n",
                        ck_pass.t, ck_front.t, ck_back.t, (long long)n_entries, (long long)n_amb);
            ck_front = StageClock();
            ck_back = StageClock();
            ck_write = StageClock();
            const int32_t mode3 = FADEHIP_BAM_FIX_MATES | FADEHIP_BAM_CLIP | (o.ubam ? FADEHIP_BAM_STORED : 0) | (o.keep_sorted ? FADEHIP_BAM_KEEP_SORTED : 0) |
                                  (o.write_index.empty() ? 0 : FADEHIP_BAM_INDEX) | calmd_flag;  // (the pass that writes: the two in front of it only name and place)
            if (sort_out ? open_sorting(mode3) : open_stream(mode3)) {
                fprintf(stderr, "[E::%s] cannot open the GPU path: %s\n", who, create_err.c_str());
                return 1;
            }
            start_pass();
        }
        StageClock ck_pass2;
        ck_pass2.start();
        if (report) {
            fputs(job == TagsJob::STATS ? "qname\trname\tpos\tcigar\tart_start\tart_end\taln_rname\taln_start\taln_end\tart_cigar\tstemloop\tstemloop_rc\t"
                                          "predicted_inverted_repeat\tIR_identity\tavgbq\tart_avgbq\tart_bq\tIR_bq\tflagbinary\tflag\tstrand"
                                        : "qname\tsc_q_scores\tsc_seq\tsc_avg_bq\tavg_bq\tart_status", rep_out);
            fputs(repeats ? "\tread_rpm\tart_rpm\n" : "\n", rep_out);
        } else if (job == TagsJob::EXTRACT && o.sorted) {
            // (nothing is written while the input streams through: header, records and marker follow the sort)
        } else if (job == TagsJob::EXTRACT) xwriter.reset(new Writer(stdout, fmt, out_hdr, &pool));
        else if (sort_out) {
            // (nothing either: whether the records leave in one window or in several is known when the input is through)
        } else if (!o.write_index.empty()) {
            index.open(o.write_index, hdr.names.size());
            index.header([&](FILE *to) {
                Writer hw(to, fmt, out_hdr, &pool, nullptr, true, false);
                hw.close();
            });
        } else {
            Writer hw(stdout, fmt, out_hdr, &pool, nullptr, true, false);  // (its members only: no end-of-file block yet)
            hw.close();
        }
        if (run_calls()) return 1;
        int64_t totals[8], n_rec = 0, n_over = 0, n_ej = 0;  // (of this pass: under --sort more passes may follow, one per window)
        fadehip_bam_totals(st, totals, &n_rec, &n_over);
        fadehip_bam_ejected(st, &n_ej);
        int64_t n_fixed = 0, n_amb = 0;
        if (fix_mates) fadehip_bam_mates(st, &n_fixed, &n_amb);
        int64_t n_calmd = 0, n_calmd_skipped = 0;
        if (calmd) fadehip_bam_calmd(st, &n_calmd, &n_calmd_skipped);
        if (report) {
            if (fflush(rep_out) != 0 || ferror(rep_out)) { fprintf(stderr, "[E::%s] write error on the report\n", who); return 1; }
        } else if (xwriter) xwriter->close();
        else if (sort_out) {
            StageClock ck_sorted;
            ck_sorted.start();
            int32_t over = 0;
            if (fadehip_recstore_over(store, &over)) throw std::runtime_error(fadehip_last_error(ctx));
            int64_t n_reset = 0;
            if (fadehip_recstore_resets(store, &n_reset)) throw std::runtime_error(fadehip_last_error(ctx));
            if (n_reset && !o.write_index.empty()) {  // (known before a byte is on stdout: the pass has only measured and stored)
                fprintf(stderr, "[E::fade-out] --sort --write-index: %lld reads are clipped to nothing; they are written zero-filled (refID 0, pos 0) at the end of the file, and a file that ends "
                                "in them is not in coordinate order by its own bytes, so no index can be made of it (samtools index refuses it too): run without --write-index, or drop those "
                                "reads from the input\n", (long long)n_reset);
                return 1;
            }
            SortedWriter sw(ctx, stdout, o.ubam, o.write_index);
            size_t n_windows = 1;
            if (!over) {
                sw.begin(out_hdr, &pool);
                sw.window(store);
            } else {
                // the records do not fit the device at once: the key space in windows that each fit, cut from the table the
                // pass has measured, and one more pass over the input per window
                int64_t nb = 0;
                if (fadehip_recstore_histogram(store, nullptr, nullptr, &nb)) throw std::runtime_error(fadehip_last_error(ctx));
                std::vector<uint64_t> hb((size_t)nb), hr((size_t)nb);
                if (fadehip_recstore_histogram(store, hb.data(), hr.data(), &nb)) throw std::runtime_error(fadehip_last_error(ctx));
                uint64_t budget = 0;
                if (fadehip_recstore_budget(store, &budget)) throw std::runtime_error(fadehip_last_error(ctx));
                std::vector<uint32_t> len32;
                for (int64_t l : hdr.lens) len32.push_back((uint32_t)l);
                fadehip::recstore::BucketLayout lay;
                fadehip::recstore::bucket_layout(len32.data(), len32.size(), lay);
                std::vector<fadehip::recstore::SortWindow> wins;
                const int64_t bad = fadehip::recstore::choose_windows(hb.data(), hr.data(), (uint32_t)nb, budget, wins);
                uint64_t all_bytes = 0;
                for (uint64_t b : hb) all_bytes += b;
                if (bad >= 0) {
                    uint64_t lo, hi;
                    int64_t ref;
                    fadehip::recstore::bucket_range(lay, (uint32_t)bad, &lo, &hi, &ref);
                    fprintf(stderr, "[E::fade-out] --sort: the records of %s from position %llu on take %llu bytes (%llu records), more than the budget of %llu bytes lets the device hold at once: "
                                    "a window of the sort is at least 65,536 positions\n", ref >= 0 ? hdr.names[(size_t)ref].c_str() : "no contig (unmapped)",
                            (unsigned long long)((uint32_t)lo ? (uint32_t)lo - 1u : 0u), (unsigned long long)hb[(size_t)bad], (unsigned long long)hr[(size_t)bad], (unsigned long long)budget);
                    return 1;
                }
                n_windows = wins.size();
                fprintf(stderr, "[W::fade-out] --sort: %llu bytes of records do not fit the budget of %llu bytes on the device: written in %zu windows, one more pass over the input for each\n",
                        (unsigned long long)all_bytes, (unsigned long long)budget, n_windows);
                sw.begin(out_hdr, &pool);
                for (const auto &w : wins) {
                    uint64_t lo, hi, unused;
                    fadehip::recstore::bucket_range(lay, w.b0, &lo, &unused);
                    fadehip::recstore::bucket_range(lay, w.b1 - 1, &unused, &hi);
                    fadehip_bam_close(st);
                    st = nullptr;
                    if (fadehip_recstore_reset(store, w.bytes, w.records) || fadehip_recstore_set_window(store, lo, hi)) throw std::runtime_error(fadehip_last_error(ctx));
                    if (open_sorting(sorting_mode)) { fprintf(stderr, "[E::%s] cannot open the GPU path: %s\n", who, create_err.c_str()); return 1; }
                    start_pass();
                    if (run_calls()) return 1;
                    sw.window(store);
                }
            }
            sw.finish();
            ck_sorted.stop();
            if (o.timing) fprintf(stderr, "[timing] --sort: %lld records sorted on the device and written in coordinate order in %zu window%s, %.3f s behind the first pass\n", (long long)sw.total,
                                  n_windows, n_windows == 1 ? "" : "s", ck_sorted.t);
        } else if (store) {
            StageClock ck_sorted;
            ck_sorted.start();
            const int64_t n_sorted = write_sorted_store(ctx, store, stdout, o.ubam, out_hdr, &pool, o.write_index);
            ck_sorted.stop();
            if (o.timing) fprintf(stderr, "[timing] --sorted: %lld records sorted on the device and written in coordinate order in %.3f s\n", (long long)n_sorted, ck_sorted.t);
        } else if (fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, stdout) != sizeof BGZF_EOF) { fprintf(stderr, "[E::%s] write error on the output stream\n", who); return 1; }
        if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "[E::%s] write error on the output stream\n", who); return 1; }
        if (index.on()) index.write();
        report_held(o);
        ck_pass2.stop();
        if (fragments && o.timing)
            fprintf(stderr, "[timing] pass 2 (records whose name is not in the set) %.3f s: front %.3f | back %.3f | write %.3f\n", ck_pass2.t, ck_front.t, ck_back.t, ck_write.t);
        if (fix_mates && o.timing) {
            fprintf(stderr, "[timing] pass 3 (clip, mate fields from the map, write) %.3f s: front %.3f | back %.3f | write %.3f; %lld records fixed, %lld left alone (mate ambiguous)\n", ck_pass2.t,
                    ck_front.t, ck_back.t, ck_write.t, (long long)n_fixed, (long long)n_amb);
        }
        if (calmd) {
            if (o.timing) genome.report();
            fprintf(stderr, "[I::fade-out] --calmd: NM and MD recomputed in %lld hard-clipped reads, %lld left as they were (unmapped, off the reference, or a CIGAR that does not fit the bases)\n",
                    (long long)n_calmd, (long long)n_calmd_skipped);
        }
        if (job != TagsJob::EXTRACT && !report) {  // filter.d:267
            OutStats stats;
            stats.read_count = totals[0]; stats.clipped = totals[1]; stats.sup = totals[2]; stats.art_sup = totals[3];
            stats.art = totals[4]; stats.art_mate = totals[5]; stats.aln_l = totals[6]; stats.aln_r = totals[7];
            stats.print();
        }
        ck_total.stop();
        if (o.timing)
            fprintf(stderr, "[timing] total %.3f s (%s, file path on the device, inflate on the %s): front (%sframe, tags read back) %.3f | back (%s, copy out) %.3f | write %.3f; "
                            "%lld records, %lld not written\n",
                    ck_total.t, who, host_inflate ? "host" : "device", host_inflate ? "" : "inflate, ", ck_front.t, report ? "report rows" : job == TagsJob::EXTRACT ? "extract records" : o.ubam ? "store" : "deflate",
                    ck_back.t, ck_write.t, (long long)n_rec, (long long)n_ej);
    } catch (const std::exception &e) {
        fprintf(stderr, "[E::%s] %s\n", who, e.what());
        return 1;
    }
    return 0;
}

// --keep-sorted (`fade annotate -c`, `fade out -c`): why the option cannot run as the command line stands, or nullptr.  Looks
// at the options, the environment and the first bytes of the input: no device is opened for it.
static const char *const kKeepSortedInput = "the input is read as a coordinate-sorted BAM file on the device: not SAM text, not a pipe";
static const char *keep_sorted_refusal(const Opts &o) {
    if (!o.clip) return "without -c no record moves: the option goes with -c";
    if (o.eject) return "--eject drops the artifact reads, and nothing is left to put in order: not with --eject";
    if (o.fragments) return "--fragments ejects the artifact reads, and nothing is left to put in order: not with --fragments";
    if (!(o.bam || o.ubam)) return "the output is SAM text: --keep-sorted writes BAM (-b) or uncompressed BAM (-u)";
    if (o.gpus > 1 || !o.out_shards.empty())
        return "it goes with one device: the devices of --gpus N > 1 and --out-shards cut the input at BGZF ranges, and the tail one holds back would belong into the next one's range";
    if (getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0) return "FADE_BAM_DEVICE=0 takes the device away, and the held tail lives on it (no host loop)";
    const std::string &path = o.pos[1];
    struct stat sb;
    uint8_t h[4] = {0, 0, 0, 0};
    bool bgzf = false;
    if (path != "-" && stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode))
        if (FILE *f = fopen(path.c_str(), "rb")) {
            bgzf = fread(h, 1, 4, f) == 4 && h[0] == 0x1f && h[1] == 0x8b && (h[3] & 4);
            fclose(f);
        }
    return bgzf ? nullptr : kKeepSortedInput;
}

// --write-index PATH (`fade annotate`, `fade out`): why the option cannot run as the command line stands, or "".  The entries
// are made on the device in the pass that writes the output: there is no host loop behind the option.  Looks at the options,
// the environment and the first bytes of the input: no device is opened for it.
static const char *const kWriteIndexInput = "the input is read as a BAM file on the device: not SAM text, not a pipe";
static std::string write_index_refusal(const Opts &o, bool reports) {
    if (!(o.bam || o.ubam)) return "the output is SAM text: an index is of BAM (-b) or uncompressed BAM (-u)";
    if (o.gpus > 1) return "it goes with one device: not with --gpus N > 1 (the devices' indexes are not merged)";
    if (!o.out_shards.empty()) return "it goes with one device and one output: not with --out-shards";
    if (getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0) return "FADE_BAM_DEVICE=0 takes the device away, and the index is made on it (no host loop)";
    if (reports) return std::string("the run with ") + (!o.stats_tsv.empty() ? "--stats-tsv" : "--clip-tsv") + " does not take the file path on the device: not with it";
    const std::string &path = o.pos[1];
    struct stat sb, sa;
    if (o.write_index == "-") return "PATH is a file of its own: not the standard output";
    if (o.write_index == path || (stat(o.write_index.c_str(), &sa) == 0 && stat(path.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino))
        return "PATH is a file of its own: not the input";
    uint8_t h[4] = {0, 0, 0, 0};
    bool bgzf = false;
    if (path != "-" && stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode))
        if (FILE *f = fopen(path.c_str(), "rb")) {
            bgzf = fread(h, 1, 4, f) == 4 && h[0] == 0x1f && h[1] == 0x8b && (h[3] & 4);
            fclose(f);
        }
    return bgzf ? "" : kWriteIndexInput;
}

// --csi: the option says how an index is written, so without an index to write it is refused, by name, before any device is opened.
static const char *const kCsiNoIndex = "it says how the index is written (a CSI, for references longer than 2^29): the option goes with --write-index PATH";

// --sort (`fade out`): why the option cannot run as the command line stands, or "".  The output's records are kept, sorted and
// compressed on one device: there is no host loop behind the option.  Looks at the options, the environment and the first bytes
// of the input: no device is opened for it.
static const char *const kSortInput = "the input is read as a BAM file on the device, once per pass: not SAM text, not a pipe";
static std::string sort_refusal(const Opts &o, bool annotate) {
    if (o.keep_sorted) return "--keep-sorted holds back a tail of coordinate-sorted input, and --sort already gives the order for input in any order: not with --keep-sorted";
    if (!(o.bam || o.ubam)) return "the output is SAM text: --sort writes BAM (-b) or uncompressed BAM (-u)";
    if (annotate) {
        if (!o.out_shards.empty()) return "it goes with one device and one output: not with --out-shards";
        if (!o.extract.empty() || o.extract_sorted)
            return std::string("the record store holds the main output: not with ") + (o.extract_sorted ? "--extract-sorted" : "--extract") + " (run fade extract --gpus 1 --sorted on the annotated file)";
        if (!o.stats_tsv.empty() || !o.clip_tsv.empty())
            return std::string("the run with ") + (!o.stats_tsv.empty() ? "--stats-tsv" : "--clip-tsv") + " does not take the file path on the device: not with it";
    } else if (o.seen.find('g') == std::string::npos) return "it goes with --gpus 1 (the records are kept and sorted on the device; there is no host loop)";
    if (o.gpus != 1) return "it goes with one device: not with --gpus N other than 1 (the store of records lives on one device)";
    if (getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0) return "FADE_BAM_DEVICE=0 takes the device away, and the records are kept and sorted on it (no host loop)";
    const std::string &path = o.pos[1];
    struct stat sb;
    uint8_t h[4] = {0, 0, 0, 0};
    bool bgzf = false;
    if (path != "-" && stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode))
        if (FILE *f = fopen(path.c_str(), "rb")) {
            bgzf = fread(h, 1, 4, f) == 4 && h[0] == 0x1f && h[1] == 0x8b && (h[3] & 4);
            fclose(f);
        }
    return bgzf ? "" : kSortInput;
}

// --sorted (`fade extract`) and --extract-sorted (`fade annotate`): why the option cannot run as the command line stands, or
// "".  The records are kept, sorted and compressed on one device: there is no host loop behind either option.  Looks at the
// options, the environment and the first bytes of the input: no device is opened for it.  `first`: a reason the caller has.
static const char *const kSortedExtractInput = "the input is read as a BAM file on the device: not SAM text, not a pipe";
static std::string sorted_extract_refusal(const Opts &o, const std::string &first) {
    if (!first.empty()) return first;
    if (o.gpus > 1) return "it goes with one device: not with --gpus N > 1 (the store of records lives on one device)";
    if (!o.out_shards.empty()) return "it goes with one device and one output: not with --out-shards";
    if (!(o.bam || o.ubam)) return "the output is SAM text: the sorted extract is BAM (-b) or uncompressed BAM (-u)";
    if (getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0) return "FADE_BAM_DEVICE=0 takes the device away, and the records are kept and sorted on it (no host loop)";
    const std::string &path = o.pos[1];
    struct stat sb;
    uint8_t h[4] = {0, 0, 0, 0};
    bool bgzf = false;
    if (path != "-" && stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode))
        if (FILE *f = fopen(path.c_str(), "rb")) {
            bgzf = fread(h, 1, 4, f) == 4 && h[0] == 0x1f && h[1] == 0x8b && (h[3] & 4);
            fclose(f);
        }
    return bgzf ? "" : kSortedExtractInput;
}

// --gpus for `fade out` / `fade extract`: 1 is the file path on the device where the input and output allow it, more is not built
static bool tags_gpus_ok(const Opts &o, const char *who) {
    if (o.seen.find('g') == std::string::npos || o.gpus == 1) return true;
    fprintf(stderr, "[E::%s] --gpus %d: this subcommand runs on one device (--gpus 1) or on the host (no --gpus)\n", who, o.gpus);
    return false;
}

int main(int argc, char **argv) {
    std::string cl;  // app.d:66
    for (int i = 0; i < argc; i++) { if (i) cl += ' '; cl += argv[i]; }
    if (argc == 1) { print_full_help(); return 0; }  // app.d:67-73
    const std::string sub = argv[1];
    if (sub == "annotate") {
        Opts o;
        std::string err;
        if (!parse_opts(argc, argv, o, err)) {
            fprintf(stderr, "std.getopt.GetOptException: %s\n", err.c_str());
            return 1;
        }
        if (!o.repeats.empty()) {  // refused here, by name, before any device is opened
            fprintf(stderr, "[E::fade-annotate] --repeats: %s\n", !o.stats_tsv.empty() ? "the repeat columns of --stats-tsv are out of scope: run fade stats --gpus 1 --repeats PATH on the annotated file"
                                                                                      : "the option goes with fade stats --gpus 1 (it adds two columns to that report's rows)");
            return 1;
        }
        if (!options_allowed(o, "tmwbucgBsTSPQXEKIYZNJ")) return 1;
        if (!o.calmd.empty()) {  // recognised, and refused by name: the fused pass also edits rs / am / as / ar / ab, and its rewrite kernel does not call the NM / MD functions yet
            fprintf(stderr, "[E::fade-annotate] --calmd: not built for the annotate pass; annotate first, then: fade out -c --calmd %s --gpus 1 -b <annotated BAM>\n", o.calmd.c_str());
            return 1;
        }
        // app.d:84-89: helpWanted | args.length < 3 (args = prog, "annotate", positionals...)
        if (o.help || o.pos.size() < 2) { print_anno_help(); return 0; }
        if (o.pos.size() < 3) {  // the reference indexes args[2] and dies; say why instead
            print_anno_help();
            fprintf(stderr, "[E::fade-annotate] an indexed fasta reference is required\n");
            return 1;
        }
        if (o.bam && o.ubam) {  // app.d:94-99
            fprintf(stderr, "[E::fade-annotate] Please use only one of the b or u flags\n");
            return 1;
        }
        const bool reports = !o.stats_tsv.empty() || !o.clip_tsv.empty();
        if (reports && (o.gpus > 1 || !o.out_shards.empty())) {  // the reports are written in record order by one writer
            fprintf(stderr, "[E::fade-annotate] %s goes with one device: not with %s\n", !o.stats_tsv.empty() ? "--stats-tsv" : "--clip-tsv",
                    o.gpus > 1 ? "--gpus N > 1" : "--out-shards");
            return 1;
        }
        if (reports && o.clip) {  // the reports describe the unclipped records
            fprintf(stderr, "[E::fade-annotate] %s describes unclipped records: not with --clip\n", !o.stats_tsv.empty() ? "--stats-tsv" : "--clip-tsv");
            return 1;
        }
        if (o.sort) {  // refused here, by name, before any device is opened: the records are kept and sorted on one device, and there is no host loop
            const std::string why = sort_refusal(o, true);
            if (!why.empty()) {
                fprintf(stderr, "[E::fade-annotate] --sort: %s\n", why.c_str());
                return 1;
            }
        }
        if (o.keep_sorted) {  // refused here, by name, before any device is opened
            if (const char *why = keep_sorted_refusal(o)) {
                fprintf(stderr, "[E::fade-annotate] --keep-sorted: %s\n", why);
                return 1;
            }
        }
        if (o.csi && o.write_index.empty() && !o.extract_sorted) {  // refused here, by name, before any device is opened
            fprintf(stderr, "[E::fade-annotate] --csi: %s or --extract-sorted\n", kCsiNoIndex);
            return 1;
        }
        if (!o.write_index.empty()) {  // refused here, by name, before any device is opened
            const std::string why = write_index_refusal(o, reports);
            if (!why.empty()) {
                fprintf(stderr, "[E::fade-annotate] --write-index: %s\n", why.c_str());
                return 1;
            }
        }
        if (o.eject) {  // refused here, before any device is opened
            if (o.clip) {
                fprintf(stderr, "[E::fade-annotate] --eject drops the artifact reads and --clip keeps them hard-clipped: `fade out` does one or the other\n");
                return 1;
            }
            if (reports) {
                fprintf(stderr, "[E::fade-annotate] %s describes records that --eject drops from the output: not with --eject\n", !o.stats_tsv.empty() ? "--stats-tsv" : "--clip-tsv");
                return 1;
            }
            if (o.gpus > 1 || !o.out_shards.empty()) {
                fprintf(stderr, "[E::fade-annotate] --eject goes with one device: not with %s (the devices' ranges of the input would cut through name groups)\n",
                        o.gpus > 1 ? "--gpus N > 1" : "--out-shards");
                return 1;
            }
        }
        if (!o.extract.empty()) {  // one file, written in record order by one writer — refused here, before any device is opened
            if (o.gpus > 1 || !o.out_shards.empty()) {
                fprintf(stderr, "[E::fade-annotate] --extract goes with one device: not with %s\n", o.gpus > 1 ? "--gpus N > 1" : "--out-shards");
                return 1;
            }
            struct stat sa, sb2;
            const bool same = o.extract == o.pos[1] || (stat(o.extract.c_str(), &sa) == 0 && stat(o.pos[1].c_str(), &sb2) == 0 && sa.st_dev == sb2.st_dev && sa.st_ino == sb2.st_ino);
            if (o.extract == "-" || same) {
                fprintf(stderr, "[E::fade-annotate] --extract PATH is a file of its own: not %s\n", o.extract == "-" ? "the standard output" : "the input");
                return 1;
            }
        }
        if (o.extract_sorted) {  // the store lives on one device: there is no host loop behind the option — refused here, by name
            const std::string why = sorted_extract_refusal(o, o.extract.empty() ? "it says how the --extract file is written: the option goes with --extract PATH"
                                                              : reports ? std::string("the run with ") + (!o.stats_tsv.empty() ? "--stats-tsv" : "--clip-tsv") + " does not take the file path on the device: not with it" : "");
            if (!why.empty()) {
                fprintf(stderr, "[E::fade-annotate] --extract-sorted: %s\n", why.c_str());
                return 1;
            }
        }
        if (!o.out_shards.empty() && o.gpus < 2) {
            fprintf(stderr, "[E::fade-annotate] --out-shards PREFIX writes one file per device: it goes with --gpus N (N >= 2)\n");
            return 1;
        }
        if (!o.extract.empty() && !o.extract_sorted) fprintf(stderr, "[W::fade extract] Output SAM/BAM will not be sorted\n");  // remap.d:13
        if (o.clip && !lane_env().on) clip_warnings(o);  // filter.d:184-185, as `fade out -c` (once: the lanes of --gpus N stay silent)
        // --gpus N on a BAM file: one process per GPU, each on its own share of the input (annotate_lanes_main); input that
        // cannot be cut (a pipe, SAM text, a small file) is read by one process that deals batches to the N devices
        if (o.gpus > 1 && !lane_env().on && !(getenv("FADE_LANES") && atoi(getenv("FADE_LANES")) == 0)) {
            bool fall_back = true;
            const int lrc = annotate_lanes_main(cl, o, &fall_back);
            if (lrc == 0 || !fall_back) return lrc;
            if (!o.out_shards.empty()) {
                fprintf(stderr, "[E::fade-annotate] --out-shards needs an input that can be cut into ranges: a BAM file (not a pipe, not SAM text) of at least %d BGZF blocks\n", 8 * o.gpus);
                return 1;
            }
        }
        // BAM file in, BAM or uBAM out: the file path on the device (FADE_BAM_DEVICE=0: the host pipeline)
        if (!reports && (o.bam || o.ubam) && (o.gpus <= 1 || lane_env().on) && !(getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0)) {
            bool fall_back = true;
            const int src = annotate_stream_main(cl, o, &fall_back);
            if (src == 0 || !fall_back) return src;
        }
        if (o.sort) {  // the store lives on the device: there is no host loop behind this option
            fprintf(stderr, "[E::fade-annotate] --sort: %s\n", kSortInput);
            return 1;
        }
        if (o.keep_sorted) {  // the tail is held on the device: there is no host loop behind this option
            fprintf(stderr, "[E::fade-annotate] --keep-sorted: %s\n", kKeepSortedInput);
            return 1;
        }
        if (!o.write_index.empty()) {  // nor behind this one
            fprintf(stderr, "[E::fade-annotate] --write-index: %s\n", kWriteIndexInput);
            return 1;
        }
        if (o.extract_sorted) {  // nor behind this one
            fprintf(stderr, "[E::fade-annotate] --extract-sorted: %s\n", kSortedExtractInput);
            return 1;
        }
        const int rc = annotate_main(cl, o);
        if (o.timing) {
            long rss_kb = 0, hwm_kb = 0;
            if (FILE *f = fopen("/proc/self/status", "r")) {
                char line[256];
                while (fgets(line, sizeof line, f)) {
                    sscanf(line, "VmRSS: %ld", &rss_kb);
                    sscanf(line, "VmHWM: %ld", &hwm_kb);
                }
                fclose(f);
            }
            if (const char *dump = getenv("FADE_SMAPS_DUMP")) {  // tools/smaps_top.py
                FILE *fi = fopen("/proc/self/smaps", "r"), *fo = fopen(dump, "w");
                char buf[4096];
                size_t n;
                while (fi && fo && (n = fread(buf, 1, sizeof buf, fi)) > 0) fwrite(buf, 1, n, fo);
                if (fi) fclose(fi);
                if (fo) fclose(fo);
            }
            fprintf(stderr, "[timing] since process start %.3f s (annotate returned); resident %ld MB, peak %ld MB\n", since_process_start(),
                    rss_kb >> 10, hwm_kb >> 10);
        }
        return rc;
    }
    if (sub == "extract") {  // app.d:130-153
        Opts o;
        std::string err;
        if (!parse_opts(argc, argv, o, err)) {
            fprintf(stderr, "std.getopt.GetOptException: %s\n", err.c_str());
            return 1;
        }
        if (!options_allowed(o, "tbugTOISNJ")) return 1;
        if (!o.calmd.empty()) {  // recognised, and refused by name
            fprintf(stderr, "[E::fade extract] --calmd: extract writes new records of the artifact sides, which carry no NM or MD: the option goes with fade out -c\n");
            return 1;
        }
        if (o.help || o.pos.size() < 2) { print_extract_help(); return 0; }
        if (!o.write_index.empty() && !o.sorted) {  // refused here, by name, before any device is opened
            // (in std.getopt's words, as before --sorted existed: without it this subcommand has no such option)
            fprintf(stderr, "std.getopt.GetOptException: Unrecognized option --write-index without --sorted\n"
                            "[E::fade extract] --write-index: the extract records leave in the order of the input's reads, and an index is of coordinate-sorted records: the option goes with --sorted\n");
            return 1;
        }
        if (o.csi && o.write_index.empty()) {  // refused here, by name, before any device is opened
            fprintf(stderr, "[E::fade extract] --csi: %s (with --sorted)\n", kCsiNoIndex);
            return 1;
        }
        if (!o.out_shards.empty()) {
            fprintf(stderr, "[E::fade extract] --out-shards: this subcommand writes one output%s\n", o.sorted ? " (--sorted puts the whole run's records in one order: not with --out-shards)" : "");
            return 1;
        }
        if (o.sorted) {  // the store lives on one device: there is no host loop behind the option
            const std::string why = sorted_extract_refusal(o, o.seen.find('g') == std::string::npos ? "it goes with --gpus 1 (the records are kept and sorted on the device; there is no host loop)" : "");
            if (!why.empty()) {
                fprintf(stderr, "[E::fade extract] --sorted: %s\n", why.c_str());
                return 1;
            }
            if (!o.write_index.empty()) {
                struct stat sa, sb2;
                const bool same = o.write_index == o.pos[1] || (stat(o.write_index.c_str(), &sa) == 0 && stat(o.pos[1].c_str(), &sb2) == 0 && sa.st_dev == sb2.st_dev && sa.st_ino == sb2.st_ino);
                if (o.write_index == "-" || same) {
                    fprintf(stderr, "[E::fade extract] --write-index: PATH is a file of its own: not %s\n", o.write_index == "-" ? "the standard output" : "the input");
                    return 1;
                }
            }
        }
        if (!tags_gpus_ok(o, "fade extract")) return 1;
        if (o.bam && o.ubam) {
            fprintf(stderr, "[E::fade-annotate] Please use only one of the b or u flags\n");  // app.d:149 (sic)
            return 1;
        }
        if (o.sorted) {
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::EXTRACT, &fall_back);
            if (fall_back) fprintf(stderr, "[E::fade extract] --sorted: %s\n", kSortedExtractInput);
            return fall_back ? 1 : rc;
        }
        if (o.seen.find('g') != std::string::npos) {  // --gpus 1: the file path on the device, where input and output allow it
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::EXTRACT, &fall_back);
            if (!fall_back) return rc;
        }
        return extract_main(cl, o);
    }
    if (sub == "out") {  // app.d:102-129
        Opts o;
        std::string err;
        if (!parse_opts(argc, argv, o, err)) {
            fprintf(stderr, "std.getopt.GetOptException: %s\n", err.c_str());
            return 1;
        }
        if (!o.calmd.empty() && !o.out_shards.empty()) {  // (refused by its own name: fade out takes no --out-shards at all)
            fprintf(stderr, "[E::fade-out] --calmd: --out-shards writes one file per device, and --calmd goes with one device (--gpus 1): not with --out-shards\n");
            return 1;
        }
        if (!options_allowed(o, "ctbugTFKIMZNJ")) return 1;
        if (o.help || o.pos.size() < 2) { print_out_help(); return 0; }
        if (!o.calmd.empty()) {  // refused here, by name, before any device is opened: the genome lives on one device, and there is no host loop
            const char *why = !o.clip ? "without -c no record is clipped and NM and MD stay true: the option goes with -c"
                              : o.fragments ? "--fragments ejects the artifact reads instead of clipping them, and no NM or MD goes stale: not with --fragments"
                              : o.sort ? "the record store behind --sort does not take the option yet: not with --sort (coordinate-sorted input stays sorted under --keep-sorted)"
                              : !(o.bam || o.ubam) ? "the output is SAM text: --calmd writes BAM (-b) or uncompressed BAM (-u)"
                              : o.seen.find('g') != std::string::npos && o.gpus != 1 ? "it goes with one device (--gpus 1): the genome the fields are computed against lives on it"
                              : getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0 ? "FADE_BAM_DEVICE=0 takes the device away, and --calmd runs on it alone (no host loop)"
                              : nullptr;
            if (why) {
                fprintf(stderr, "[E::fade-out] --calmd: %s\n", why);
                return 1;
            }
        }
        if (o.sort) {  // refused here, by name, before any device is opened: the records are kept and sorted on one device, and there is no host loop
            const std::string why = sort_refusal(o, false);
            if (!why.empty()) {
                fprintf(stderr, "[E::fade-out] --sort: %s\n", why.c_str());
                return 1;
            }
        }
        if (o.fix_mates) {  // refused here, by name, before any device is opened: the map lives on one device, and there is no host loop
            const char *why = !o.clip ? "without -c no record moves and no mate field goes stale: the option goes with -c"
                              : o.fragments ? "--fragments ejects the artifact reads with every read of their name, and no mate is left to fix: not with --fragments"
                              : !(o.bam || o.ubam) ? "the output is SAM text: --fix-mates writes BAM (-b) or uncompressed BAM (-u)"
                              : o.seen.find('g') != std::string::npos && o.gpus != 1 ? "it goes with one device (--gpus 1): the mate map lives on it"
                              : getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0 ? "FADE_BAM_DEVICE=0 takes the device away, and --fix-mates runs on it alone (no host loop)"
                              : nullptr;
            if (why) {
                fprintf(stderr, "[E::fade-out] --fix-mates: %s\n", why);
                return 1;
            }
        }
        if (o.keep_sorted) {  // refused here, by name, before any device is opened
            if (const char *why = keep_sorted_refusal(o)) {
                fprintf(stderr, "[E::fade-out] --keep-sorted: %s\n", why);
                return 1;
            }
        }
        if (o.csi && o.write_index.empty()) {  // refused here, by name, before any device is opened
            fprintf(stderr, "[E::fade-out] --csi: %s\n", kCsiNoIndex);
            return 1;
        }
        if (!o.write_index.empty()) {  // refused here, by name, before any device is opened
            const std::string why = write_index_refusal(o, false);
            if (!why.empty()) {
                fprintf(stderr, "[E::fade-out] --write-index: %s\n", why.c_str());
                return 1;
            }
        }
        if (!tags_gpus_ok(o, "fade out")) return 1;
        if (o.bam && o.ubam) {
            fprintf(stderr, "[E::fade-annotate] Please use only one of the b or u flags\n");  // app.d:122 (sic)
            return 1;
        }
        static const char *const kCalmdInput = "the input is read as a BAM file on the device: not SAM text, not a pipe, not the standard input";
        if (o.fix_mates) {
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::FIX_MATES, &fall_back);
            if (fall_back && !o.calmd.empty()) fprintf(stderr, "[E::fade-out] --calmd: %s\n", kCalmdInput);
            if (fall_back) fprintf(stderr, "[E::fade-out] --fix-mates: the input is read three times, as a BAM file on the device: not SAM text, not a pipe, not %s\n", o.pos[1].c_str());
            return fall_back ? 1 : rc;
        }
        if (o.keep_sorted) {  // the tail is held on the device: there is no host loop behind this option either (--gpus 1 is implied)
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::OUT, &fall_back);
            if (fall_back) fprintf(stderr, "[E::fade-out] --keep-sorted: %s\n", kKeepSortedInput);
            return fall_back ? 1 : rc;
        }
        if (o.fragments) {  // the set of names lives on the device: there is no host loop behind this option
            const char *why = o.clip ? "-c clips the artifact reads and --fragments ejects them with every read of their name: one or the other"
                              : !(o.bam || o.ubam) ? "the output is SAM text: --fragments writes BAM (-b) or uncompressed BAM (-u)"
                              : getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0 ? "FADE_BAM_DEVICE=0 takes the device away, and --fragments runs on it alone (no host loop)"
                              : nullptr;
            if (why) {
                fprintf(stderr, "[E::fade-out] --fragments: %s\n", why);
                return 1;
            }
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::FRAGMENTS, &fall_back);
            if (fall_back) fprintf(stderr, "[E::fade-out] --fragments: the input is read twice, as a BAM file on the device: not SAM text, not a pipe, not %s\n", o.pos[1].c_str());
            return fall_back ? 1 : rc;
        }
        if (!o.calmd.empty()) {  // the genome lives on the device: no host loop behind this option (--gpus 1 is implied; --write-index rides along)
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::OUT, &fall_back);
            if (fall_back) fprintf(stderr, "[E::fade-out] --calmd: %s\n", kCalmdInput);
            return fall_back ? 1 : rc;
        }
        if (o.sort) {  // the store lives on the device: no host loop behind this option either
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::OUT, &fall_back);
            if (fall_back) fprintf(stderr, "[E::fade-out] --sort: %s\n", kSortInput);
            return fall_back ? 1 : rc;
        }
        if (!o.write_index.empty()) {  // the entries are made on the device: no host loop behind this option either (--gpus 1 is implied)
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::OUT, &fall_back);
            if (fall_back) fprintf(stderr, "[E::fade-out] --write-index: %s\n", kWriteIndexInput);
            return fall_back ? 1 : rc;
        }
        if (o.seen.find('g') != std::string::npos) {  // --gpus 1: the file path on the device, where input and output allow it
            bool fall_back = true;
            const int rc = tags_stream_main(cl, o, TagsJob::OUT, &fall_back);
            if (!fall_back) return rc;
        }
        return out_main(cl, o);
    }
    if (sub == "stats" || sub == "stats-clip") {  // app.d:154-209
        Opts o;
        std::string err;
        const bool parsed = parse_opts(argc, argv, o, err), with_gpus = parsed && o.seen.find('g') != std::string::npos;
        if (parsed && !o.repeats.empty()) {  // refused here, by name, before any device is opened
            const std::string no_bed = fadehip::bed::path_refusal(o.repeats);
            struct stat rsb;
            const char *why = sub != "stats" ? "the rows of stats-clip carry no coordinates: the option goes with fade stats"
                              : !with_gpus ? "it goes with --gpus 1 (the intervals are held and queried on the device; there is no host loop)"
                              : !no_bed.empty() ? no_bed.c_str()
                              : (stat(o.repeats.c_str(), &rsb) != 0 || !S_ISREG(rsb.st_mode)) ? "the BED file is read as a plain file: not a pipe, not a directory, not a missing path" : nullptr;
            if (why) {
                fprintf(stderr, "[E::fade %s] --repeats: %s\n", sub.c_str(), why);
                return 1;
            }
        }
        if (!with_gpus) {
            fprintf(stderr, "[E::fade] %s is outside the MI355X annotate hot path; run the reference fade for it, or write its report "
                            "during the run: fade annotate %s PATH.  On an annotated BAM file one MI355X writes it: fade %s --gpus 1 <annotated BAM> [out.tsv]\n",
                    sub.c_str(), sub == "stats" ? "--stats-tsv" : "--clip-tsv", sub.c_str());
            return 1;
        }
        const std::string who = "fade " + sub;
        if (!options_allowed(o, "tgTR")) return 1;
        if (o.help || o.pos.size() < 2 || o.pos.size() > 3) { print_report_help(sub == "stats"); return o.pos.size() > 3 ? 1 : 0; }
        if (o.gpus != 1) {
            fprintf(stderr, "[E::%s] --gpus %d: the report is written on one device (--gpus 1)\n", who.c_str(), o.gpus);
            return 1;
        }
        // the rows are written on the device alone: there is no host loop behind the option
        if (getenv("FADE_BAM_DEVICE") && atoi(getenv("FADE_BAM_DEVICE")) == 0) {
            fprintf(stderr, "[E::%s] --gpus 1: FADE_BAM_DEVICE=0 takes the device away, and the report is written on it alone (no host loop)\n", who.c_str());
            return 1;
        }
        bool fall_back = true;
        const int rc = tags_stream_main(cl, o, sub == "stats" ? TagsJob::STATS : TagsJob::STATS_CLIP, &fall_back);
        if (fall_back) fprintf(stderr, "[E::%s] --gpus 1: the input is read as an annotated BAM file on the device: not SAM text, not a pipe, not %s\n", who.c_str(), o.pos[1].c_str());
        return fall_back ? 1 : rc;
    }
    if (sub == "-h" || sub == "--help") { print_full_help(); return 0; }
    fprintf(stderr, "[E::fade] %s is not a fade subcommand\n", sub.c_str());  // app.d:218-220
    print_full_help();
    return 1;
}
