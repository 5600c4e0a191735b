/// extern(C) binding of include/fadehip.h (ABI version 3) for the D host of blachlylab/fade.
///
/// NOT COMPILED IN THIS REPOSITORY'S ENVIRONMENT: the build image has no D compiler (ldc2, dmd, gdc, dub are
/// all absent) and none of FADE's dependencies, so this file has never been compiled or run.  It mirrors
/// include/fadehip.h declaration by declaration; the same ABI is exercised from C++ (fade_amd/csrc/host) and
/// from Python/ctypes (fade_amd/_lib.py) by the test suite.
module fadehip;

extern (C) nothrow @nogc:

enum FADEHIP_ABI_VERSION = 3;
enum FADEHIP_MAX_OPS = 16;
enum FADEHIP_MAX_QUERY = 512;
enum FADEHIP_MAX_LONG_QUERY = 32768;
enum FADEHIP_NUM_SLOTS = 4;

enum : int
{
    FADEHIP_OK = 0,
    FADEHIP_E_INVALID = -1,
    FADEHIP_E_NODEVICE = -2,
    FADEHIP_E_HIP = -3,
    FADEHIP_E_NOMEM = -4,
    FADEHIP_E_UNSUPPORTED = -5,
    FADEHIP_E_STATE = -6,
    FADEHIP_E_RESIDUE = -7,
    FADEHIP_E_RCCL = -8
}

struct fadehip_ctx;

/// Parasail("ACTGN", open, ext, match, mismatch) -- source/anno.d:36
struct fadehip_params
{
    int open = 10;
    int ext = 2;
    int match = 2;
    int mismatch = -3;
    int max_ref_len = 1 << 20;
    int max_batch_reads = 1 << 20;
    long trace_bytes = 0;
    int trace_all = 0;
    uint rules = FADEHIP_RULES_DEFAULT; /// FADEHIP_RULE_* : the assumptions about libparasail that could not be checked
}

/// same bits as oracle/fade_oracle.h FO_RULE_* (SURVEY.md Appendix A)
enum : uint
{
    FADEHIP_RULE_END_MIN_REF_THEN_QUERY = 1u << 0,
    FADEHIP_RULE_HDIR_DIAG_F_E = 1u << 1,
    FADEHIP_RULE_GAP_TIE_EXTENDS = 1u << 2,
    FADEHIP_RULE_EQ_BY_CHAR = 1u << 3,
    FADEHIP_RULE_SAM_GAP_LETTERS = 1u << 4,
    FADEHIP_RULE_PAD_SOFTCLIP = 1u << 5,
    FADEHIP_RULE_N_MATCHES_N = 1u << 6,
    FADEHIP_RULES_DEFAULT = 0x7f
}

/// what source/analysis.d:69-113 reads from a dparasail result
struct fadehip_sw_result
{
    int score;
    int end_query, end_ref;
    int beg_query, beg_ref; /// beg_ref == res.position
    int n_ops;
    uint[FADEHIP_MAX_OPS] ops; /// BAM-encoded: castable to dhtslib CigarOp
}

struct fadehip_read_batch
{
    int n_reads;
    const(int)* tid;
    const(int)* pos;
    const(ushort)* flag;
    const(ubyte)* has_sa;
    const(int)* l_seq;
    const(uint)* cigar_off;
    const(uint)* cigar_ops;
    const(uint)* seq_off;
    const(ubyte)* seq_packed;
    int n_skipped; /// records left out because anno.d:61-65 gives them rs = 0 (unmapped, no S op)
    int ref_span_bound; /// max cigar.alignedLength over the batch, 0 = let the library scan the CIGARs
    int n_with_seq;     /// ABI 3: records whose seq_off slice is not empty (0 = unknown)
    int l_seq_min;      /// ABI 3: bounds of l_seq over the records with bases (0 = unknown)
    int l_seq_max;
    int reserved;
}

struct fadehip_aln
{
    int read_idx;
    int art; /// bit0 art_left, bit1 art_right
    long win_start;
    int win_len;
    int clip_left, clip_right;
    int aligned_len;
    fadehip_sw_result sw;
}

struct fadehip_anno_out
{
    ubyte* rs;
    fadehip_aln* aln;
    int aln_cap;
    int n_aln;
    long[8] stats;
    int n_oversize;
    int reserved;
}

/// zero-copy results: views into the slot's pinned result block, valid until the slot is uploaded again
struct fadehip_anno_view
{
    const(ubyte)* rs;
    const(fadehip_aln)* aln;
    int n_reads, n_aln;
    long[8] stats;
    int n_oversize;
    int reserved;
}

void fadehip_params_default(fadehip_params* p);
int fadehip_abi_version();
int fadehip_create(fadehip_ctx** out_, int device, const(fadehip_params)* params);
void fadehip_destroy(fadehip_ctx* ctx);
const(char)* fadehip_last_error(const(fadehip_ctx)* ctx);
int fadehip_host_alloc(fadehip_ctx* ctx, size_t bytes, void** out_);
int fadehip_host_free(fadehip_ctx* ctx, void* p);
int fadehip_host_register(fadehip_ctx* ctx, void* p, size_t bytes);
size_t fadehip_batch_bytes(int n_reads, long n_cigar_ops, long n_seq_bytes);
int fadehip_batch_bind(void* base, int n_reads, long n_cigar_ops, long n_seq_bytes, fadehip_read_batch* b);
int fadehip_sw_batch(fadehip_ctx* ctx, int n, const(ubyte)* q, const(long)* q_off,
        const(ubyte)* r, const(long)* r_off, fadehip_sw_result* out_);
/// parasail's stats mode (stats.d:123,164): Parasail(alphabet, open, ext, match, mismatch).aligner!("sw","stats","striped","16")
struct fadehip_sw_stats_result { int score, end_query, end_ref, matches, similar, length; }
int fadehip_sw_stats_batch(fadehip_ctx* ctx, const(int)* scoring4 /* open, ext, match, mismatch */, int n,
        const(ubyte)* q, const(long)* q_off, const(ubyte)* r, const(long)* r_off, fadehip_sw_stats_result* out_);
/// filter.d:15-91 clipRead over n BAM records (block_size first), concatenated: record k loses trim_left[k] reference bases at
/// the front when rs[k] & 2, trim_right[k] at the back when rs[k] & 4, or is reset; out_off receives n + 1 offsets into out_
int fadehip_clip_batch(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, const(ubyte)* rs,
        const(int)* trim_left, const(int)* trim_right, ubyte* out_, long out_cap, long* out_off);
/// fadehip_clip_batch, then NM and MD of every record that leaves hard-clipped recomputed against the uploaded genome; updated: [n] out, 0 untouched, 1 updated, 2 skipped
int fadehip_calmd_batch(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, const(ubyte)* rs,
                        const(int)* trim_left, const(int)* trim_right, ubyte* out_, long out_cap, long* out_off, ubyte* updated);
/// remap.d:11-87 (`fade extract`) over n BAM records: side 2k (left, built when rs[k] & 2) and 2k + 1 (right, rs[k] & 4) of record k
/// become new mapped records on contig art_tid[s] at the 0-based art_pos[s] with the ops cig[cig_off[s] .. cig_off[s + 1]), the read
/// reverse-complemented, its qualities reversed; out_off receives 2n + 1 offsets into out_ (a side whose bit is clear takes nothing)
int fadehip_extract_batch(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, const(ubyte)* rs,
        const(int)* art_tid, const(long)* art_pos, const(long)* cig_off, const(uint)* cig, ubyte* out_, long out_cap, long* out_off);
/// filter.d:209-265 (plain `fade out`) over n BAM records: keep[k] = 1 when record k would be written.  grouped == 0: ejected when
/// rs[k] & 6; grouped != 0 (name-sorted input): a run of consecutive records with equal names is ejected as a whole when one has rs & 6
int fadehip_eject_batch(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, const(ubyte)* rs, int grouped, ubyte* keep);
/// remap.d:31-50, filter.d:24-25,58-59,190-196: rs and am read back out of n BAM records into the arrays the three calls above take.
/// have[k]: bit 0 an integer rs (rs[k] its low byte), bit 1 an am:Z, bits 2 / 3 its left / right side is "name,pos,cigar"; per such side
/// s = 2k + side the contig (first of that name in ref_names, or -1), the position and the ops cig[cig_off[s] .. cig_off[s + 1]);
/// trim_left / trim_right the reference bases those ops take.  More ops than cig_cap: FADEHIP_E_INVALID, nothing written
int fadehip_tags_batch(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, int n_ref, const(char*)* ref_names,
        ubyte* rs, ubyte* have, int* trim_left, int* trim_right, int* art_tid, long* art_pos, long* cig_off, uint* cig, long cig_cap);
/// The rows of `fade stats` (which = FADEHIP_BAM_REPORT_STATS) or `fade stats-clip` (FADEHIP_BAM_REPORT_CLIP) over records annotated earlier, as TSV text written on the device; row_off [2n + 1]: slot 2k is record k's left side, 2k + 1 its right side
int fadehip_report_batch(fadehip_ctx* ctx, int which, int n, const(ubyte)* recs, const(long)* rec_off, int n_ref, const(char*)* ref_names,
                         ubyte* out_, long out_cap, long* row_off);
/// order[j]: the record that comes j-th in stable coordinate order — by (refID, pos + 1) as unsigned, ties in the order given
int fadehip_coord_order_batch(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, int* order);
/// The .bai entries of coordinate-sorted records (include/fadehip.h states the rule): chunks are runs of one (refID, bin), linear
/// entries the 16 kb windows a mapped record newly reaches, refs runs of one refID (-1 included); offsets are BGZF virtual offsets
struct fadehip_index_chunk { int tid; uint bin; ulong beg, end; }
struct fadehip_index_linear { int tid; uint window; ulong off; }
struct fadehip_index_ref { int tid; int reserved; ulong off_beg, off_end, n_mapped, n_unmapped; }
struct fadehip_index_call
{
    const(fadehip_index_chunk)* chunks;
    const(fadehip_index_linear)* linear;
    const(fadehip_index_ref)* refs;
    long n_chunks, n_linear, n_refs, n_records;
    ulong first_key, last_key;
}
/// ... of n records the caller brings at the virtual offsets voff [n + 1]; *out_ points into memory of the ctx
int fadehip_index_batch(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, const(ulong)* voff, fadehip_index_call* out_);
/// The host's part: the calls' entries, rebased by the file offset of each call's first member, become one .bai
struct fadehip_bai;
fadehip_bai* fadehip_bai_create(int n_ref);
int fadehip_bai_add(fadehip_bai* b, ulong base_file_offset, const(fadehip_index_call)* call);
int fadehip_bai_finish(fadehip_bai* b, const(ubyte)** bytes, size_t* n);
const(char)* fadehip_bai_error(const(fadehip_bai)* b);
void fadehip_bai_destroy(fadehip_bai* b);
/// The same entries under a CSI geometry (4 <= min_shift, 1 <= depth <= 8, min_shift + 3 * depth <= 32): bins of a tree of that depth,
/// windows of 2^min_shift positions, the span held to 2^(min_shift + 3 * depth); (14, 5) gives fadehip_index_batch's arrays
int fadehip_index_batch_csi(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, const(ulong)* voff, int min_shift, int depth, fadehip_index_call* out_);
/// ... and the host's part: one .csi's UNCOMPRESSED payload (every bin with its loffset, the pseudo-bin, n_no_coor); the writer puts it into BGZF members
struct fadehip_csi;
fadehip_csi* fadehip_csi_create(int n_ref, int min_shift, int depth);
int fadehip_csi_add(fadehip_csi* b, ulong base_file_offset, const(fadehip_index_call)* call);
int fadehip_csi_finish(fadehip_csi* b, const(ubyte)** payload, size_t* n);
const(char)* fadehip_csi_error(const(fadehip_csi)* b);
void fadehip_csi_destroy(fadehip_csi* b);
/// A set of read names resident on the device (`fade out --fragments`): exact, growing; records in the shapes fadehip_eject_batch takes.
/// add_batch: the names of the records with pick[k] != 0 (pick null: every record); contains_batch: hit[k] = 1 when record k's name is
/// in the set; count: distinct names.  A malformed record: FADEHIP_E_INVALID with its index, the set unchanged.
struct fadehip_nameset;
int fadehip_nameset_create(fadehip_ctx* ctx, fadehip_nameset** out_);
int fadehip_nameset_add_batch(fadehip_nameset* s, int n, const(ubyte)* recs, const(long)* rec_off, const(ubyte)* pick);
int fadehip_nameset_contains_batch(fadehip_nameset* s, int n, const(ubyte)* recs, const(long)* rec_off, ubyte* hit);
int fadehip_nameset_count(fadehip_nameset* s, long* n_names);
void fadehip_nameset_destroy(fadehip_nameset* s);
struct fadehip_mateset;
int fadehip_mateset_create(fadehip_ctx* ctx, fadehip_mateset** out_);
int fadehip_mateset_add_batch(fadehip_mateset* s, int n, const(ubyte)* recs, const(long)* rec_off, const(ubyte)* rs,
                              const(int)* trim_left, const(int)* trim_right, const(ubyte)* pick);
int fadehip_mates_fix_batch(fadehip_mateset* s, int n, const(ubyte)* recs, const(long)* rec_off, const(ubyte)* rs,
                            const(int)* trim_left, const(int)* trim_right, ubyte* out_, long out_cap, long* out_off, ubyte* fixed);
int fadehip_mateset_count(fadehip_mateset* s, long* n_entries, long* n_ambiguous);
void fadehip_mateset_destroy(fadehip_mateset* s);
/// A store of BAM records on the device: added in any order (add_batch, or a FADEHIP_BAM_STORE_EXTRACT stream), sorted once by
/// (refID, pos + 1) as unsigned with ties in the order added, drained in that order (fadehip.h, DESIGN.md 3.8l)
struct fadehip_recstore;
enum FADEHIP_RECSTORE_RAW = 1;     /// fadehip_recstore_drain's flags: the records back to back, no codec
enum FADEHIP_RECSTORE_STORED = 2;  /// ... stored BGZF members (0: members from the device compressor)
enum FADEHIP_RECSTORE_INDEX = 4;   /// ... beside 0 or STORED: *idx also gets the drained records' .bai entries, relative to the drain's first member
int fadehip_recstore_create(fadehip_ctx* ctx, fadehip_recstore** out_);
int fadehip_recstore_add_batch(fadehip_recstore* s, int n, const(ubyte)* recs, const(long)* rec_off, const(ubyte)* pick);
int fadehip_recstore_count(fadehip_recstore* s, long* n_records, long* n_bytes);
int fadehip_recstore_sort(fadehip_recstore* s);
int fadehip_recstore_drain(fadehip_recstore* s, int flags, ulong max_payload, const(ubyte)** out_, size_t* out_bytes, long* n_records, fadehip_index_call* idx);
int fadehip_recstore_index_geometry(fadehip_recstore* s, int min_shift, int depth);  /// before the first drain: FADEHIP_RECSTORE_INDEX hands out the entries of a CSI of that geometry
void fadehip_recstore_destroy(fadehip_recstore* s);
/// the sorted main output (FADEHIP_BAM_STORE_OUTPUT streams): the most the store may cost, bytes + 64 per record (0: derived
/// from the device's free memory; FADEHIP_RECSTORE_BUDGET overrides); the bucket table over the header's contig lengths, from
/// which the windows of a file that does not fit are cut, and whether the measured pass went over the budget; the window of
/// keys a pass keeps, both ends inclusive; reset empties the store for the next window, sized once for what is coming
int fadehip_recstore_set_budget(fadehip_recstore* s, ulong bytes);
int fadehip_recstore_budget(fadehip_recstore* s, ulong* bytes);  /// the budget in force; 0: none set
int fadehip_recstore_measure(fadehip_recstore* s, int n_ref, const(long)* ref_len);
int fadehip_recstore_over(fadehip_recstore* s, int* over);
int fadehip_recstore_resets(fadehip_recstore* s, long* n_reset);  /// reset records (zero-filled, sorted last) the STORE_OUTPUT streams wrote: a file that ends in them cannot be indexed
int fadehip_recstore_histogram(fadehip_recstore* s, ulong* bytes, ulong* records, long* n_buckets);
int fadehip_recstore_set_window(fadehip_recstore* s, ulong lo_key, ulong hi_key_inclusive);
int fadehip_recstore_reset(fadehip_recstore* s, ulong bytes, ulong records);

/// A set of genomic intervals on the device and the overlap query over it (what `bedtools subtract -A` against a RepeatMasker
/// BED decides): intervals (chrom, start, end), chrom an index into the names given at create, 0-based half-open,
/// 0 <= start < end <= 2^31 - 1, added in any order and sealed once; a query (chrom, qs, qe) of longs, which may be negative,
/// hits iff qs < qe and an interval of that chrom shares a base with it.  A bad interval fails its add by index and adds nothing;
/// load_bed is create + add in pieces + seal over a plain-text BED file (names in order of first appearance).
struct fadehip_intervals;
int fadehip_intervals_create(fadehip_ctx* ctx, int n_chrom, const(char*)* chrom_names, fadehip_intervals** out_);
int fadehip_intervals_add(fadehip_intervals* s, long n, const(int)* chrom, const(long)* start, const(long)* end);
int fadehip_intervals_seal(fadehip_intervals* s);
int fadehip_intervals_count(fadehip_intervals* s, long* n_intervals, int* n_chrom);
int fadehip_intervals_overlap_batch(fadehip_intervals* s, long n, const(int)* chrom, const(long)* start, const(long)* end, ubyte* hit);
int fadehip_intervals_load_bed(fadehip_ctx* ctx, const(char)* path, fadehip_intervals** out_);
void fadehip_intervals_destroy(fadehip_intervals* s);
/// fadehip_report_batch's stats rows with two more columns, read_rpm and art_rpm: 1 where (rname, art_start, art_end) /
/// (aln_rname, aln_start, aln_end), as the row prints them, overlap an interval of the sealed set
int fadehip_report_batch_repeats(fadehip_ctx* ctx, int n, const(ubyte)* recs, const(long)* rec_off, int n_ref, const(char*)* ref_names,
                                 fadehip_intervals* intervals, ubyte* out_, long out_cap, long* row_off);
int fadehip_genome_upload(fadehip_ctx* ctx, int n_contigs, const(long)* lengths, const(ubyte*)* seqs);
/// columns 2-5 of a .fai line: bases to take, file offset of the first base (of the uncompressed text), bases and bytes per line
struct fadehip_fai_entry { long length, offset; int line_bases, line_width; }
/// the same genome read by the library from the FASTA file (plain or bgzip) through its index: contig c is entries[c]
int fadehip_genome_upload_fasta(fadehip_ctx* ctx, const(char)* path, int n_contigs, const(fadehip_fai_entry)* entries);
/// fetchSequence (analysis.d:63) on the uploaded genome: n upper-case letters of contig tid from the 0-based start
int fadehip_genome_fetch(fadehip_ctx* ctx, int tid, long start, long n, ubyte* out_);
int fadehip_annotate_upload(fadehip_ctx* ctx, int slot, const(fadehip_read_batch)* batch);
int fadehip_annotate_run(fadehip_ctx* ctx, int slot, int floor_len, int window);
int fadehip_annotate_submit(fadehip_ctx* ctx, int slot, const(fadehip_read_batch)* batch,
        int floor_len, int window);
int fadehip_annotate_results(fadehip_ctx* ctx, int slot, fadehip_anno_view* out_);
int fadehip_annotate_collect(fadehip_ctx* ctx, int slot, fadehip_anno_out* out_);
int fadehip_sync(fadehip_ctx* ctx);
int fadehip_last_run_profile(fadehip_ctx* ctx, int slot, float* ms4, long* counts6);
int fadehip_stats_allreduce(fadehip_ctx** ctxs, int n_ctx, long* counters, int count);
/// one process per GPU: rank 0 writes the RCCL id to id_path, the others read it (fadehip.h)
int fadehip_stats_allreduce_rank(fadehip_ctx* ctx, int rank, int n_ranks, const(char)* id_path, long* counters, int count);

/// BGZF members made on the device (htslib bgzf_write's deflate under util.d:65-76); lane 0 or 1
enum FADEHIP_BGZF_BLOCK = 0xff00;
enum FADEHIP_BGZF_LANES = 2;
int fadehip_bgzf_deflate_submit(fadehip_ctx* ctx, int lane, const(void)* src, size_t n_bytes);
int fadehip_bgzf_deflate_wait(fadehip_ctx* ctx, int lane, const(ubyte)** out_, size_t* out_bytes);
/// whole BGZF members in, their payloads out (one wavefront per member; CRC32 and ISIZE checked)
int fadehip_bgzf_inflate(fadehip_ctx* ctx, const(void)* members, size_t n_bytes, void* out_, size_t out_cap, size_t* out_bytes);

/// The file path on the device: anno.d:44-50 as a byte stream (fadehip.h, "the file path on the device")
struct fadehip_bam_stream;
struct fadehip_bam_config {
    int floor_len;               /// --min-length
    int window;                  /// -w
    int n_ref;                   /// contigs of the BAM header
    int flags;                   /// 1 (FADEHIP_BAM_STORED): uncompressed BGZF out; 2 (FADEHIP_BAM_NO_OUTPUT): back makes no BGZF (measurement); 4 (FADEHIP_BAM_CLIP): hard-clip the artifact calls; 8 (FADEHIP_BAM_EXTRACT): every call also leaves `fade extract`'s records; 16 (FADEHIP_BAM_EJECT): artifact calls are not written; 32 (FADEHIP_BAM_EJECT_GROUPS): nor the records of their name group; 64 (FADEHIP_BAM_FROM_TAGS): rs and am come out of the records (annotated earlier), nothing is aligned
    const(char*)* ref_names;     /// [n_ref]
    uint first_record;           /// payload bytes of the first member passed that precede the first record
    uint tail_trim;              /// payload bytes at the end of the last member that belong to the next reader
}
enum FADEHIP_BAM_CHUNKS = 3;
enum FADEHIP_BAM_STORED = 1;     /// fadehip_bam_config.flags: uncompressed BGZF out (`fade annotate -u`)
enum FADEHIP_BAM_NO_OUTPUT = 2;  /// ... back releases the annotated records without compressing them (measurement)
enum FADEHIP_BAM_EXTRACT = 8;    /// ... every call also builds `fade extract`'s records of its artifact calls (`fade annotate --extract`): fadehip_bam_back_extract
enum FADEHIP_BAM_EJECT = 16;     /// ... artifact calls are not written (`fade annotate --eject`, input not name-sorted), by this run's rs; not with FADEHIP_BAM_CLIP
enum FADEHIP_BAM_EJECT_GROUPS = 32;  /// ... name-sorted input: nor any record of an artifact call's name group (implies FADEHIP_BAM_EJECT); a group never lies across two calls
enum FADEHIP_BAM_FROM_TAGS = 64;  /// ... the records were annotated earlier: rs and am are read back out of them on the device and CLIP / EJECT / EJECT_GROUPS / EXTRACT are `fade out -c` / `fade out` / `fade extract`; no genome, floor_len and window ignored; a needed am side that is not well-formed fails the call at its back (FADEHIP_E_INVALID, the record's index in fadehip_last_error)
enum FADEHIP_BAM_COLLECT_NAMES = 128;  /// ... with FROM_TAGS: every record with an integer rs and rs & 6 adds its name to the attached set
enum FADEHIP_BAM_EJECT_NAMED = 256;    /// ... with FROM_TAGS: a record is written exactly when its name is not in the attached set (both: with STORED / NO_OUTPUT only)
enum FADEHIP_BAM_KEEP_SORTED = 512;    /// ... with CLIP (beside it STORED, EXTRACT, FROM_TAGS only), coordinate-sorted input: the records leave in stable order by (refID, pos + 1) as unsigned, a held tail staying on the device between calls
enum FADEHIP_BAM_REPORT_STATS = 1024;  /// ... with FROM_TAGS | NO_OUTPUT (beside them STORED only): every call also leaves the rows of `fade stats` over its records (fadehip_bam_back_report); also `which` of fadehip_report_batch
enum FADEHIP_BAM_REPORT_CLIP = 2048;   /// ... the same for `fade stats-clip`; the two may be set together
enum FADEHIP_BAM_COLLECT_MATES = 8192; /// ... with FROM_TAGS | CLIP | NO_OUTPUT (beside them STORED only): every primary paired-end record whose name is in the name set stores its placement as it leaves in the mate set
enum FADEHIP_BAM_FIX_MATES = 16384;    /// ... with FROM_TAGS | CLIP (beside them STORED, KEEP_SORTED, INDEX only): every record's mate fields follow the placement the mate set holds for its mate
enum FADEHIP_BAM_INDEX = 4096;         /// ... beside every flag that writes output: every call also leaves the .bai entries of the records it writes (fadehip_bam_back_index)
enum FADEHIP_BAM_STORE_EXTRACT = 32768;  /// ... with EXTRACT: the calls' extract records go into the attached record store and stay on the device (fadehip_bam_use_recstore); fadehip_bam_back_extract gives 0 bytes and the records added
enum FADEHIP_BAM_CLIP = 4;       /// ... artifact calls leave hard-clipped (`fade annotate -c`), by this run's rs and alignments
int fadehip_bam_open(fadehip_ctx* ctx, const(fadehip_bam_config)* cfg, fadehip_bam_stream** out_);
/// the set of the same ctx a COLLECT_NAMES stream adds to / an EJECT_NAMED stream looks up in; before the first front call
int fadehip_bam_use_nameset(fadehip_bam_stream* st, fadehip_nameset* s);
int fadehip_bam_use_mateset(fadehip_bam_stream* st, fadehip_mateset* s);
int fadehip_bam_mates(fadehip_bam_stream* st, long* n_fixed, long* n_ambiguous);
enum FADEHIP_BAM_CALMD = 262144;  /// ... with FROM_TAGS | CLIP (beside them STORED, FIX_MATES, KEEP_SORTED, INDEX, NO_OUTPUT only), a genome uploaded: NM and MD of every record that leaves hard-clipped are recomputed against it
int fadehip_bam_calmd(fadehip_bam_stream* st, long* n_updated, long* n_skipped);
enum FADEHIP_BAM_STORE_OUTPUT = 131072;  /// ... the calls' OUTPUT records go into the attached record store and stay on the device: sorted and drained there, they are the stream's records in coordinate order as they leave; fadehip_bam_back gives 0 bytes.  With the annotate path, FROM_TAGS, CLIP, EJECT, EJECT_GROUPS, EJECT_NAMED, FIX_MATES only
/// the store of the same ctx a STORE_EXTRACT stream appends its extract records to, or a STORE_OUTPUT stream its output records; before the first front call
int fadehip_bam_use_recstore(fadehip_bam_stream* st, fadehip_recstore* s);
enum FADEHIP_BAM_REPORT_REPEATS = 65536;  /// ... with REPORT_STATS: the stats rows gain read_rpm and art_rpm against the attached set of intervals (fadehip_bam_use_intervals)
/// the sealed set of the same ctx a REPORT_REPEATS stream queries; before the first front call
int fadehip_bam_use_intervals(fadehip_bam_stream* st, fadehip_intervals* s);
int fadehip_bam_prepare(fadehip_bam_stream* st, size_t call_bytes);
int fadehip_bam_front(fadehip_bam_stream* st, const(void)* members, size_t n_bytes, int last);
int fadehip_bam_front_raw(fadehip_bam_stream* st, const(void)* payload, size_t n_bytes, int last);
int fadehip_bam_back(fadehip_bam_stream* st, const(ubyte)** out_, size_t* out_bytes);
/// FADEHIP_BAM_EXTRACT: the extract records (uncompressed BAM records, pinned memory) of the call the most recent back finished
int fadehip_bam_back_extract(fadehip_bam_stream* st, const(ubyte)** recs, size_t* n_bytes, long* n_records);
/// With FADEHIP_BAM_REPORT_STATS / _CLIP (which: one of the two): the report's rows of the call the most recent back finished, TSV lines without a header line, in pinned memory
int fadehip_bam_back_report(fadehip_bam_stream* st, int which, const(ubyte)** text, size_t* n_bytes, long* n_rows);
/// With FADEHIP_BAM_INDEX: the .bai entries of the call the most recent back finished, relative to its first member, in pinned memory
int fadehip_bam_back_index(fadehip_bam_stream* st, fadehip_index_call* out_);
/// With FADEHIP_BAM_INDEX, before the first front call: the calls leave the entries of a CSI of that geometry (fadehip_index_batch_csi)
int fadehip_bam_index_geometry(fadehip_bam_stream* st, int min_shift, int depth);
int fadehip_bam_totals(fadehip_bam_stream* st, long* stats8, long* n_records, long* n_oversize);
/// FADEHIP_BAM_EJECT: records not written, over the calls back has taken
int fadehip_bam_ejected(fadehip_bam_stream* st, long* n_ejected);
/// FADEHIP_BAM_KEEP_SORTED: records and bytes held back behind the most recent finished call
int fadehip_bam_held(fadehip_bam_stream* st, long* n_records, long* n_bytes);
void fadehip_bam_close(fadehip_bam_stream* st);
