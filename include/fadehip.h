/*
 * fadehip.h — C ABI of the MI355X (gfx950) `fade annotate` hot path.
 *
 * Drop-in boundary.  The reference (blachlylab/fade) has no plugin API; its hot path is a
 * synchronous per-record FFI seam:
 *     auto p   = Parasail("ACTGN", 10, 2, 2, -3);          source/anno.d:36
 *     auto res = p.sw_striped(q_seq, ref_seq);             source/analysis.d:67
 * inside  annotateTask (source/anno.d:55-110)  <-  foreach(rec; parallel(bam.allRecords))
 * (source/anno.d:44-50).  One call per clip cannot feed a GPU, so this ABI exposes the same
 * contract in two batched forms:
 *
 *   Level 1  fadehip_sw_*        — a batch of (query, reference) strings -> {score, position, cigar}
 *                                   replaces analysis.d:67 (the dparasail/libparasail call).
 *   Level 2  fadehip_annotate_*  — a batch of BAM-native read records against a genome resident
 *                                   in HBM -> rs byte per read + the alignment of every read
 *                                   that was re-aligned.  Replaces the body of annotateTask:
 *                                   anno.d:61-74 (gate, parse_clips, SA), analysis.d:34-64
 *                                   (floor, reverse complement util.d:23-34, window, FASTA fetch),
 *                                   analysis.d:67 (SW), analysis.d:69-83,98-107 (artifact gates),
 *                                   readstatus.d:5-26 (rs).  The caller keeps I/O and formats the
 *                                   am/as/ar/ab strings (analysis.d:84-92,108-118, anno.d:94-107).
 *
 * Plain C: pointers and sizes only.  Every function returns 0 on success or a negative
 * FADEHIP_E_* code and never throws or aborts across the boundary; fadehip_last_error(ctx) returns
 * the message of the calling thread's last failure on that ctx.  A ctx is bound to one device; its slots may be driven
 * by one host thread or by one thread each (create, destroy, genome_upload and sw_batch by one thread while no slot is busy).
 * There is no CPU fallback: without a usable HIP device fadehip_create fails.
 */
#ifndef FADEHIP_H
#define FADEHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FADEHIP_ABI_VERSION 3
#define FADEHIP_MAX_OPS 16   /* ops reported per alignment (FADE rejects > 10, analysis.d:69) */
#define FADEHIP_MAX_QUERY 512 /* longest query of the wave kernels (8 alignments per wavefront) */
#define FADEHIP_MAX_LONG_QUERY 32768 /* longer queries, up to this, take a thread-per-alignment kernel (slow path) */
#define FADEHIP_NUM_SLOTS 4   /* batches in flight per ctx (each slot has its own stream, device buffers and pinned result block) */
/* The CIGAR ops dhtslib's Cigar.alignedLength sums (analysis.d:53,111-113; filter.d:27,61): M, D, N, =, X — bit k set for
 * BAM op code k.  One definition for the gate kernel, the host-side bounds and the tag formatters (the oracle restates it
 * as fo_cigar_aligned_length).  [The dhtslib commit FADE pins is not available here; if its alignedLength also counted I,
 * this constant is the only place to change.] */
#define FADEHIP_REF_CONSUMING_OPS 0x18Du
#define FADEHIP_OP_CONSUMES_REF(op) ((FADEHIP_REF_CONSUMING_OPS >> ((op) & 15u)) & 1u)

enum {
    FADEHIP_OK = 0,
    FADEHIP_E_INVALID = -1,     /* bad argument */
    FADEHIP_E_NODEVICE = -2,    /* no HIP device / wrong architecture */
    FADEHIP_E_HIP = -3,         /* a HIP runtime call failed (message has the HIP error) */
    FADEHIP_E_NOMEM = -4,       /* host or device allocation failed */
    FADEHIP_E_UNSUPPORTED = -5, /* scoring parameters, read or window length outside kernel limits */
    FADEHIP_E_STATE = -6,       /* call out of order (e.g. wait on an idle slot) */
    FADEHIP_E_RESIDUE = -7,     /* FASTA contains a byte this encoding cannot represent ('=') */
    FADEHIP_E_RCCL = -8         /* an RCCL call failed */
};

typedef struct fadehip_ctx fadehip_ctx;

/* Parasail("ACTGN", open, ext, match, mismatch) — anno.d:36.  The alphabet is fixed to
 * A,C,T,G,N + wildcard (every other residue scores 0), as parasail_matrix_create builds it.
 * Accepted: 0 < ext <= open, and 0 <= score + open <= 15 for score in {match, mismatch, 0} (4-bit profile
 * entries).  FADE's 10/2/2/-3 and any match <= 2 run the two-pass path; larger match scores exceed the 16-bit
 * ranges of its score pass and take the single-pass packed kernel (match <= 7) or the int32 kernel: same results,
 * lower rate. */
typedef struct {
    int32_t open;      /* 10: cost of the first gap base */
    int32_t ext;       /* 2 : cost of each further gap base */
    int32_t match;     /* 2 */
    int32_t mismatch;  /* -3 */
    int32_t max_ref_len;   /* longest reference window re-aligned; 0 -> 2^20, which is also the most.  Windows of up to 32,000
                              columns take the 16-lane wave kernels (8 alignments per wavefront; the window streams through LDS in
                              chunks), up to 65,000 — and reads of 513 .. 4,096 bases — the one-alignment-per-wavefront kernel,
                              beyond that the thread-per-alignment kernel (slow path); a read whose window is longer than
                              max_ref_len is left un-re-aligned and counted in n_oversize */
    int32_t max_batch_reads; /* capacity of one annotate batch; 0 -> 1<<20 */
    int64_t trace_bytes;   /* device bytes reserved for trace tables / checkpoints; 0 -> sized on demand */
    int32_t trace_all;     /* 1: level 2 returns a CIGAR for every re-aligned read (default: only for reads whose
                              score and end cell can still pass FADE's gates; the others have sw.n_ops == 0) */
    uint32_t rules;        /* FADEHIP_RULE_* bits; 0 -> FADEHIP_RULES_DEFAULT */
} fadehip_params;

/* Behaviour of the un-vendored arithmetic behind analysis.d:67 (libparasail 2.4.3 through dparasail 0.3.3) that could
 * not be checked against its source in this environment (DESIGN.md "parity unpinned").  Each
 * assumption is a switch with the same meaning and bit as oracle/fade_oracle.h's FO_RULE_*: should a maintainer find
 * that parasail does the opposite, it is a parameter, not a kernel edit.  Non-default settings run a slower variant of
 * the traced re-computation; the default costs nothing.  With END_MIN_REF_THEN_QUERY, HDIR_DIAG_F_E or GAP_TIE_EXTENDS
 * off, reads beyond 512 bases and windows beyond 32,000 columns all take the thread-per-alignment kernel (the
 * one-alignment-per-wavefront kernel carries the default of those three only). */
enum {
    FADEHIP_RULE_END_MIN_REF_THEN_QUERY = 1u << 0, /* A.3 end cell: max H, ties -> smallest ref index, then smallest query index (off: first in row-major order) */
    FADEHIP_RULE_HDIR_DIAG_F_E = 1u << 1,          /* A.4 traceback priority DIAG > F (query-only) > E (ref-only)  (off: DIAG > E > F) */
    FADEHIP_RULE_GAP_TIE_EXTENDS = 1u << 2,        /* A.4 a gap "opens" only on strict >, ties extend  (off: ties open) */
    FADEHIP_RULE_EQ_BY_CHAR = 1u << 3,             /* A.4 '=' vs 'X' by residue equality  (off: by the sign of the matrix entry) */
    FADEHIP_RULE_SAM_GAP_LETTERS = 1u << 4,        /* A.5 ref-only step 'D', query-only step 'I'  (off: swapped) */
    FADEHIP_RULE_PAD_SOFTCLIP = 1u << 5,           /* A.6 CIGAR padded with S for unaligned query ends  (off: no padding) */
    FADEHIP_RULE_N_MATCHES_N = 1u << 6,            /* A.1 N vs N scores `match`  (off: `mismatch`) */
    FADEHIP_RULES_DEFAULT = 0x7f
};

void fadehip_params_default(fadehip_params *p);
int fadehip_abi_version(void);

/* device < 0 -> current device.  Fails with FADEHIP_E_NODEVICE when no gfx950 device exists. */
int fadehip_create(fadehip_ctx **out, int device, const fadehip_params *params);
void fadehip_destroy(fadehip_ctx *ctx);
const char *fadehip_last_error(const fadehip_ctx *ctx); /* never NULL; ctx may be NULL */

/* Pinned host memory so that submit can use hipMemcpyAsync.  fadehip_host_register pins memory the caller already has
 * (and may have been filling before the ctx existed: a reader that starts while the device is still being brought up);
 * fadehip_host_free takes the registration back and leaves the memory to the caller. */
int fadehip_host_alloc(fadehip_ctx *ctx, size_t bytes, void **out);
int fadehip_host_free(fadehip_ctx *ctx, void *p);
int fadehip_host_register(fadehip_ctx *ctx, void *p, size_t bytes);

/* ------------------------------------------------------------------ Level 1: the SW seam -- */
/* What FADE reads from a parasail result (analysis.d:69-113): res.score, res.position
 * (= beg_ref), res.cigar (BAM-encoded len<<4|op with "MIDNSHP=X", soft-clip padded). */
typedef struct {
    int32_t score;
    int32_t end_query, end_ref; /* 0-based inclusive end cell */
    int32_t beg_query, beg_ref; /* 0-based; beg_ref is dparasail's `position` */
    int32_t n_ops;              /* true op count; only min(n_ops, FADEHIP_MAX_OPS) stored */
    uint32_t ops[FADEHIP_MAX_OPS];
} fadehip_sw_result;

/* n alignments; strings are ASCII, concatenated, q_off/r_off hold n+1 offsets.  Synchronous. */
int fadehip_sw_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *q, const int64_t *q_off,
                     const uint8_t *r, const int64_t *r_off, fadehip_sw_result *out);

/* What `fade stats` reads from parasail's stats mode (stats.d:123,164): score, 0-based inclusive end cell, and the
 * matches / similar / length of the path that ends in it. */
typedef struct { int32_t score, end_query, end_ref, matches, similar, length; } fadehip_sw_stats_result;
/* stats.d:123,164 — Parasail(alphabet, open, ext, match, mismatch).aligner!("sw","stats","striped","16") over n pairs.
 * Scores come with the call (the ctx's rules apply): open >= 1, ext >= 1 (ext may exceed open), match >= 1,
 * mismatch <= 0, each of magnitude <= 32767; anything else is FADEHIP_E_UNSUPPORTED.  q and r may each hold
 * 0 .. FADEHIP_MAX_LONG_QUERY bases; a pair with an empty string gives all zeros.  Strings and offsets as in
 * fadehip_sw_batch.  Synchronous, on a stream and buffers of its own (calls on one ctx are serialised by a lock): it may
 * be called from any thread while annotate slots are in flight and does not touch their buffers. */
int fadehip_sw_stats_batch(fadehip_ctx *ctx, const int32_t scoring[4] /* open, ext, match, mismatch */, int32_t n,
                           const uint8_t *q, const int64_t *q_off, const uint8_t *r, const int64_t *r_off,
                           fadehip_sw_stats_result *out);

/* filter.d:15-91 clipRead (`fade out -c`) over n BAM records (block_size first, as in a file), concatenated, rec_off holding
 * n + 1 offsets.  Record k is hard-clipped on the left by trim_left[k] reference bases when rs[k] has bit 1 (value 2), then
 * on the right by trim_right[k] reference bases, measured against what the left step left, when it has bit 2 (value 4): the
 * query bases that go become H ops, pos moves with the left clip, bin follows the new span; a length that is not below the
 * aligned length resets the record (a zero-filled one that keeps its name and the bases and qualities trimmed so far, no
 * CIGAR, no aux).  Every other record and all aux bytes pass unchanged.  The clipped records go to out back to back,
 * out_off receives n + 1 offsets; out must hold them (a record grows by at most eight bytes).  The device function is the one
 * the file path runs under FADEHIP_BAM_CLIP; there rs and the lengths are the run's own results.  A record whose
 * block_size, l_read_name, n_cigar_op and l_seq do not fit its bytes: FADEHIP_E_INVALID, with its index in
 * fadehip_last_error.  Synchronous, and apart from the annotate slots as fadehip_sw_stats_batch is; fadehip_clip_batch,
 * fadehip_extract_batch, fadehip_eject_batch and fadehip_tags_batch share one stream, one set of buffers and one lock per
 * ctx: calls of any of them on one ctx, from whichever threads, run one after the other. */
int fadehip_clip_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                       const int32_t *trim_left, const int32_t *trim_right, uint8_t *out, int64_t out_cap, int64_t *out_off);

/* fadehip_clip_batch, then NM and MD follow the clip: a hard clip takes reference bases off the aligned part of a read, so the
 * NM and MD a record came in with describe an alignment that no longer exists.  Every record is written as fadehip_clip_batch
 * writes it (same out / out_off shapes); then a record that leaves hard-clipped (not reset, not unclipped) and carries an
 * MD:Z field or an NM field of an integer type (c C s S i I) gets the two recomputed against the uploaded genome
 * (fadehip_genome_upload / _upload_fasta; none: FADEHIP_E_STATE) from the record as it leaves — refID, the new pos, the new
 * CIGAR, the surviving bases:
 *   subject   flag 0x4 clear, 0 <= refID < contigs, pos >= 0, at least one base left, the leaving CIGAR's query bases
 *             (M I S = X) equal to the bases left, and pos + its reference bases (M D N = X) within the contig.  A record
 *             that is not keeps its aux bytes: updated[k] = 2 (skipped).
 *   walk      over M / = / X a base matches when the read's 4-bit code is 0 ('='), or equals the genome's and is not 15 (N);
 *             a mismatch writes the run of matches in front of it and the genome's letter ("=ACMGRSVTWYHKDBN"[code], what
 *             fadehip_genome_fetch prints) and counts 1 into NM; a D op writes the run, '^' and its reference letters and
 *             counts its length (every D op its own number and caret); an I op counts its length; N, S, H and P write and
 *             count nothing, and do not end a run; the text ends with the last run.
 *   tags      the first MD:Z field's value is replaced where it stands; the first integer NM field is replaced where it stands
 *             by the value as C, S or I, the smallest that holds it.  NM:Z, MD:i, later duplicates and every other byte stay;
 *             a missing field is not added.  The walk over the aux area ends at a field that is not whole.  updated[k] = 1.
 * Every other record: updated[k] = 0, its bytes those of fadehip_clip_batch.  An output of more than out_cap bytes:
 * FADEHIP_E_INVALID with the number needed in fadehip_last_error, and nothing is written to out, out_off or updated.  The
 * device functions are the ones the file path runs under FADEHIP_BAM_CALMD.  Checks, stream, buffers and lock as
 * fadehip_clip_batch.  tests/calmd_model.py states the rule in plain Python; no byte equality with `samtools calmd` is claimed. */
int fadehip_calmd_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                        const int32_t *trim_left, const int32_t *trim_right, uint8_t *out, int64_t out_cap, int64_t *out_off,
                        uint8_t *updated /* [n] out: 0 untouched, 1 updated, 2 skipped */);

/* remap.d:11-87 (`fade extract`) over n BAM records (block_size first, as in a file), concatenated, rec_off holding n + 1
 * offsets.  Side 2k is the left side of record k and is built when rs[k] has bit 1 (value 2), side 2k + 1 the right one, built
 * when it has bit 2 (value 4): a new mapped record on contig art_tid[s] at the 0-based art_pos[s] with the CIGAR ops
 * cig[cig_off[s] .. cig_off[s + 1]) (BAM-encoded), the read's name, its bases reverse-complemented and its qualities
 * reversed, flag 0x10 exactly when the read has it clear, mapq 0, mate refID 0, mate pos 0, tlen 0, bin over the new span,
 * no aux.  The entries of a side whose bit is clear are ignored, and out_off[s + 1] == out_off[s] there.  The records go
 * to out back to back, left before right, in input order; out_off receives 2n + 1 offsets.  A side takes
 * 36 + l_read_name + 4 n_ops + (l_seq + 1) / 2 + l_seq bytes; more than out_cap in all is FADEHIP_E_INVALID and nothing is
 * written.  The CIGAR's query length is not held against l_seq (`fade extract` does not either).  The device function is
 * the one the file path runs under FADEHIP_BAM_EXTRACT; there the fields are the run's own results.  A record whose
 * block_size, l_read_name, n_cigar_op and l_seq do not fit its bytes, or a built side whose CIGAR offsets step backwards:
 * FADEHIP_E_INVALID, with the record's index in fadehip_last_error.  Synchronous, on the stream and buffers it shares with
 * fadehip_clip_batch (see there). */
int fadehip_extract_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                          const int32_t *art_tid /* [2n] */, const int64_t *art_pos /* [2n] */, const int64_t *cig_off /* [2n + 1] */,
                          const uint32_t *cig, uint8_t *out, int64_t out_cap, int64_t *out_off /* [2n + 1] */);

/* filter.d:209-265 (plain `fade out`) over n BAM records (block_size first, as in a file), concatenated, rec_off holding
 * n + 1 offsets: keep[k] = 1 when record k would be written, 0 when it is ejected.  grouped == 0: a record is ejected when
 * rs[k] & 6.  grouped != 0: the records are taken as name-sorted — maximal runs of consecutive records with equal names
 * (l_read_name and every name byte) are groups, and a group is ejected as a whole when one of its records has rs & 6; the
 * work per record does not grow with a group's length.  Whether a file is name-sorted is the caller's to decide (`fade out`
 * looks at its first ten records).  The kernels are the ones the file path runs under FADEHIP_BAM_EJECT /
 * FADEHIP_BAM_EJECT_GROUPS; there rs is the run's own result.  A record whose block_size or l_read_name does not fit its
 * bytes: FADEHIP_E_INVALID, with the record's index in fadehip_last_error.  Synchronous, on the stream and buffers it shares
 * with fadehip_clip_batch (see there). */
int fadehip_eject_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                        int grouped, uint8_t *keep /* [n] out */);

/* rs and am read back out of n BAM records (block_size first, as in a file), concatenated, rec_off holding n + 1 offsets:
 * what `fade extract` and `fade out` parse from a file annotated earlier (remap.d:31-50, filter.d:24-25,58-59,190-196), in
 * the shapes fadehip_clip_batch, fadehip_eject_batch and fadehip_extract_batch take, so that the calls compose without glue.
 * The first aux field named rs and the first named am count (bam_aux_get's rule).
 *   have[k] bit 0: the rs field is an integer (c C s S i I); rs[k] is then the low byte of its value (tag.to!ubyte), else
 *     0 — an rs of any other type counts as absent.  Bit 1: the am field has type Z.
 *   am is "left;right", cut at its first ';' (without one the whole string is the left side and the right side is empty).
 *     have[k] bit 2 (left) / bit 3 (right): the side is well-formed, "name,pos,cigar" — name up to the first comma (may be
 *     empty), pos what std.conv.to!long accepts (an optional sign, digits, nothing else, a value of 64 bits), cigar zero or
 *     more pairs of a count (digits, below 2^28) and a letter of MIDNSHP=XB, and nothing behind it.
 *   For a well-formed side s = 2k + side: art_tid[s] is the first contig of ref_names whose name equals name byte for
 *     byte, or -1 (also for an empty name); art_pos[s] the position; cig[cig_off[s] .. cig_off[s + 1]) its ops,
 *     BAM-encoded, as many as the text holds (FADEHIP_MAX_OPS does not apply); trim_left[k] / trim_right[k] the reference
 *     bases the left / right side's ops take (FADEHIP_OP_CONSUMES_REF), at most INT32_MAX.
 *   Any other side: art_tid -1, art_pos 0, no ops, trim 0.  A malformed am is never an error here; whether it matters is the
 *     consumer's to decide.
 * cig_off receives 2n + 1 offsets.  More ops than cig_cap: FADEHIP_E_INVALID, the number needed is in fadehip_last_error
 * and nothing is written.  A record whose block_size, l_read_name, n_cigar_op and l_seq do not fit its bytes, or whose aux
 * area is not whole fields: FADEHIP_E_INVALID, with the record's index in fadehip_last_error.  ref_names (n_ref C strings,
 * the header's contigs) go up with every call.  Synchronous, on the stream and buffers it shares with fadehip_clip_batch
 * (see there). */
int fadehip_tags_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t n_ref,
                       const char *const *ref_names, uint8_t *rs /* [n] */, uint8_t *have /* [n] */, int32_t *trim_left /* [n] */,
                       int32_t *trim_right /* [n] */, int32_t *art_tid /* [2n] */, int64_t *art_pos /* [2n] */,
                       int64_t *cig_off /* [2n + 1] */, uint32_t *cig, int64_t cig_cap);

/* The rows of `fade stats` (stats.d:75-186; which = FADEHIP_BAM_REPORT_STATS) or `fade stats-clip` (noclip.d:17-73; which =
 * FADEHIP_BAM_REPORT_CLIP) over n BAM records that were annotated earlier (shapes and ref_names as fadehip_tags_batch takes),
 * as TSV text without the header line, written on the device.  Slot 2k is the left side of record k, slot 2k + 1 its right
 * side; row_off receives 2n + 1 offsets into out, a slot without a row taking no bytes, so the rows stand in input order,
 * left before right.  rs counts only as an integer field, the first of its name, by its low byte.
 *   stats: a record takes part with an integer rs, rs & 6 and an am:Z (any other record is skipped); one row of 21 columns
 *     per set bit.  art_start / art_end come from the first (left) or last (right) S op anywhere in the CIGAR and the
 *     aligned length; the am side is "name,pos,cigar" as fadehip_tags_batch has it, cut at am's first ';', pos within
 *     int32, aln_end = pos + the reference bases of the side's CIGAR; as / ar are cut at ';' (piece 0 left, piece 1 right),
 *     ab's first (left) or last (right) bytes, as many as the as piece has, are the side's qualities; the predicted repeat
 *     is the as piece up to the end of parasail's sw_stats alignment {3, 8, 10, -5} (under the ctx's rules) of its first
 *     round(0.75 length) bytes against the ar piece.  The call fails with FADEHIP_E_INVALID and the record's index in
 *     fadehip_last_error where the reference would die of a range or conversion error: a needed am side that is not
 *     well-formed or whose pos is outside int32; as / ar / ab absent or not Z; no piece 1 where the right side is needed; an
 *     empty as piece; ab shorter than the piece; no S op; refID outside ref_names.  A piece longer than
 *     FADEHIP_MAX_LONG_QUERY: FADEHIP_E_UNSUPPORTED.
 *   stats-clip: a record takes part with an integer rs and rs & 1; one row of 6 columns per clip parse_clips finds (util.d:
 *     37-62, with its quirk: leading S ops all count as the left clip, the last one wins).  Qualities + 33 in byte
 *     arithmetic (0xff gives a space), bases from =ACMGRSVTWYHKDBN.  FADEHIP_E_INVALID with the record's index: a clip on a
 *     record with l_seq 0, or one longer than l_seq.
 * The float columns are "%g" of float(num) / float(den): nan, inf, else six significant digits.  A record whose fields do not
 * fit its bytes or whose aux area is not whole fields: FADEHIP_E_INVALID with its index.  More than out_cap bytes:
 * FADEHIP_E_INVALID, the number needed is in fadehip_last_error; a call that fails writes nothing.  Synchronous, on the stream
 * and buffers it shares with fadehip_clip_batch (see there).  (The two constants are fadehip_bam_config.flags bits, defined
 * with them below: there they ask the file path for the same rows.) */
int fadehip_report_batch(fadehip_ctx *ctx, int32_t which, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t n_ref,
                         const char *const *ref_names, uint8_t *out, int64_t out_cap, int64_t *row_off /* [2n + 1] */);

/* The stable coordinate order of n BAM records (shapes as fadehip_eject_batch takes), whatever order they come in: the key
 * of a record is (refID as uint32, pos + 1 as uint32) compared as one 64-bit number — refID -1 sorts last, as in samtools —
 * and records of one key keep the order they came in.  order[j] is the index of the record that comes j-th.  The sort is
 * the one of the file path under FADEHIP_BAM_KEEP_SORTED; it also puts fadehip_clip_batch's output in order.  NULL
 * arguments: FADEHIP_E_INVALID before any device call; n = 0 is fine.  A malformed record: FADEHIP_E_INVALID with its
 * index.  Synchronous, on the stream and buffers it shares with fadehip_clip_batch (see there). */
int fadehip_coord_order_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t *order /* [n] */);

/* The BAM index (.bai, SAM specification 5.2) of coordinate-sorted records, built where they are written.
 * The rule, which tests/bai_model.py states in Python:
 *   span     beg = max(pos, 0), end = beg + max(reflen, 1); reflen over FADEHIP_REF_CONSUMING_OPS, 0 for a record with flag 4;
 *            bin = reg2bin(beg, end), never the record's bin field.  refID >= 0 with end > 2^29: FADEHIP_E_UNSUPPORTED (BAI
 *            cannot hold it), fadehip_last_error names the record
 *   order    the key (refID as uint32, pos + 1 as uint32) must not decrease: else FADEHIP_E_INVALID, naming the record
 *   chunks   every maximal run of consecutive records of one (refID >= 0, bin): (offset of its first record, offset behind
 *            its last)
 *   linear   per record with flag 4 clear, the 16 kb windows beg >> 14 .. (end - 1) >> 14 that no earlier such record of its
 *            refID in the call reaches: (refID, window, the record's offset)
 *   refs     every maximal run of one refID, -1 included: its first offset, the offset behind it, its records by flag 4
 * Offsets are BGZF virtual offsets relative to the call: fadehip_bai_add rebases them.  The arrays are dense and in stream
 * order.  htslib's folding of sparse deep bins into their parents is not done; byte equality with `samtools index` is not
 * claimed. */
typedef struct { int32_t tid; uint32_t bin; uint64_t beg, end; } fadehip_index_chunk;
typedef struct { int32_t tid; uint32_t window; uint64_t off; } fadehip_index_linear;
typedef struct { int32_t tid; int32_t reserved; uint64_t off_beg, off_end, n_mapped, n_unmapped; } fadehip_index_ref;
typedef struct {
    const fadehip_index_chunk *chunks;
    const fadehip_index_linear *linear;
    const fadehip_index_ref *refs;
    int64_t n_chunks, n_linear, n_refs;
    int64_t n_records;               /* records the call wrote */
    uint64_t first_key, last_key;    /* of its first and last record (0 without records) */
} fadehip_index_call;

/* The index entries of n BAM records the caller brings (shapes as fadehip_eject_batch takes; n_cigar_op must fit too) with
 * virtual offsets the caller brings: voff[k] is where record k starts, voff[k + 1] where it ends.  The kernels are the ones
 * the file path runs under FADEHIP_BAM_INDEX.  *out points into memory of the ctx, good until the next record-batch call on
 * it.  NULL arguments: FADEHIP_E_INVALID before any device call; n = 0 gives empty arrays.  Synchronous, on the stream and
 * buffers it shares with fadehip_clip_batch (see there). */
int fadehip_index_batch(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint64_t *voff /* [n + 1] */,
                        fadehip_index_call *out);

/* The same entries under a CSI geometry (min_shift, depth) — what `samtools index -c` answers BAI's 2^29 with (DESIGN.md
 * 3.8p; tests/csi_model.py states the rule in Python).  4 <= min_shift, 1 <= depth <= 8, min_shift + 3 * depth <= 32, else
 * FADEHIP_E_INVALID before any device call; limit = 2^(min_shift + 3 * depth).
 *   bins     level l = 0 (the root) .. depth has 8^l bins of 2^(min_shift + 3 (depth - l)) positions, numbered from
 *            (8^l - 1) / 7; a record's bin is the deepest one that holds [beg, end).  (14, 5) gives fadehip_index_batch's arrays
 *   span     refID >= 0 with end > limit: FADEHIP_E_UNSUPPORTED; fadehip_last_error names the record, the limit as a power of
 *            two and "CSI"
 *   linear   windows of 2^min_shift positions.  A CSI file holds no linear index: fadehip_csi_finish derives every bin's
 *            loffset from the entries
 * Order, chunks, refs, offsets and the lifetime of *out are fadehip_index_batch's; so are all kernels but the first, which
 * has a second form that takes the geometry. */
int fadehip_index_batch_csi(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint64_t *voff /* [n + 1] */,
                            int32_t min_shift, int32_t depth, fadehip_index_call *out);

/* The host's part: a .bai out of the calls' entries, in stream order.  No device is involved (a NULL builder or argument:
 * FADEHIP_E_INVALID; fadehip_bai_error has the message).
 *   add     offsets + (base_file_offset << 16); chunks, first-writer-wins linear entries and reference runs appended per
 *           reference; first_key below the previous call's last_key: FADEHIP_E_INVALID (the builder is left unchanged)
 *   finish  within a bin, in file order, a chunk merges into the one before when prev.end >> 16 >= next.beg >> 16; a window
 *           without an entry takes the next higher window's; pseudo-bin 37450 per reference with records; n_no_coor.
 *           *bytes is the builder's, good until it is destroyed or added to */
typedef struct fadehip_bai fadehip_bai;
fadehip_bai *fadehip_bai_create(int32_t n_ref);
int fadehip_bai_add(fadehip_bai *b, uint64_t base_file_offset, const fadehip_index_call *call);
int fadehip_bai_finish(fadehip_bai *b, const uint8_t **bytes, size_t *n);
const char *fadehip_bai_error(const fadehip_bai *b); /* never NULL; b may be NULL */
void fadehip_bai_destroy(fadehip_bai *b);

/* ... and a .csi (CSI version 1) out of entries made under the same geometry.  create: NULL for a negative n_ref or a geometry
 * that is not valid.  add is fadehip_bai_add's (bins up to the geometry's last, windows below 8^depth).
 *   finish  chunks merge as a .bai's; bins in ascending number, each with its loffset: the linear entries back-filled (a window
 *           without an entry takes the next higher window's value), read at the bin's first window — the k-th bin of level l
 *           begins at window k << 3 (depth - l) —, 0 when that window lies behind the last one with a value; behind the bins the
 *           pseudo-bin ((1 << (3 * depth + 3)) - 1) / 7 + 1 with loffset 0 and fadehip_bai_finish's two chunks; n_no_coor.
 *           *payload is UNCOMPRESSED: "CSI\1", min_shift, depth, l_aux = 0, n_ref, the references, n_no_coor.  The file is the
 *           payload in BGZF members followed by the end-of-file marker, which is the writer's to do.  *payload is the
 *           builder's, good until it is destroyed or added to
 * htslib's choice of a depth and its folding of bins are not reproduced; byte equality with `samtools index -c` is not claimed. */
typedef struct fadehip_csi fadehip_csi;
fadehip_csi *fadehip_csi_create(int32_t n_ref, int32_t min_shift, int32_t depth);
int fadehip_csi_add(fadehip_csi *b, uint64_t base_file_offset, const fadehip_index_call *call);
int fadehip_csi_finish(fadehip_csi *b, const uint8_t **payload, size_t *n);
const char *fadehip_csi_error(const fadehip_csi *b); /* never NULL; b may be NULL */
void fadehip_csi_destroy(fadehip_csi *b);

/* A set of read names, resident on the device: what lets `fade out --fragments` eject whole fragments — the artifact read,
 * its mate, its supplementary and secondary lines — from input in any order, without a sort by name in front and a second
 * one behind.  Records have the shapes fadehip_eject_batch takes.  Two names are equal when l_read_name and every name byte
 * are; the set is exact (a hash decides where to look, never whether two names are equal) and grows as names are added.
 *   add_batch       the names of the records with pick[k] != 0 go into the set (pick NULL: every record); a name that is
 *                   there already is not added again
 *   contains_batch  hit[k] = 1 when record k's name is in the set, else 0
 *   count           distinct names in the set (waits for whatever of the set is still running on the device)
 * The two batch calls are synchronous, on the stream, the buffers and the lock they share with fadehip_clip_batch (see
 * there); a file path may use the set at the same time (fadehip_bam_use_nameset).  A record whose block_size or
 * l_read_name does not fit its bytes: FADEHIP_E_INVALID, with the record's index in fadehip_last_error, and the set is left
 * as it was before the call.  A NULL set or NULL arrays: FADEHIP_E_INVALID before anything reaches the device.  destroy
 * comes after every stream that uses the set has been closed, and before fadehip_destroy.
 * Environment, read at create: FADEHIP_NAMESET_SLOTS=N, the first table's size (default 65536, at least 16, rounded up to a
 * power of two); FADEHIP_NAMESET_HASH_BITS=N, 0 .. 64 (default 64): the hash is cut to its low N bits before any use — with
 * 0 every name collides with every other.  Results depend on neither. */
typedef struct fadehip_nameset fadehip_nameset;
int fadehip_nameset_create(fadehip_ctx *ctx, fadehip_nameset **out);
int fadehip_nameset_add_batch(fadehip_nameset *s, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *pick /* [n] or NULL */);
int fadehip_nameset_contains_batch(fadehip_nameset *s, int32_t n, const uint8_t *recs, const int64_t *rec_off, uint8_t *hit /* [n] out */);
int fadehip_nameset_count(fadehip_nameset *s, int64_t *n_names);
void fadehip_nameset_destroy(fadehip_nameset *s);

/* A map, resident on the device, from (read name, segment) to where that record ends up once `fade out -c` has clipped
 * it — and the call that lets every record's mate fields follow: after a hard clip the mate's next_pos, tlen, flag 0x20 and
 * MC:Z describe a record that no longer exists, and the mate of a reset record points at nothing.
 * A record is paired-end when flag & 0x1 is set and exactly one of 0x40 / 0x80 is; its key is l_read_name, the name bytes
 * and flag & 0xC0; its mate's key is the same name with the other segment.  "As it leaves" is the record as
 * fadehip_clip_batch writes it for the same rs, trim_left and trim_right.
 *   add_batch   every primary (flag & 0x900 == 0) paired-end record with pick[k] != 0 (pick NULL: every such record)
 *               stores its placement as it leaves under its key: reset / unmapped / mapped, refID, pos, strand, the 5' end
 *               (pos, or for a reverse record pos + max(1, reference bases of the leaving CIGAR) - 1) and the leaving
 *               CIGAR as SAM text.  A second insert under a key the map holds marks the entry ambiguous, whatever the two
 *               placements are and whichever came first.
 *   fix_batch   writes every record as fadehip_clip_batch does (same out / out_off shapes); then a record that leaves
 *               paired-end and whose mate's key is in the map and not ambiguous gets its mate fields from the mate's
 *               placement V — V reset: flag |= 0x8, flag &= ~0x22, next_refID / next_pos its own refID / pos, tlen 0, the
 *               first MC:Z field removed; otherwise next_refID / next_pos V's, 0x20 V's strand, 0x8 exactly when V is
 *               unmapped, tlen 0 when either is unmapped, a refID is negative or the two differ, else with
 *               d = V's 5' end - its own: d + 1 when d >= 0, d - 1 otherwise; the value of the first MC:Z field replaced in
 *               place by V's CIGAR text (the field removed when V is unmapped or has no ops; none is added; an MC of
 *               another type and a second MC:Z stay).  Its own refID, pos, bin, mapq and every other aux byte never
 *               change.  fixed[k]: 0 untouched, 1 fixed, 2 the mate's key is ambiguous (the record leaves as
 *               fadehip_clip_batch writes it).  An output of more than out_cap bytes: FADEHIP_E_INVALID with the number
 *               needed in fadehip_last_error, and nothing is written to out, out_off or fixed.
 *   count       keys in the map, and how many of them are ambiguous.
 * The calls are synchronous, on the stream, the buffers and the lock they share with fadehip_clip_batch.  A malformed
 * record (block_size, l_read_name, n_cigar_op, l_seq against its bytes) or a negative trim: FADEHIP_E_INVALID with the
 * record's index, the map left as it was.  A NULL map or NULL arrays: FADEHIP_E_INVALID before anything reaches the device.
 * Environment, read at create: FADEHIP_MATESET_SLOTS and FADEHIP_MATESET_HASH_BITS, as the name set's two.  Results depend
 * on neither.  tests/mates_model.py states the rule in plain Python. */
typedef struct fadehip_mateset fadehip_mateset;
int fadehip_mateset_create(fadehip_ctx *ctx, fadehip_mateset **out);
int fadehip_mateset_add_batch(fadehip_mateset *s, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                              const int32_t *trim_left, const int32_t *trim_right, const uint8_t *pick /* [n] or NULL */);
int fadehip_mates_fix_batch(fadehip_mateset *s, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *rs,
                            const int32_t *trim_left, const int32_t *trim_right, uint8_t *out, int64_t out_cap,
                            int64_t *out_off /* [n + 1] out */, uint8_t *fixed /* [n] out */);
int fadehip_mateset_count(fadehip_mateset *s, int64_t *n_entries, int64_t *n_ambiguous);
void fadehip_mateset_destroy(fadehip_mateset *s);

/* A store of BAM records, resident on the device: what lets `fade extract --sorted` and `fade annotate --extract-sorted`
 * write their extract records in coordinate order with a .bai, without a `samtools sort` and `samtools index` behind them.
 * An extract record lies at its artifact alignment, so the output order has nothing to do with the input's: the store
 * collects the records of a whole run, sorts them once, and hands them out in order (tests/recstore_model.py
 * states the rule in plain Python).
 *   add_batch  the records with pick[k] != 0 (pick NULL: every record) are appended, in the order they come; shapes as
 *              fadehip_eject_batch takes (n_cigar_op and l_seq must fit too).  A malformed record: FADEHIP_E_INVALID with
 *              its index, the store left as it was.  A stream opened with FADEHIP_BAM_STORE_EXTRACT appends its calls'
 *              extract records to the same store, call by call in stream order.
 *   count      records and their bytes, as added so far
 *   sort       closes the store for adding (a later add, or a stream that appends: FADEHIP_E_STATE) and puts the records in
 *              the order of fadehip_coord_order_batch: by (refID as uint32) << 32 | (pos + 1 as uint32) — refID -1 last —
 *              and, within one key, in the order they were added.  Waits for whatever still appends on the device.
 *   drain      after sort (before: FADEHIP_E_STATE): hands out the next maximal run of records, in final order, whose bytes
 *              total at most max_payload (and at most 2^30) — always at least one record, never a part of one; *n_records 0:
 *              the store is drained.  flags:
 *                FADEHIP_RECSTORE_RAW     *out: the records back to back, no codec
 *                0                        *out: BGZF members from the device compressor, ready for the file
 *                FADEHIP_RECSTORE_STORED  *out: stored members, as FADEHIP_BAM_STORED makes them
 *                FADEHIP_RECSTORE_INDEX   beside 0 or STORED (with RAW: FADEHIP_E_INVALID): *idx also gets the drained
 *                                         records' index entries, by the rule and the kernels of fadehip_index_batch, at
 *                                         virtual offsets relative to the drain's first member — fadehip_bai_add rebases
 *                                         them as it does a stream's calls.  A record that ends beyond 2^29:
 *                                         FADEHIP_E_UNSUPPORTED naming the record (its number in final order); that drain
 *                                         hands out nothing and the store stays where it was.
 *              *out is pinned memory of the store and *idx points into memory of the store, both good until its next drain.
 * The calls are synchronous; add_batch and sort take the lock fadehip_clip_batch takes, drain uses compressor lane 0 (no
 * stream of the ctx may be using it).  The store grows as records come: the arena and the per-record arrays double, after a
 * wait for the device, with a copy on the device.  A device allocation that fails is FADEHIP_E_NOMEM; more than 2^31 - 1
 * records is FADEHIP_E_UNSUPPORTED.  destroy comes after every stream that uses the store has been closed, and before
 * fadehip_destroy.  Environment, read at create: FADEHIP_RECSTORE_BYTES=N, the first arena's size (default 64 MiB, at least
 * 256).  Results do not depend on it. */
typedef struct fadehip_recstore fadehip_recstore;
#define FADEHIP_RECSTORE_RAW 1
#define FADEHIP_RECSTORE_STORED 2
#define FADEHIP_RECSTORE_INDEX 4
int fadehip_recstore_create(fadehip_ctx *ctx, fadehip_recstore **out);
int fadehip_recstore_add_batch(fadehip_recstore *s, int32_t n, const uint8_t *recs, const int64_t *rec_off, const uint8_t *pick /* [n] or NULL */);
int fadehip_recstore_count(fadehip_recstore *s, int64_t *n_records, int64_t *n_bytes);
int fadehip_recstore_sort(fadehip_recstore *s);
int fadehip_recstore_drain(fadehip_recstore *s, int32_t flags, uint64_t max_payload, const uint8_t **out, size_t *out_bytes, int64_t *n_records,
                           fadehip_index_call *idx /* NULL without FADEHIP_RECSTORE_INDEX */);
/* The entries FADEHIP_RECSTORE_INDEX drains hand out are made under the CSI geometry (fadehip_index_batch_csi) from then on,
 * for fadehip_csi_add; a record beyond the geometry's limit fails the drain as one beyond 2^29 does without.  Before the first
 * drain that hands out records (later: FADEHIP_E_STATE; fadehip_recstore_reset does not open it again); a geometry that is not
 * valid: FADEHIP_E_INVALID.  A store on which it is never called launches the kernels it always has. */
int fadehip_recstore_index_geometry(fadehip_recstore *s, int32_t min_shift, int32_t depth);
void fadehip_recstore_destroy(fadehip_recstore *s);
/* The store behind a coordinate-sorted MAIN output: a stream opened with FADEHIP_BAM_STORE_OUTPUT appends every record it
 * would have written, and a file whose records do not fit the device at once is written in windows of the key space, one pass
 * over the input per window (tests/sorted_out_model.py states the rule in plain Python).  A store on which
 * none of these calls is made behaves as it always has.
 *   set_budget   the most the store may cost: cost = bytes + 64 per record (the item and the sort's arrays).  0: derived from
 *                hipMemGetInfo — two fifths of what is free less 2 GiB — and FADEHIP_RECSTORE_BUDGET=N in the
 *                environment overrides either at the call.  From then on a growth never allocates beyond the budget, and a
 *                call that would take the cost over it fails with FADEHIP_E_NOMEM — unless the store measures.
 *   measure      ref_len[n_ref]: the header's contig lengths.  Builds and zeroes the bucket table: reference r has
 *                ((len[r] + 1) >> 16) + 1 buckets of 65,536 positions, and one more bucket, the last, takes refID -1 and
 *                every refID outside the header.  From then on (until reset) FADEHIP_BAM_STORE_OUTPUT streams add the bytes
 *                and records they write to their buckets, and a call that would take the cost over the budget sends the
 *                store OVER instead of failing: its contents are dropped, later calls store nothing, measuring goes on.
 *   over         *over: 1 when that happened.   histogram: the table — bytes[] and records[] of *n_buckets entries each
 *                (on entry *n_buckets is what the arrays hold; both NULL: only the number is wanted).  Both wait for the device.
 *   set_window   the keys [lo_key, hi_key_inclusive] a FADEHIP_BAM_STORE_OUTPUT stream keeps (keys as sort's); records
 *                outside it are dropped as an ejected record is, and counted apart.  Default: every key.
 *   reset        empties the store, sorted or not, and ends measuring; memory, budget, window and table stay.  The arena
 *                and the item arrays are sized once for `bytes` and `records`, so that a window's pass never grows.
 * set_budget, measure and set_window take an EMPTY, unsorted store (else FADEHIP_E_STATE); measure comes once; histogram
 * comes after measure.  NULL arguments: FADEHIP_E_INVALID before any device call. */
int fadehip_recstore_set_budget(fadehip_recstore *s, uint64_t bytes);
int fadehip_recstore_budget(fadehip_recstore *s, uint64_t *bytes); /* the budget in force (derived, given or from the environment); 0: none set */
int fadehip_recstore_measure(fadehip_recstore *s, int32_t n_ref, const int64_t *ref_len);
int fadehip_recstore_over(fadehip_recstore *s, int32_t *over);
/* Reset records — reads a clip left nothing of, written zero-filled (refID 0, pos 0) and sorted last — among what
 * FADEHIP_BAM_STORE_OUTPUT streams have finished since create or reset, inside the window or not.  A file that ends in them
 * is not in coordinate order by its own bytes: no index can be made of it. */
int fadehip_recstore_resets(fadehip_recstore *s, int64_t *n_reset);
int fadehip_recstore_histogram(fadehip_recstore *s, uint64_t *bytes, uint64_t *records, int64_t *n_buckets);
int fadehip_recstore_set_window(fadehip_recstore *s, uint64_t lo_key, uint64_t hi_key_inclusive);
int fadehip_recstore_reset(fadehip_recstore *s, uint64_t bytes, uint64_t records);

/* A set of genomic intervals resident on the device, and the overlap query over it (tests/intervals_model.py
 * states the rule in Python): what `bedtools subtract -A` against a RepeatMasker BED decides, as one look-up per query.
 *   interval  (chrom, start, end): chrom an index into the names the set was created with, start and end 0-based half-open,
 *             0 <= start < end <= 2^31 - 1.  Duplicates and any order are fine.
 *   query     (chrom, qs, qe) of int64, which may be negative: hit = 1 iff qs < qe and the set holds an interval of that
 *             chrom with start < qe and qs < end — any overlap of at least one base.  chrom outside [0, n_chrom): 0.
 *   create    n_chrom names (NUL-terminated, non-empty, compared as exact bytes); a name twice: FADEHIP_E_INVALID.
 *   add       n intervals, any number of calls.  A bad interval — chrom outside the names, or the bounds above — is found on
 *             the device: FADEHIP_E_INVALID, fadehip_last_error names its index in the call, and NOTHING of the call is added.
 *             After seal: FADEHIP_E_STATE.
 *   seal      sorts the intervals by (chrom, start) (the stable radix sort of FADEHIP_BAM_KEEP_SORTED) and leaves per interval
 *             its start and the running maximum of chrom << 32 | end — which the chrom ids, rising along the order, segment
 *             by contig — and every contig's range.  A second seal: FADEHIP_E_STATE.  A set without intervals seals fine.
 *   overlap_batch  n queries, a binary search each (about log2 of the set's size probes).  Before seal: FADEHIP_E_INVALID.
 *   count     the intervals added so far, and the names.
 *   load_bed  create + add in pieces + seal over a BED file: lines end at LF (a CR in front of it is dropped, the last line may
 *             lack its LF); empty lines and lines that start with '#', "track" or "browser" are skipped; fields are separated
 *             by tabs, at least three, further ones ignored; the name is 1 to 255 bytes; start and end are decimal digits
 *             only, within the bounds above; names get their ids in order of first appearance.  Anything else:
 *             FADEHIP_E_INVALID, fadehip_last_error names the 1-based line.  The file is read in pieces and never stands in
 *             memory as text.  A path ending in .gz or .bgz is refused by name (FADEHIP_E_INVALID): plain text only.
 * The calls are synchronous and take the lock fadehip_clip_batch takes.  A sealed set never changes: any number of streams
 * and calls may read it at once.  The raw arrays grow by doubling, with a copy on the device; a device allocation that
 * fails is FADEHIP_E_NOMEM; more than 2^31 - 1 intervals is FADEHIP_E_UNSUPPORTED.  destroy comes after every stream that
 * uses the set has been closed, and before fadehip_destroy.  Environment, read at create: FADEHIP_INTERVALS_CAP=N, the
 * intervals the first arrays hold (default 1 Mi, at least 16).  Results do not depend on it. */
typedef struct fadehip_intervals fadehip_intervals;
int fadehip_intervals_create(fadehip_ctx *ctx, int32_t n_chrom, const char *const *chrom_names, fadehip_intervals **out);
int fadehip_intervals_add(fadehip_intervals *s, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end);
int fadehip_intervals_seal(fadehip_intervals *s);
int fadehip_intervals_count(fadehip_intervals *s, int64_t *n_intervals, int32_t *n_chrom);
int fadehip_intervals_overlap_batch(fadehip_intervals *s, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, uint8_t *hit /* [n] */);
int fadehip_intervals_load_bed(fadehip_ctx *ctx, const char *path, fadehip_intervals **out);
void fadehip_intervals_destroy(fadehip_intervals *s);

/* fadehip_report_batch's stats rows (which = FADEHIP_BAM_REPORT_STATS) with a sealed set of intervals: every row keeps its
 * 21 columns byte for byte and gains "\tread_rpm\tart_rpm", each 0 or 1 — read_rpm is the query (rname, art_start, art_end),
 * art_rpm the query (aln_rname, aln_start, aln_end), in exactly the values the row prints.  A contig is matched to the set by
 * its name's bytes: rname through ref_names, aln_rname by its bytes as they stand in am, also when ref_names does not carry
 * that name.  A name the set does not hold hits nothing.  The rule is per row.  A set that is not sealed, or of another ctx:
 * FADEHIP_E_INVALID.  Everything else as fadehip_report_batch. */
int fadehip_report_batch_repeats(fadehip_ctx *ctx, int32_t n, const uint8_t *recs, const int64_t *rec_off, int32_t n_ref, const char *const *ref_names,
                                 fadehip_intervals *intervals, uint8_t *out, int64_t out_cap, int64_t *row_off /* [2n + 1] */);

/* ------------------------------------------------------ Level 2: annotateTask over a batch -- */
/* Upload the indexed FASTA once (what IndexedFastaFile + fetchSequence serve, analysis.d:63).
 * seqs[c] holds lengths[c] ASCII residues (any case; upper-cased on device as analysis.d:63 does).
 * Stored in HBM as 4-bit codes, two bases per byte. */
int fadehip_genome_upload(fadehip_ctx *ctx, int32_t n_contigs, const int64_t *lengths,
                          const uint8_t *const *seqs);

/* The same genome from the FASTA FILE through its .fai index (what IndexedFastaFile is opened on, anno.d:23): the library
 * reads the file itself, straight into two pinned staging chunks (at most 4 reading threads; one chunk fills while the device
 * works on the other), and a kernel turns file bytes into packed bases — the host does work per contig, never per base, and
 * holds two chunks instead of the text.  Contig c of the genome is entries[c] (columns 2-5 of its .fai line), in the caller's
 * order whatever the file's; `length` is the number of bases to take and may be less than the contig holds; entries may
 * overlap or repeat file ranges; length 0 is legal (line_bases may then be 0).  The ctx is left exactly as
 * fadehip_genome_upload leaves it for the same residues (and on failure).  The file is read front to back once, in chunks of
 * 64 MB (FADEHIP_FASTA_CHUNK=bytes, at least 4096, read at every call); copies and launches number file bytes / chunk, not
 * contigs.  An index that does not describe the file — a line terminator, '>' or a control byte where a base should be —
 * is FADEHIP_E_INVALID ("index does not match the FASTA", with the contig index), as is an entry that ends beyond the file
 * (found before anything is enqueued); '=' is FADEHIP_E_RESIDUE.
 * A file that starts with a BGZF member (bgzip) is inflated on the device, .fai offsets being offsets in the uncompressed
 * text (no .gzi: the file is read front to back); CRC32 / ISIZE failures are FADEHIP_E_INVALID, empty members are legal.
 * gzip without BGZF framing is FADEHIP_E_UNSUPPORTED.  Synchronous. */
typedef struct { int64_t length, offset; int32_t line_bases, line_width; } fadehip_fai_entry; /* .fai columns 2-5 */
int fadehip_genome_upload_fasta(fadehip_ctx *ctx, const char *path, int32_t n_contigs, const fadehip_fai_entry *entries);

/* fetchSequence (analysis.d:63) on the uploaded genome: n letters "=ACMGRSVTWYHKDBN"[code] of contig tid from the 0-based
 * start (upper case; a byte outside IUPAC reads as '=').  A device-to-host copy of the packed bytes, unpacked on the host.
 * Synchronous.  A range outside the contig: FADEHIP_E_INVALID; before any upload: FADEHIP_E_STATE. */
int fadehip_genome_fetch(fadehip_ctx *ctx, int32_t tid, int64_t start, int64_t n, uint8_t *out);

/* BAM-native structure-of-arrays view of n records (what annotateTask reads from a bam1_t). */
typedef struct {
    int32_t n_reads;
    const int32_t *tid;        /* [n] core.tid */
    const int32_t *pos;        /* [n] core.pos, 0-based */
    const uint16_t *flag;      /* [n] core.flag */
    const uint8_t *has_sa;     /* [n] 1 iff the record carries an SA aux tag (anno.d:73) */
    const int32_t *l_seq;      /* [n] core.l_qseq */
    const uint32_t *cigar_off; /* [n+1] index of the record's first op in cigar_ops */
    const uint32_t *cigar_ops; /* BAM-encoded ops, all records concatenated */
    const uint32_t *seq_off;   /* [n+1] byte offset of the record's packed sequence */
    const uint8_t *seq_packed; /* BAM 4-bit sequence bytes, each record byte-aligned.  Only mapped records with an S op
                                  are ever read (anno.d:61): the others may have an empty slice, seq_off[i+1] == seq_off[i] */
    /* ABI 2.  anno.d:61-65 gives an unmapped record, or one without an S op, rs = 0 before looking at anything else:
     * a caller may leave such records out of the batch (they need not cross PCIe) and pass their number here; it is
     * added to the read_count of the batch's stats.  rs / read_idx then index the records that were sent. */
    int32_t n_skipped;
    /* Upper bound of cigar.alignedLength (analysis.d:53) over the batch, or 0 if the caller does not know it: the
     * launches of a run are sized from it (window <= bound + 2 * window-size).  With 0 the library scans the CIGARs
     * itself (about 1 ms per 10^5 records on one host thread).  A bound that turns out too small fails the batch at
     * collect (FADEHIP_E_INVALID), it is never trusted for memory safety. */
    int32_t ref_span_bound;
    /* ABI 3.  What a caller that fills its own block knows for free and the library otherwise finds with one pass over
     * the records (about 1 ms per 10^6 records on one host thread): the number of records that carry bases (a non-empty
     * seq_packed slice — only those can be re-aligned) and the shortest / longest l_seq among THOSE.  With
     * n_with_seq > 0 (and ref_span_bound > 0) fadehip_annotate_upload does no per-record host work: the launches and
     * result buffers of the run are sized from these bounds, and cigar_off / seq_off / l_seq are validated by the gate
     * kernel before anything is dereferenced through them.  A bound that turns out wrong (more records with bases than
     * n_with_seq, or one whose l_seq lies outside [l_seq_min, l_seq_max]) fails the batch at results (FADEHIP_E_INVALID);
     * it is never trusted for memory safety.  0 = unknown. */
    int32_t n_with_seq;
    int32_t l_seq_min, l_seq_max;
    int32_t reserved;
} fadehip_read_batch;

/* One pinned block for the nine arrays of a batch, so that upload is ONE hipMemcpyAsync at PCIe speed: allocate
 * fadehip_batch_bytes(...) with fadehip_host_alloc, let fadehip_batch_bind point the arrays into it (canonical order,
 * 256-byte aligned), fill them through the pointers (cigar_off[n] = n_cigar_ops, seq_off[n] = n_seq_bytes).  Arrays
 * laid out any other way are first gathered into the slot's own pinned staging block (one host copy more). */
size_t fadehip_batch_bytes(int32_t n_reads, int64_t n_cigar_ops, int64_t n_seq_bytes);
int fadehip_batch_bind(void *base, int32_t n_reads, int64_t n_cigar_ops, int64_t n_seq_bytes, fadehip_read_batch *b);

/* One entry per read that was re-aligned (clip longer than min-length), in no particular order.
 * sw.score / end_query / end_ref are always set.  Unless params.trace_all, the traceback (beg_*, ops)
 * is only completed when the result can still be an artifact call; otherwise sw.n_ops == 0, beg_* == -1
 * (score or end cell already fail analysis.d:74-80 / 98-104, or the CIGAR has more than 10 ops, which
 * analysis.d:69-70 rejects whatever they are). */
typedef struct {
    int32_t read_idx;
    int32_t art;         /* bit0 art_left, bit1 art_right (analysis.d:82,106) */
    int64_t win_start;   /* `start` of analysis.d:45-51 */
    int32_t win_len;     /* ref_seq.length */
    int32_t clip_left, clip_right; /* parse_clips(rec.cigar) lengths (anno.d:68) */
    int32_t aligned_len; /* rec.cigar.alignedLength (analysis.d:53) */
    fadehip_sw_result sw;
} fadehip_aln;

typedef struct {
    uint8_t *rs;          /* [n_reads] out: ReadStatus.raw per read (anno.d:63,94) */
    fadehip_aln *aln;     /* [aln_cap] out */
    int32_t aln_cap;      /* in: capacity of aln (n_reads is always enough) */
    int32_t n_aln;        /* out */
    int64_t stats[8];     /* out: stats.d:45-54 over this batch: read_count, clipped, sup, art_sup,
                             art, art_mate, aln_l, aln_r */
    int32_t n_oversize;   /* out: soft-clipped reads left un-re-aligned because the read (> FADEHIP_MAX_LONG_QUERY) or its
                             window (> max_ref_len) exceeds the kernels' limits; their rs keeps the sc / sup bits */
    int32_t reserved;
} fadehip_anno_out;

/* Zero-copy form of the results: pointers into the slot's pinned result block, valid until the slot is RUN again. */
typedef struct {
    const uint8_t *rs;        /* [n_reads] */
    const fadehip_aln *aln;   /* [n_aln] */
    int32_t n_reads, n_aln;
    int64_t stats[8];
    int32_t n_oversize;       /* as in fadehip_anno_out */
    int32_t reserved;
} fadehip_anno_view;

/* Asynchronous pipeline, slot in [0, FADEHIP_NUM_SLOTS); one host thread can keep every slot busy:
 *   upload  : ONE hipMemcpyAsync of the batch block (see fadehip_batch_bind) on the slot's copy stream, into the input
 *             buffer the slot's run in flight does not use; returns at once.  Uploading batch k + 1 right after run(k)
 *             takes the H2D off the slot's critical path; the results of run(k) stay valid until run(k + 1)
 *   run     : enqueues gate -> score pass (SW score, end cell, wave snapshots) -> selection of the alignments that can
 *             still be artifact calls -> device-side plan of the traced re-computation -> traced re-computation of
 *             their last steps -> traceback + artifact gates -> D2H of rs / aln / counters into the slot's pinned
 *             result block.  Nothing is read back in between: launches are sized from host-side bounds (read lengths,
 *             ref_span_bound), counts stay on the device, persistent waves draw work from device-side tables.
 *             Returns as soon as everything is enqueued (FADEHIP_KERNEL=pk|int32, the single-pass kernels kept for
 *             A/B runs, still block on the gate's counters).
 *   results : waits for the slot, then hands out views (collect: copies them into the caller's arrays).  Errors the
 *             device found in the batch (bad tid, window beyond max_ref_len, ...) are reported HERE, not by run.  If
 *             the traced re-computation needed more scratch than the slot held, the scratch grows and the batch runs
 *             again inside this call (a warm-up effect; FADEHIP_DEBUG=1 reports it).
 * submit = upload + run.  The batch arrays handed to upload / submit must stay valid and unchanged until the results /
 * collect of the run that consumes them has returned.  floor_len = --min-length (app.d:17), window = --window-size (app.d:18). */
int fadehip_annotate_upload(fadehip_ctx *ctx, int slot, const fadehip_read_batch *batch);
int fadehip_annotate_run(fadehip_ctx *ctx, int slot, int32_t floor_len, int32_t window);
int fadehip_annotate_submit(fadehip_ctx *ctx, int slot, const fadehip_read_batch *batch,
                            int32_t floor_len, int32_t window);
int fadehip_annotate_results(fadehip_ctx *ctx, int slot, fadehip_anno_view *out);
int fadehip_annotate_collect(fadehip_ctx *ctx, int slot, fadehip_anno_out *out);
int fadehip_sync(fadehip_ctx *ctx);

/* Measurement (after results / collect of that run): device time of the last run on `slot`, from hipEvents recorded
 * on the slot's stream around the kernels.  ms[0] gate, ms[1] the dominant kernel (the score pass; the single forward
 * kernel under FADEHIP_KERNEL=pk|int32), ms[2] everything after it up to the artifact gates (selection, plan, traced
 * pass 2, traceback, re-run rounds), ms[3] whole run.  With several slots in flight these are durations on a shared
 * device.  counts[0] alignments, counts[1] DP cells, counts[2] trace scratch bytes of the largest pass-2 plan,
 * counts[3] algorithmic bytes of the dominant kernel as SURVEY.md §8(d) defines them (packed query + packed window +
 * 16 B descriptor + 64 B result slot per alignment), counts[4] bytes of wave snapshots the score pass leaves for
 * pass 2 (the wave's loop-carried state every 128 sweep steps; written only when the slot's previous run sent more than
 * 1/32 of its alignments to pass 2 — 0 otherwise), counts[5] candidates traced by pass 2. */
int fadehip_last_run_profile(fadehip_ctx *ctx, int slot, float ms[4], int64_t counts[6]);

/* ------------------------------------------------------ BGZF compression of the output stream -- */
/* What htslib's bgzf_write + zlib do behind SAMWriter(..., SAMWriterTypes.BAM) (util.d:65-76) for the write at
 * anno.d:47-49: the uncompressed BAM byte stream cut into blocks of FADEHIP_BGZF_BLOCK bytes, each compressed into one
 * BGZF member (SAM spec 4.1: gzip header with the BC subfield, one final dynamic-Huffman or stored DEFLATE block,
 * CRC32, ISIZE).  On the device: one workgroup per block with the block in LDS (hash matching, minimum-redundancy
 * codes, bit packing, CRC-32), then the members packed into one contiguous byte stream — what goes to the file, minus
 * the end-of-file marker, which the caller appends once.  Any inflater reads it (zlib, htslib, samtools).
 *   submit : H2D of src[0, n_bytes) (host memory; pinned memory from fadehip_host_alloc copies at PCIe speed), the
 *            kernels; returns at once.  src must stay unchanged until wait returns.
 *   wait   : the members' bytes in a pinned buffer of the lane, valid until the lane's next submit.
 * Two lanes, each with its own stream: one compresses while the other's result is copied back.
 * A call's input is cut into blocks of FADEHIP_BGZF_BLOCK bytes (htslib's block size; the block fills a CU's LDS), or —
 * while the stream is mostly incompressible (the previous call's ratio above 0.45: packed bases, uniform qualities) —
 * of half that (0x7f00): two blocks then share a CU and the rate is 1.5x, for 0.5 % more output.  Either way the
 * stream stays smaller than zlib -6's over 0xff00-byte blocks (tests/test_gpu_bgzf.py).  FADEHIP_BGZF_GEOM=64|32 pins it. */
#define FADEHIP_BGZF_BLOCK 0xff00
#define FADEHIP_BGZF_LANES 2
int fadehip_bgzf_deflate_submit(fadehip_ctx *ctx, int lane, const void *src, size_t n_bytes);
int fadehip_bgzf_deflate_wait(fadehip_ctx *ctx, int lane, const uint8_t **out, size_t *out_bytes);

/* ------------------------------------------------------ BGZF decompression of the input stream -- */
/* What htslib's bgzf_read + zlib's inflate do under dhtslib's SAMReader for `bam.allRecords` (anno.d:44): whole BGZF
 * members in, their payloads out, in order and contiguous.  On the device: one wavefront per member (a DEFLATE stream
 * decodes serially; a file has tens of thousands of members), tables in LDS, CRC32 and ISIZE of every trailer checked.
 * members[0, n_bytes) must hold whole members only (a reader cuts at member boundaries: BSIZE of the BC subfield);
 * out receives at most out_cap bytes, *out_bytes their number.  Synchronous (H2D, kernel, D2H); the streaming file path
 * (fadehip_bam_*) keeps the bytes on the device instead.  A malformed member or a corrupt stream: FADEHIP_E_INVALID
 * with the member's index and the reason in fadehip_last_error. */
int fadehip_bgzf_inflate(fadehip_ctx *ctx, const void *members, size_t n_bytes, void *out, size_t out_cap, size_t *out_bytes);

/* ------------------------------------------------------ the file path on the device: BGZF in, BGZF out -- */
/* anno.d:44-50 as a byte stream: `foreach(rec; bam.allRecords) { annotateTask(rec); out.write(rec); }` with the reader's
 * inflate, the record framing, annotateTask (the level-2 kernels), the tag updates of anno.d:63,94-107 and the writer's
 * deflate all on the device.  The host reads compressed bytes from the input file and writes compressed bytes to the
 * output file; 1.0 byte in and about as much out cross PCIe per compressed byte of the file, nothing else.
 *
 * The caller parses the BAM header itself (it needs the contig names for fadehip_genome_upload anyway), writes the
 * output's header members itself, and then passes the input's members from the one that holds the first record on
 * (first_record = bytes of that member's payload in front of the first record: the BGZF virtual offset's low 16 bits).
 *   front : whole BGZF members of the input (any number; cut where the caller likes — records may span members and
 *           calls).  Inflates and frames the records that are complete (the tail of a record cut by the end of the call is
 *           kept for the next one), waits ONCE for the device — the buffers of the call are sized from what the framing
 *           found — and returns with the annotate kernels and the tag sizes of the call enqueued.  The input buffer may be
 *           reused when front returns.  Two calls are in flight: call k + 1 is framed while call k is annotated.
 *   back  : finishes the oldest front call (reads its sizes, enqueues the kernel that writes the records with their tags),
 *           compresses what it produced and returns the BGZF members in pinned memory — the kernel packs them there itself —,
 *           valid until the back call AFTER the next (a writer thread may still be writing them while the next call
 *           compresses).  If the call after is through its front half too, its compressor is enqueued before this call's
 *           members are waited for.  Outputs come in input order.  Without a front call waiting: FADEHIP_E_STATE (it never
 *           blocks for one).
 * front and back may run on two threads (one each): while back compresses chunk k, front works on chunks k+1 and k+2; front
 * blocks while FADEHIP_BAM_CHUNKS chunks await back (a single-threaded caller alternates front and back).  A record already
 * carrying rs / am / as / ar / ab is updated the way htslib's bam_aux_update_int / bam_aux_update_str do (first occurrence:
 * an integer rs keeps its slot and takes the unsigned type letter of its size; a string tag is replaced at its position; a
 * tag of the wrong kind — rs:Z, am:i — is left as it is, as htslib's EINVAL leaves it).  Errors (corrupt member, impossible
 * record, input ending inside a record when last != 0) fail the call and every later one; what the device finds in a
 * call's records after front has returned surfaces at the call's back.  fadehip_bam_totals counts the calls back has taken.
 * The genome must have been uploaded (fadehip_genome_upload) by the first front call — unless the stream was opened with
 * FADEHIP_BAM_FROM_TAGS, which needs none; the stream uses the ctx's slots 0 and
 * 1 and both BGZF lanes.
 * fadehip_bam_prepare (optional, before the first front call, typically on a thread of its own beside the caller's start-up):
 * makes what the first calls would otherwise make one after the other — the streams of the second slot and of the
 * compressor, the staging buffers of the members, the buffers of call_bytes inflated bytes — side by side, and pays for
 * the first copy and the first wait of every stream.  The genome may go up meanwhile (fadehip_genome_upload on another
 * thread).  Results do not depend on it. */
typedef struct fadehip_bam_stream fadehip_bam_stream;
typedef struct fadehip_bam_config {
    int32_t floor_len;            /* --min-length (anno.d: artifact_floor_length) */
    int32_t window;               /* -w (align_buffer_size) */
    int32_t n_ref;                /* contigs of the BAM header: refID is checked against it, ref_names[refID] goes into am */
    int32_t flags;                /* FADEHIP_BAM_STORED: uncompressed BGZF out (`fade annotate -u`, htslib's level 0);
                                   * FADEHIP_BAM_NO_OUTPUT: back waits for the call's annotated records (on the device) and gives
                                   * their buffer back without making BGZF of them, *out_bytes = 0 — the rate of the record path
                                   * alone, from BAM record bytes to annotated record bytes (bench.py's value_from_records);
                                   * FADEHIP_BAM_CLIP: records called artifacts leave hard-clipped (`fade annotate -c`: what
                                   * `fade out -c` would make of the annotated file, in the same pass — by this run's rs and
                                   * alignments, never by tags read back; the five tags describe the unclipped read).  It
                                   * combines with the other two flags and holds for front and front_raw alike;
                                   * FADEHIP_BAM_EXTRACT: every call also builds `fade extract`'s records of its artifact calls
                                   * (`fade annotate --extract`), one per set artifact bit of rs, left before right, in input
                                   * order, from the record as it came in (with FADEHIP_BAM_CLIP too) and this run's alignment:
                                   * fadehip_bam_back_extract hands them out.  Combines with the other three;
                                   * FADEHIP_BAM_EJECT: records called artifacts are not written (`fade annotate --eject` on input
                                   * that is not name-sorted: what plain `fade out` would make of the annotated file, in the same
                                   * pass — by this run's rs, never by an rs tag read back).  FADEHIP_BAM_EJECT_GROUPS (implies
                                   * FADEHIP_BAM_EJECT): name-sorted input — neither is any record that shares an ejected record's
                                   * name with it in one run of consecutive records (mates, supplementary and secondary lines).
                                   * The caller decides which (`fade out`: the first ten names are non-decreasing); a name group
                                   * is never split between two calls: a call that is not the last gives its last group back to
                                   * the next (a call that is one group yields nothing), and a group longer than a call can hold
                                   * is FADEHIP_E_UNSUPPORTED.  Both combine with STORED, NO_OUTPUT and EXTRACT (the extract
                                   * records are built of the ejected artifact calls all the same); with FADEHIP_BAM_CLIP,
                                   * fadehip_bam_open returns FADEHIP_E_INVALID.  fadehip_bam_totals is not changed by them;
                                   * FADEHIP_BAM_FROM_TAGS: the records were annotated earlier, and rs and am come out of the
                                   * records themselves (the first field of each name, as fadehip_tags_batch reads them) instead of
                                   * out of a run of the aligner: `fade out -c` (with CLIP), plain `fade out` (EJECT or
                                   * EJECT_GROUPS) and `fade extract` (EXTRACT, usually with NO_OUTPUT) as the file path.  No
                                   * genome is needed, floor_len and window are ignored, no tag is written or updated and the aux
                                   * bytes pass unchanged.  Alone, every record passes byte for byte.  CLIP: a record with an
                                   * integer rs and rs & 6 is hard-clipped by the reference bases of its am sides' CIGARs (only the
                                   * third field of a side whose bit is set has to parse); a record without an integer rs passes.
                                   * EJECT: a record is written only with an integer rs and !(rs & 6) — one without rs is dropped;
                                   * EJECT_GROUPS: a record without rs neither ejects its group nor is dropped on its own.
                                   * EXTRACT: a record takes part with an integer rs, rs & 6 and an am:Z; per set bit one record
                                   * from that side's contig (-1: unknown or empty name; of two contigs of one name the first),
                                   * position and ops, at most 65535 of them.  A side that is needed and not well-formed fails
                                   * the call at its back: FADEHIP_E_INVALID, fadehip_last_error names the record's index in the
                                   * stream.  fadehip_bam_totals then sums stats.d:45-54 over the rs read back (read_count over
                                   * every record, the other seven over records with an integer rs), fadehip_bam_ejected counts
                                   * every record not written;
                                   * FADEHIP_BAM_COLLECT_NAMES / FADEHIP_BAM_EJECT_NAMED: the two passes of `fade out --fragments`
                                   * over a set of names attached with fadehip_bam_use_nameset.  Both need FROM_TAGS, exclude
                                   * each other and combine with STORED and NO_OUTPUT only (anything else: FADEHIP_E_INVALID at
                                   * fadehip_bam_open); without a set attached the first front call fails with FADEHIP_E_STATE.
                                   * COLLECT_NAMES: every record with an integer rs and rs & 6 adds its name to the set; the
                                   * records pass as under FROM_TAGS alone.  EJECT_NAMED: a record is written exactly when its
                                   * name is not in the set — also one without rs (filter.d:221-246's rule for a group, not
                                   * :254-257's); no name group is held back between calls.  Totals as under FROM_TAGS;
                                   * fadehip_bam_ejected counts the records not written;
                                   * FADEHIP_BAM_KEEP_SORTED: with CLIP (beside it STORED, EXTRACT and FROM_TAGS only; anything
                                   * else: FADEHIP_E_INVALID at fadehip_bam_open), for coordinate-sorted input: the records leave
                                   * in stable order by key — (refID as uint32, pos + 1 as uint32) of the record as it leaves,
                                   * a reset record as an unmapped one (refID -1, pos -1) — so the stream's output over all its
                                   * calls is what it writes without the flag, record for record the same bytes, in that order.
                                   * A call writes the records, held over or its own, whose key is not above the key as it came
                                   * in of its last record; the others are held on the device until a later call (the last call
                                   * writes all).  Input keys that decrease fail that call's back: FADEHIP_E_INVALID,
                                   * fadehip_last_error names the record's index in the stream; nothing of the call is written;
                                   * FADEHIP_BAM_REPORT_STATS / FADEHIP_BAM_REPORT_CLIP: `fade stats` / `fade stats-clip` as the file
                                   * path — every call also leaves the rows of the report(s) over its records, by the rules and the
                                   * kernels of fadehip_report_batch: fadehip_bam_back_report hands them out.  Valid only with
                                   * FROM_TAGS | NO_OUTPUT; beside them STORED alone may stand (and is ignored), anything else is
                                   * FADEHIP_E_INVALID at fadehip_bam_open; the two may be set together.  What fadehip_report_batch
                                   * fails on fails the call at its back, fadehip_last_error naming the record's index in the stream;
                                   * FADEHIP_BAM_INDEX: every call also leaves the .bai entries (fadehip_index_call, by the rule and
                                   * the kernels of fadehip_index_batch) of the records it writes, as they leave — clipped, in
                                   * KEEP_SORTED's order, without the ejected ones — at virtual offsets relative to the call's
                                   * first member: fadehip_bam_back_index hands them out, fadehip_bai_add takes them.  It stands
                                   * beside every flag that writes output (STORED, CLIP, KEEP_SORTED, EXTRACT, EJECT,
                                   * EJECT_GROUPS, FROM_TAGS, EJECT_NAMED) and changes no output byte; with NO_OUTPUT, REPORT_* or
                                   * COLLECT_NAMES fadehip_bam_open returns FADEHIP_E_INVALID and names the flag.  Records that
                                   * leave with a key below the key in front (within a call or between two) fail that call's
                                   * back: FADEHIP_E_INVALID, "record N: not in coordinate order", N counting the records the
                                   * stream has written; a record that ends beyond 2^29: FADEHIP_E_UNSUPPORTED;
                                   * FADEHIP_BAM_COLLECT_MATES / FADEHIP_BAM_FIX_MATES: mate fields that follow the hard clip, the
                                   * rule of fadehip_mates_fix_batch over a file, in passes behind one of COLLECT_NAMES on the same
                                   * name set.  COLLECT_MATES (needs FROM_TAGS | CLIP | NO_OUTPUT, beside them STORED alone; a name
                                   * set and a mate set attached): every primary paired-end record whose name is in the name set
                                   * stores its placement as it leaves in the mate set.  FIX_MATES (needs FROM_TAGS | CLIP; beside
                                   * them STORED, KEEP_SORTED and INDEX only; a mate set attached): every record is clipped as under
                                   * CLIP alone, then its mate fields are set from the mate set; fadehip_bam_mates counts.  A
                                   * record's own refID, pos and bin never change, so KEEP_SORTED's order and INDEX's entries are
                                   * those of CLIP alone, but for the bytes MC gains or loses.  Any other combination:
                                   * FADEHIP_E_INVALID at fadehip_bam_open, naming the flag; without the sets attached the first
                                   * front call fails with FADEHIP_E_STATE;
                                   * FADEHIP_BAM_STORE_EXTRACT: needs EXTRACT (without it: FADEHIP_E_INVALID at fadehip_bam_open,
                                   * naming the flag) and stands wherever EXTRACT does.  The calls' extract records are written
                                   * into the record store attached with fadehip_bam_use_recstore (none attached: the first front
                                   * call fails with FADEHIP_E_STATE), in stream order, and stay on the device: no copy to the
                                   * host is made, and fadehip_bam_back_extract gives 0 bytes and the number of records the call
                                   * added.  No other output byte changes.  A store that has been sorted: FADEHIP_E_STATE;
                                   * FADEHIP_BAM_STORE_OUTPUT: the records the stream would write go into the record store attached
                                   * with fadehip_bam_use_recstore (none attached: the first front call fails with
                                   * FADEHIP_E_STATE), in stream order, and stay on the device; fadehip_bam_back hands out 0 bytes.
                                   * Sorting and draining the store gives the stream's records, byte for byte, in coordinate order
                                   * of the records AS THEY LEAVE — a clipped record at its new pos, a reset record last.  Stands
                                   * with the annotate path and with FROM_TAGS, CLIP, EJECT, EJECT_GROUPS, EJECT_NAMED and
                                   * FIX_MATES; any other flag beside it: FADEHIP_E_INVALID at fadehip_bam_open, naming the flag.
                                   * The store's budget, table and window (fadehip_recstore_measure, _set_window) apply;
                                   * FADEHIP_BAM_CALMD: needs FROM_TAGS | CLIP and an uploaded genome (none by the first front
                                   * call: FADEHIP_E_STATE); beside them STORED, FIX_MATES, KEEP_SORTED, INDEX and NO_OUTPUT
                                   * only (not STORE_OUTPUT) (else FADEHIP_E_INVALID at fadehip_bam_open, naming the flag).  Every record
                                   * that leaves hard-clipped gets NM and MD recomputed by the rule of fadehip_calmd_batch;
                                   * fadehip_bam_calmd counts.  No other byte of the output changes, and a record's refID, pos and
                                   * bin never do, so order and index entries are those of the stream without the flag;
                                   * FADEHIP_BAM_REPORT_REPEATS: only with REPORT_STATS (else FADEHIP_E_INVALID at fadehip_bam_open)
                                   * and wherever it stands: the stats rows gain the two columns of fadehip_report_batch_repeats,
                                   * against the sealed set attached with fadehip_bam_use_intervals (none attached: the first
                                   * front call fails with FADEHIP_E_STATE).  The clip report's rows do not change */
    const char *const *ref_names; /* [n_ref] NUL-terminated */
    uint32_t first_record;        /* payload bytes of the first member passed to front that precede the first record */
    uint32_t tail_trim;           /* payload bytes at the END of the last member (front's last call) that are not this stream's:
                                   * a reader of a range of the file stops where the next range's first record starts */
} fadehip_bam_config;
#define FADEHIP_BAM_CHUNKS 3
#define FADEHIP_BAM_STORED 1
#define FADEHIP_BAM_NO_OUTPUT 2
#define FADEHIP_BAM_CLIP 4
#define FADEHIP_BAM_EXTRACT 8
#define FADEHIP_BAM_EJECT 16
#define FADEHIP_BAM_EJECT_GROUPS 32
#define FADEHIP_BAM_FROM_TAGS 64
#define FADEHIP_BAM_COLLECT_NAMES 128
#define FADEHIP_BAM_EJECT_NAMED 256
#define FADEHIP_BAM_KEEP_SORTED 512
#define FADEHIP_BAM_REPORT_STATS 1024
#define FADEHIP_BAM_REPORT_CLIP 2048
#define FADEHIP_BAM_INDEX 4096
#define FADEHIP_BAM_COLLECT_MATES 8192
#define FADEHIP_BAM_FIX_MATES 16384
#define FADEHIP_BAM_STORE_EXTRACT 32768
#define FADEHIP_BAM_REPORT_REPEATS 65536
#define FADEHIP_BAM_STORE_OUTPUT 131072
#define FADEHIP_BAM_CALMD 262144
int fadehip_bam_open(fadehip_ctx *ctx, const fadehip_bam_config *cfg, fadehip_bam_stream **out);
/* The set a stream opened with FADEHIP_BAM_COLLECT_NAMES adds to, or one opened with FADEHIP_BAM_EJECT_NAMED looks names up
 * in: a set of the same ctx, attached before the first front call (later: FADEHIP_E_STATE).  The set is the caller's and
 * outlives the stream; it may grow while two calls of the stream are in flight. */
int fadehip_bam_use_nameset(fadehip_bam_stream *st, fadehip_nameset *s);
/* The mate map a stream opened with FADEHIP_BAM_COLLECT_MATES stores placements in, or one opened with
 * FADEHIP_BAM_FIX_MATES sets mate fields from: a map of the same ctx, attached before the first front call (later:
 * FADEHIP_E_STATE).  The map is the caller's and outlives the stream.  fadehip_bam_mates: the records fixed and the records
 * left alone because their mate's key is ambiguous, over the calls finished so far. */
int fadehip_bam_use_mateset(fadehip_bam_stream *st, fadehip_mateset *s);
int fadehip_bam_mates(fadehip_bam_stream *st, int64_t *n_fixed, int64_t *n_ambiguous);
/* FADEHIP_BAM_CALMD: the hard-clipped records whose NM / MD were recomputed and the ones left alone because they are not
 * subject to the rule (fadehip_calmd_batch's updated[] 1 and 2), over the calls finished so far. */
int fadehip_bam_calmd(fadehip_bam_stream *st, int64_t *n_updated, int64_t *n_skipped);
/* The record store a stream opened with FADEHIP_BAM_STORE_EXTRACT appends its extract records to, or one opened with
 * FADEHIP_BAM_STORE_OUTPUT its output records (either flag; neither: FADEHIP_E_INVALID): a store of the same ctx,
 * attached before the first front call (later: FADEHIP_E_STATE).  The store is the caller's and outlives the stream; it is
 * sorted and drained after the stream's last back call. */
int fadehip_bam_use_recstore(fadehip_bam_stream *st, fadehip_recstore *s);
/* The set of intervals a stream opened with FADEHIP_BAM_REPORT_REPEATS queries: a SEALED set of the same ctx (not sealed:
 * FADEHIP_E_INVALID), attached before the first front call (later: FADEHIP_E_STATE).  The set is the caller's and outlives
 * the stream; several streams may share it. */
int fadehip_bam_use_intervals(fadehip_bam_stream *st, fadehip_intervals *s);
int fadehip_bam_prepare(fadehip_bam_stream *st, size_t call_bytes);
int fadehip_bam_front(fadehip_bam_stream *st, const void *members, size_t n_bytes, int last);
/* front for a caller that inflates itself (host cores otherwise idle; the device then spends its time on the rest):
 * payload = the members' inflated bytes, any cut, pinned memory for PCIe speed.  Calls of both kinds may alternate. */
int fadehip_bam_front_raw(fadehip_bam_stream *st, const void *payload, size_t n_bytes, int last);
/* (*out is good during the next back call and no longer: write it, or have it written, before the call after next) */
int fadehip_bam_back(fadehip_bam_stream *st, const uint8_t **out, size_t *out_bytes);
/* With FADEHIP_BAM_EXTRACT: the extract records of the call the most recent fadehip_bam_back finished — uncompressed BAM
 * records (block_size first) back to back, in pinned memory, good as long as that back call's *out; a call without
 * artifact calls gives 0 bytes, 0 records (and *recs NULL).  Without the flag, or before any back: FADEHIP_E_STATE. */
int fadehip_bam_back_extract(fadehip_bam_stream *st, const uint8_t **recs, size_t *n_bytes, int64_t *n_records);
/* With FADEHIP_BAM_REPORT_STATS / _CLIP (which: one of the two): the report's rows of the call the most recent fadehip_bam_back
 * finished — TSV lines without a header line, in input record order, the left side before the right, so that the calls of a
 * stream give the report one piece behind the other — in pinned memory, good as long as that back call's *out; a call
 * without rows gives 0 bytes, 0 rows (and *text NULL).  Without that flag, or before any back: FADEHIP_E_STATE. */
int fadehip_bam_back_report(fadehip_bam_stream *st, int32_t which, const uint8_t **text, size_t *n_bytes, int64_t *n_rows);
/* With FADEHIP_BAM_INDEX: the index entries of the call the most recent fadehip_bam_back finished, in pinned memory, good as
 * long as that back call's *out; a call that wrote nothing gives empty arrays.  Without the flag, or before any back:
 * FADEHIP_E_STATE. */
int fadehip_bam_back_index(fadehip_bam_stream *st, fadehip_index_call *out);
/* With FADEHIP_BAM_INDEX (without: FADEHIP_E_INVALID), before the first front call (later: FADEHIP_E_STATE): the calls' entries
 * are made under the CSI geometry (fadehip_index_batch_csi; not valid: FADEHIP_E_INVALID), for fadehip_csi_add, and a record
 * that ends beyond the geometry's limit fails the call at its back as one beyond 2^29 does without.  A stream on which it is
 * never called launches the kernels it always has. */
int fadehip_bam_index_geometry(fadehip_bam_stream *st, int32_t min_shift, int32_t depth);
/* totals so far: the eight Stats.parse counters (stats.d:45-54), records, reads beyond the kernels' limits */
int fadehip_bam_totals(fadehip_bam_stream *st, int64_t stats[8], int64_t *n_records, int64_t *n_oversize);
/* FADEHIP_BAM_EJECT: records not written, over the calls back has taken (0 without the flag) */
int fadehip_bam_ejected(fadehip_bam_stream *st, int64_t *n_ejected);
/* FADEHIP_BAM_KEEP_SORTED: the records (and their bytes) held back on the device behind the most recent finished call; 0 / 0
 * without the flag and behind the last call.  fadehip_bam_close with records still held gives them back unwritten. */
int fadehip_bam_held(fadehip_bam_stream *st, int64_t *n_records, int64_t *n_bytes);
void fadehip_bam_close(fadehip_bam_stream *st);

/* Sum counters over the ranks' devices with one ncclAllReduce (RCCL) — single process, one ctx
 * per device.  counters is [n_ctx][count] in, every row holds the sum on return. */
int fadehip_stats_allreduce(fadehip_ctx *const *ctxs, int n_ctx, int64_t *counters, int count);

/* The same sum with one PROCESS per GPU (the lanes of `fade annotate --gpus N`, bench.py's ranks use torch.distributed for
 * it): rank 0 makes the ncclUniqueId and leaves it in the file id_path (written under another name, then renamed), the
 * other ranks wait for the file (up to a minute); ncclCommInitRank, one ncclAllReduce(int64, sum), the communicator is
 * destroyed again.  counters[count] in, the sums out. */
int fadehip_stats_allreduce_rank(fadehip_ctx *ctx, int rank, int n_ranks, const char *id_path, int64_t *counters, int count);

#ifdef __cplusplus
}
#endif
#endif
