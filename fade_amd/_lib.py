"""ctypes binding of fade_amd/libfadehip.so (include/fadehip.h).

The library is the product path; there is no fallback.  Loading fails loudly when the shared
object is missing, and fadehip_create fails when no gfx950 device is present.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FADEHIP_LIB") or os.path.join(HERE, "libfadehip.so")  # FADEHIP_LIB: A/B builds of the same ABI

MAX_OPS = 16
NUM_SLOTS = 4
ABI_VERSION = 3
RULES_DEFAULT = 0x7f
REF_CONSUMING_OPS = (0, 2, 3, 7, 8)  # include/fadehip.h FADEHIP_REF_CONSUMING_OPS (dhtslib Cigar.alignedLength: M, D, N, =, X)
ROW_CLASSES = (4, 6, 8, 10, 12, 14, 16, 20, 24, 32)  # query rows per lane of the wave kernels (fadehip_kernels.hpp class_rows)


def row_class(l_seq):
    """R of the sw_pk_kernel<R, .> instantiation that serves reads of l_seq bases (16 R >= l_seq)."""
    return next(r for r in ROW_CLASSES if 16 * r >= l_seq)

# every symbol include/fadehip.h declares
EXPORTS = [
    "fadehip_params_default", "fadehip_abi_version", "fadehip_create", "fadehip_destroy", "fadehip_last_error",
    "fadehip_host_alloc", "fadehip_host_free", "fadehip_host_register", "fadehip_batch_bytes", "fadehip_batch_bind", "fadehip_sw_batch",
    "fadehip_genome_upload", "fadehip_annotate_upload", "fadehip_annotate_run", "fadehip_annotate_submit",
    "fadehip_annotate_results", "fadehip_annotate_collect",
    "fadehip_sync", "fadehip_last_run_profile", "fadehip_stats_allreduce",
    "fadehip_bgzf_deflate_submit", "fadehip_bgzf_deflate_wait", "fadehip_stats_allreduce_rank", "fadehip_bgzf_inflate",
    "fadehip_bam_open", "fadehip_bam_front", "fadehip_bam_front_raw", "fadehip_bam_back", "fadehip_bam_totals", "fadehip_bam_close",
    "fadehip_bam_prepare", "fadehip_sw_stats_batch", "fadehip_clip_batch", "fadehip_extract_batch", "fadehip_bam_back_extract",
    "fadehip_eject_batch", "fadehip_bam_ejected", "fadehip_genome_upload_fasta", "fadehip_genome_fetch", "fadehip_tags_batch",
    "fadehip_nameset_create", "fadehip_nameset_add_batch", "fadehip_nameset_contains_batch", "fadehip_nameset_count", "fadehip_nameset_destroy",
    "fadehip_bam_use_nameset", "fadehip_bam_held", "fadehip_coord_order_batch", "fadehip_report_batch",
    "fadehip_bam_back_report",
    "fadehip_index_batch", "fadehip_bam_back_index", "fadehip_bai_create", "fadehip_bai_add", "fadehip_bai_finish", "fadehip_bai_error",
    "fadehip_bai_destroy",
    "fadehip_index_batch_csi", "fadehip_bam_index_geometry", "fadehip_recstore_index_geometry", "fadehip_csi_create", "fadehip_csi_add",
    "fadehip_csi_finish", "fadehip_csi_error", "fadehip_csi_destroy",
    "fadehip_mateset_create", "fadehip_mateset_add_batch", "fadehip_mates_fix_batch", "fadehip_mateset_count", "fadehip_mateset_destroy",
    "fadehip_bam_use_mateset", "fadehip_bam_mates",
    "fadehip_calmd_batch", "fadehip_bam_calmd",
    "fadehip_recstore_create", "fadehip_recstore_add_batch", "fadehip_recstore_count", "fadehip_recstore_sort", "fadehip_recstore_drain",
    "fadehip_recstore_destroy", "fadehip_bam_use_recstore",
    "fadehip_recstore_set_budget", "fadehip_recstore_measure", "fadehip_recstore_over", "fadehip_recstore_histogram",
    "fadehip_recstore_set_window", "fadehip_recstore_reset", "fadehip_recstore_budget", "fadehip_recstore_resets",
    "fadehip_intervals_create", "fadehip_intervals_add", "fadehip_intervals_seal", "fadehip_intervals_count", "fadehip_intervals_overlap_batch",
    "fadehip_intervals_load_bed", "fadehip_intervals_destroy", "fadehip_report_batch_repeats", "fadehip_bam_use_intervals",
]
BAM_STORED, BAM_NO_OUTPUT, BAM_CLIP, BAM_EXTRACT, BAM_EJECT, BAM_EJECT_GROUPS, BAM_FROM_TAGS = 1, 2, 4, 8, 16, 32, 64  # fadehip_bam_config.flags
BAM_COLLECT_NAMES, BAM_EJECT_NAMED = 128, 256
BAM_KEEP_SORTED = 512
BAM_REPORT_STATS, BAM_REPORT_CLIP = 1024, 2048  # ... and `which` of fadehip_report_batch / fadehip_bam_back_report
BAM_INDEX = 4096  # every call leaves the .bai entries of the records it writes (fadehip_bam_back_index)
BAM_COLLECT_MATES, BAM_FIX_MATES = 8192, 16384  # mate fields that follow the hard clip: a MateSet attached (fadehip_bam_use_mateset)
BAM_STORE_EXTRACT = 32768  # with BAM_EXTRACT: the extract records go into a RecStore attached (fadehip_bam_use_recstore), not to the host
BAM_REPORT_REPEATS = 65536  # with BAM_REPORT_STATS: the rows gain read_rpm and art_rpm against an IntervalSet attached (fadehip_bam_use_intervals)
BAM_CALMD = 262144  # NM and MD of the records that leave hard-clipped follow the clip (the genome uploaded; fadehip_bam_calmd counts)
BAM_STORE_OUTPUT = 131072  # the OUTPUT records go into a RecStore attached (fadehip_bam_use_recstore): sorted and drained there, back hands out nothing
RECSTORE_RAW, RECSTORE_STORED, RECSTORE_INDEX = 1, 2, 4  # fadehip_recstore_drain's flags
BGZF_BLOCK = 0xff00
BGZF_LANES = 2


class Params(C.Structure):
    _fields_ = [("open", C.c_int32), ("ext", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32),
                ("max_ref_len", C.c_int32), ("max_batch_reads", C.c_int32), ("trace_bytes", C.c_int64),
                ("trace_all", C.c_int32), ("rules", C.c_uint32)]


class SwResult(C.Structure):
    _fields_ = [("score", C.c_int32), ("end_query", C.c_int32), ("end_ref", C.c_int32), ("beg_query", C.c_int32),
                ("beg_ref", C.c_int32), ("n_ops", C.c_int32), ("ops", C.c_uint32 * MAX_OPS)]


class Aln(C.Structure):
    _fields_ = [("read_idx", C.c_int32), ("art", C.c_int32), ("win_start", C.c_int64), ("win_len", C.c_int32),
                ("clip_left", C.c_int32), ("clip_right", C.c_int32), ("aligned_len", C.c_int32), ("sw", SwResult)]


SW_DTYPE = np.dtype([("score", "<i4"), ("end_query", "<i4"), ("end_ref", "<i4"), ("beg_query", "<i4"),
                     ("beg_ref", "<i4"), ("n_ops", "<i4"), ("ops", "<u4", (MAX_OPS,))])
ALN_DTYPE = np.dtype([("read_idx", "<i4"), ("art", "<i4"), ("win_start", "<i8"), ("win_len", "<i4"),
                      ("clip_left", "<i4"), ("clip_right", "<i4"), ("aligned_len", "<i4"), ("sw", SW_DTYPE)])
# fadehip_sw_stats_result: parasail's stats mode (stats.d:123,164)
SW_STATS_DTYPE = np.dtype([("score", "<i4"), ("end_query", "<i4"), ("end_ref", "<i4"), ("matches", "<i4"),
                           ("similar", "<i4"), ("length", "<i4")])
assert SW_DTYPE.itemsize == C.sizeof(SwResult)
assert ALN_DTYPE.itemsize == C.sizeof(Aln)


class ReadBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("tid", C.c_void_p), ("pos", C.c_void_p), ("flag", C.c_void_p),
                ("has_sa", C.c_void_p), ("l_seq", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar_ops", C.c_void_p),
                ("seq_off", C.c_void_p), ("seq_packed", C.c_void_p), ("n_skipped", C.c_int32),
                ("ref_span_bound", C.c_int32), ("n_with_seq", C.c_int32), ("l_seq_min", C.c_int32),
                ("l_seq_max", C.c_int32), ("reserved", C.c_int32)]


class AnnoOut(C.Structure):
    _fields_ = [("rs", C.c_void_p), ("aln", C.c_void_p), ("aln_cap", C.c_int32), ("n_aln", C.c_int32),
                ("stats", C.c_int64 * 8), ("n_oversize", C.c_int32), ("reserved", C.c_int32)]


class AnnoView(C.Structure):
    _fields_ = [("rs", C.c_void_p), ("aln", C.c_void_p), ("n_reads", C.c_int32), ("n_aln", C.c_int32),
                ("stats", C.c_int64 * 8), ("n_oversize", C.c_int32), ("reserved", C.c_int32)]


class BamConfig(C.Structure):
    _fields_ = [("floor_len", C.c_int32), ("window", C.c_int32), ("n_ref", C.c_int32), ("flags", C.c_int32),
                ("ref_names", C.POINTER(C.c_char_p)), ("first_record", C.c_uint32), ("tail_trim", C.c_uint32)]


class FaiEntry(C.Structure):  # fadehip_fai_entry: columns 2-5 of a .fai line
    _fields_ = [("length", C.c_int64), ("offset", C.c_int64), ("line_bases", C.c_int32), ("line_width", C.c_int32)]


class IndexCall(C.Structure):  # fadehip_index_call: the .bai entries of one call (or of one fadehip_index_batch)
    _fields_ = [("chunks", C.c_void_p), ("linear", C.c_void_p), ("refs", C.c_void_p), ("n_chunks", C.c_int64),
                ("n_linear", C.c_int64), ("n_refs", C.c_int64), ("n_records", C.c_int64), ("first_key", C.c_uint64),
                ("last_key", C.c_uint64)]


INDEX_CHUNK_DTYPE = np.dtype([("tid", "<i4"), ("bin", "<u4"), ("beg", "<u8"), ("end", "<u8")])
INDEX_LINEAR_DTYPE = np.dtype([("tid", "<i4"), ("window", "<u4"), ("off", "<u8")])
INDEX_REF_DTYPE = np.dtype([("tid", "<i4"), ("reserved", "<i4"), ("off_beg", "<u8"), ("off_end", "<u8"), ("n_mapped", "<u8"),
                            ("n_unmapped", "<u8")])
assert (INDEX_CHUNK_DTYPE.itemsize, INDEX_LINEAR_DTYPE.itemsize, INDEX_REF_DTYPE.itemsize) == (24, 16, 40)


class FadeHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fadehip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """Load libfadehip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); fade_amd has no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.fadehip_params_default.argtypes = [C.POINTER(Params)]
    L.fadehip_params_default.restype = None
    L.fadehip_abi_version.restype = C.c_int
    L.fadehip_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Params)]
    L.fadehip_destroy.argtypes = [vp]
    L.fadehip_destroy.restype = None
    L.fadehip_last_error.argtypes = [vp]
    L.fadehip_last_error.restype = C.c_char_p
    L.fadehip_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.fadehip_host_free.argtypes = [vp, vp]
    L.fadehip_host_register.argtypes = [vp, vp, C.c_size_t]
    L.fadehip_batch_bytes.argtypes = [i32, i64, i64]
    L.fadehip_batch_bytes.restype = C.c_size_t
    L.fadehip_batch_bind.argtypes = [vp, i32, i64, i64, C.POINTER(ReadBatch)]
    L.fadehip_annotate_results.argtypes = [vp, C.c_int, C.POINTER(AnnoView)]
    L.fadehip_sw_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.fadehip_sw_stats_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.fadehip_clip_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i64, vp]
    L.fadehip_extract_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.fadehip_eject_batch.argtypes = [vp, i32, vp, vp, vp, C.c_int, vp]
    L.fadehip_tags_batch.argtypes = [vp, i32, vp, vp, i32, C.POINTER(C.c_char_p), vp, vp, vp, vp, vp, vp, vp, vp, i64]
    L.fadehip_report_batch.argtypes = [vp, i32, i32, vp, vp, i32, C.POINTER(C.c_char_p), vp, i64, vp]
    L.fadehip_nameset_create.argtypes = [vp, C.POINTER(vp)]
    L.fadehip_nameset_add_batch.argtypes = [vp, i32, vp, vp, vp]
    L.fadehip_nameset_contains_batch.argtypes = [vp, i32, vp, vp, vp]
    L.fadehip_nameset_count.argtypes = [vp, C.POINTER(i64)]
    L.fadehip_nameset_destroy.argtypes = [vp]
    L.fadehip_nameset_destroy.restype = None
    L.fadehip_bam_use_nameset.argtypes = [vp, vp]
    L.fadehip_mateset_create.argtypes = [vp, C.POINTER(vp)]
    L.fadehip_mateset_add_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.fadehip_mates_fix_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.fadehip_mateset_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.fadehip_mateset_destroy.argtypes = [vp]
    L.fadehip_mateset_destroy.restype = None
    L.fadehip_bam_use_mateset.argtypes = [vp, vp]
    L.fadehip_recstore_create.argtypes = [vp, C.POINTER(vp)]
    L.fadehip_recstore_add_batch.argtypes = [vp, i32, vp, vp, vp]
    L.fadehip_recstore_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.fadehip_recstore_sort.argtypes = [vp]
    L.fadehip_recstore_drain.argtypes = [vp, i32, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(i64), C.POINTER(IndexCall)]
    L.fadehip_recstore_destroy.argtypes = [vp]
    L.fadehip_recstore_destroy.restype = None
    L.fadehip_bam_use_recstore.argtypes = [vp, vp]
    L.fadehip_recstore_set_budget.argtypes = [vp, C.c_uint64]
    L.fadehip_recstore_budget.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.fadehip_recstore_measure.argtypes = [vp, i32, vp]
    L.fadehip_recstore_over.argtypes = [vp, C.POINTER(i32)]
    L.fadehip_recstore_resets.argtypes = [vp, C.POINTER(i64)]
    L.fadehip_recstore_histogram.argtypes = [vp, vp, vp, C.POINTER(i64)]
    L.fadehip_recstore_set_window.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.fadehip_recstore_reset.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.fadehip_intervals_create.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.fadehip_intervals_add.argtypes = [vp, i64, vp, vp, vp]
    L.fadehip_intervals_seal.argtypes = [vp]
    L.fadehip_intervals_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i32)]
    L.fadehip_intervals_overlap_batch.argtypes = [vp, i64, vp, vp, vp, vp]
    L.fadehip_intervals_load_bed.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.fadehip_intervals_destroy.argtypes = [vp]
    L.fadehip_intervals_destroy.restype = None
    L.fadehip_report_batch_repeats.argtypes = [vp, i32, vp, vp, i32, C.POINTER(C.c_char_p), vp, vp, i64, vp]
    L.fadehip_bam_use_intervals.argtypes = [vp, vp]
    L.fadehip_bam_mates.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.fadehip_calmd_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.fadehip_bam_calmd.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.fadehip_genome_upload.argtypes = [vp, i32, vp, vp]
    L.fadehip_genome_upload_fasta.argtypes = [vp, C.c_char_p, i32, C.POINTER(FaiEntry)]
    L.fadehip_genome_fetch.argtypes = [vp, i32, i64, i64, vp]
    L.fadehip_annotate_upload.argtypes = [vp, C.c_int, C.POINTER(ReadBatch)]
    L.fadehip_annotate_run.argtypes = [vp, C.c_int, i32, i32]
    L.fadehip_annotate_submit.argtypes = [vp, C.c_int, C.POINTER(ReadBatch), i32, i32]
    L.fadehip_annotate_collect.argtypes = [vp, C.c_int, C.POINTER(AnnoOut)]
    L.fadehip_sync.argtypes = [vp]
    L.fadehip_last_run_profile.argtypes = [vp, C.c_int, C.POINTER(C.c_float * 4), C.POINTER(i64 * 6)]
    L.fadehip_stats_allreduce.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_int]
    L.fadehip_bgzf_deflate_submit.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.fadehip_stats_allreduce_rank.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, vp, C.c_int]
    L.fadehip_bgzf_deflate_wait.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fadehip_bgzf_inflate.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.fadehip_bam_open.argtypes = [vp, C.POINTER(BamConfig), C.POINTER(vp)]
    L.fadehip_bam_prepare.argtypes = [vp, C.c_size_t]
    L.fadehip_bam_front.argtypes = [vp, vp, C.c_size_t, C.c_int]
    L.fadehip_bam_front_raw.argtypes = [vp, vp, C.c_size_t, C.c_int]
    L.fadehip_bam_back.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fadehip_bam_back_extract.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(i64)]
    L.fadehip_bam_back_report.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(i64)]
    L.fadehip_bam_ejected.argtypes = [vp, C.POINTER(i64)]
    L.fadehip_bam_held.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.fadehip_coord_order_batch.argtypes = [vp, i32, vp, vp, vp]
    L.fadehip_index_batch.argtypes = [vp, i32, vp, vp, vp, C.POINTER(IndexCall)]
    L.fadehip_bam_back_index.argtypes = [vp, C.POINTER(IndexCall)]
    L.fadehip_bai_create.argtypes = [i32]
    L.fadehip_bai_create.restype = vp
    L.fadehip_bai_add.argtypes = [vp, C.c_uint64, C.POINTER(IndexCall)]
    L.fadehip_bai_finish.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fadehip_bai_error.argtypes = [vp]
    L.fadehip_bai_error.restype = C.c_char_p
    L.fadehip_bai_destroy.argtypes = [vp]
    L.fadehip_bai_destroy.restype = None
    L.fadehip_index_batch_csi.argtypes = [vp, i32, vp, vp, vp, i32, i32, C.POINTER(IndexCall)]
    L.fadehip_bam_index_geometry.argtypes = [vp, i32, i32]
    L.fadehip_recstore_index_geometry.argtypes = [vp, i32, i32]
    L.fadehip_csi_create.argtypes = [i32, i32, i32]
    L.fadehip_csi_create.restype = vp
    L.fadehip_csi_add.argtypes = [vp, C.c_uint64, C.POINTER(IndexCall)]
    L.fadehip_csi_finish.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.fadehip_csi_error.argtypes = [vp]
    L.fadehip_csi_error.restype = C.c_char_p
    L.fadehip_csi_destroy.argtypes = [vp]
    L.fadehip_csi_destroy.restype = None
    L.fadehip_bam_totals.argtypes = [vp, C.POINTER(i64 * 8), C.POINTER(i64), C.POINTER(i64)]
    L.fadehip_bam_close.argtypes = [vp]
    L.fadehip_bam_close.restype = None
    for name in EXPORTS:
        getattr(L, name)  # AttributeError here means the .so is stale against include/fadehip.h
    _lib = L
    return L
