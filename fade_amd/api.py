"""Host-side mirror of the reference interface for the annotate hot path, over the C ABI.

Reference seam (D):
    auto p = Parasail("ACTGN", 10, 2, 2, -3);           source/anno.d:36
    auto res = p.sw_striped(q_seq, ref_seq);            source/analysis.d:67
    res.score / res.position / res.cigar                source/analysis.d:69-113
    annotateTask(rec, &p, fai, mfai, floor, window)     source/anno.d:55-110

Everything that computes runs in libfadehip.so on the GPU; this module only marshals numpy
arrays and formats the am/as/ar/ab strings exactly as analysis.d:84-92,108-118 and
anno.d:94-107 do.  There is no CPU implementation of the alignment here.
"""
import ctypes as C
import os
import re

import numpy as np

from . import _lib
from ._lib import ALN_DTYPE, SW_DTYPE, SW_STATS_DTYPE, FadeHipError
from ._lib import BAM_STORED, BAM_NO_OUTPUT, BAM_CLIP, BAM_EXTRACT, BAM_EJECT, BAM_EJECT_GROUPS, BAM_FROM_TAGS  # noqa: F401  (fadehip_bam_config.flags)

CIGAR_OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"
_NT16_ARR = np.frombuffer(NT16.encode(), dtype=np.uint8)
# util.d:18-20
_COMP = np.array([0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15], dtype=np.uint8)


def cigar_str(ops):
    return "".join("%d%s" % (int(o) >> 4, CIGAR_OPS[int(o) & 0xF]) for o in ops)


class Context:
    """One fadehip_ctx (one GPU)."""

    def __init__(self, device=-1, open=10, ext=2, match=2, mismatch=-3, max_ref_len=0, max_batch_reads=0,
                 trace_bytes=0, trace_all=False, rules=None):
        self._L = _lib.load()
        p = _lib.Params()
        self._L.fadehip_params_default(C.byref(p))
        p.open, p.ext, p.match, p.mismatch = open, ext, match, mismatch
        if max_ref_len:
            p.max_ref_len = max_ref_len
        if max_batch_reads:
            p.max_batch_reads = max_batch_reads
        p.trace_bytes = trace_bytes
        p.trace_all = 1 if trace_all else 0
        if rules is not None:
            p.rules = rules
        h = C.c_void_p()
        rc = self._L.fadehip_create(C.byref(h), device, C.byref(p))
        if rc != 0:
            raise FadeHipError(rc, self._L.fadehip_last_error(None).decode())
        self._h = h
        self._keep = {}
        self._views = {}
        self.contig_names = None

    def close(self):
        if getattr(self, "_h", None):
            for ptr in getattr(self, "_pinned", []):
                self._L.fadehip_host_free(self._h, ptr)
            self._pinned = []
            self._L.fadehip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise FadeHipError(rc, self._L.fadehip_last_error(self._h).decode())

    # ---- level 1: the SW seam (analysis.d:67)
    def sw_batch_packed(self, q_concat, q_off, r_concat, r_off):
        q_concat = np.ascontiguousarray(q_concat, dtype=np.uint8)
        r_concat = np.ascontiguousarray(r_concat, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.int64)
        r_off = np.ascontiguousarray(r_off, dtype=np.int64)
        n = len(q_off) - 1
        out = np.zeros(n, dtype=SW_DTYPE)
        self._chk(self._L.fadehip_sw_batch(self._h, n, q_concat.ctypes.data, q_off.ctypes.data, r_concat.ctypes.data,
                                           r_off.ctypes.data, out.ctypes.data))
        return out

    def sw_batch(self, queries, refs):
        qs = [q.encode() if isinstance(q, str) else bytes(q) for q in queries]
        rs = [r.encode() if isinstance(r, str) else bytes(r) for r in refs]
        q_off = np.zeros(len(qs) + 1, dtype=np.int64)
        r_off = np.zeros(len(rs) + 1, dtype=np.int64)
        np.cumsum([len(q) for q in qs], out=q_off[1:])
        np.cumsum([len(r) for r in rs], out=r_off[1:])
        qc = np.frombuffer(b"".join(qs), dtype=np.uint8) if q_off[-1] else np.zeros(0, np.uint8)
        rc = np.frombuffer(b"".join(rs), dtype=np.uint8) if r_off[-1] else np.zeros(0, np.uint8)
        return self.sw_batch_packed(qc, q_off, rc, r_off)

    # ---- parasail's stats mode: the inverted-repeat search of `fade stats` (stats.d:87,123,164)
    def sw_stats_batch_packed(self, q_concat, q_off, r_concat, r_off, scoring=(3, 8, 10, -5)):
        q_concat = np.ascontiguousarray(q_concat, dtype=np.uint8)
        r_concat = np.ascontiguousarray(r_concat, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.int64)
        r_off = np.ascontiguousarray(r_off, dtype=np.int64)
        sc = np.ascontiguousarray(scoring, dtype=np.int32)
        if sc.shape != (4,):
            raise ValueError("scoring is (open, ext, match, mismatch)")
        n = len(q_off) - 1
        out = np.zeros(n, dtype=SW_STATS_DTYPE)
        self._chk(self._L.fadehip_sw_stats_batch(self._h, sc.ctypes.data, n, q_concat.ctypes.data, q_off.ctypes.data,
                                                 r_concat.ctypes.data, r_off.ctypes.data, out.ctypes.data))
        return out

    def sw_stats_batch(self, qs, rs, scoring=(3, 8, 10, -5)):
        """Parasail("ACTGN", *scoring).aligner!("sw", "stats", "striped", "16") over the pairs (qs[k], rs[k]): a structured
        array (score, end_query, end_ref, matches, similar, length) in the order of the pairs."""
        if len(qs) != len(rs):
            raise ValueError("qs and rs differ in length")
        qb = [q.encode() if isinstance(q, str) else bytes(q) for q in qs]
        rb = [r.encode() if isinstance(r, str) else bytes(r) for r in rs]
        q_off = np.zeros(len(qb) + 1, dtype=np.int64)
        r_off = np.zeros(len(rb) + 1, dtype=np.int64)
        np.cumsum([len(q) for q in qb], out=q_off[1:])
        np.cumsum([len(r) for r in rb], out=r_off[1:])
        qc = np.frombuffer(b"".join(qb), dtype=np.uint8) if q_off[-1] else np.zeros(0, np.uint8)
        rc = np.frombuffer(b"".join(rb), dtype=np.uint8) if r_off[-1] else np.zeros(0, np.uint8)
        return self.sw_stats_batch_packed(qc, q_off, rc, r_off, scoring)

    # ---- filter.d:15-91 clipRead (`fade out -c`): the device function of the file path's clip=True, on records brought here
    def clip_batch_packed(self, recs, rec_off, rs, trim_left, trim_right):
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        rs = np.ascontiguousarray(rs, dtype=np.uint8)
        tl = np.ascontiguousarray(trim_left, dtype=np.int32)
        tr = np.ascontiguousarray(trim_right, dtype=np.int32)
        n = len(rec_off) - 1
        if not (len(rs) == len(tl) == len(tr) == n):
            raise ValueError("rs, trim_left and trim_right hold one entry per record")
        out = np.zeros(len(recs) + 8 * n + 8, dtype=np.uint8)  # (a clipped record gains at most two H ops)
        out_off = np.zeros(n + 1, dtype=np.int64)
        self._chk(self._L.fadehip_clip_batch(self._h, n, recs.ctypes.data, rec_off.ctypes.data, rs.ctypes.data, tl.ctypes.data,
                                             tr.ctypes.data, out.ctypes.data, len(out), out_off.ctypes.data))
        return out[:out_off[n]], out_off

    def clip_batch(self, records, rs, trim_left, trim_right):
        """Hard-clips BAM records (bytes, block_size first) as `fade out -c` does: record k loses trim_left[k] reference
        bases at the front when rs[k] & 2 and trim_right[k] at the back when rs[k] & 4 (or is reset when a length is not
        below its aligned length).  Returns the records as a list of bytes, in order."""
        rb = [bytes(r) for r in records]
        off = np.zeros(len(rb) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rb], out=off[1:])
        cat = np.frombuffer(b"".join(rb), dtype=np.uint8) if off[-1] else np.zeros(0, np.uint8)
        out, out_off = self.clip_batch_packed(cat, off, rs, trim_left, trim_right)
        return [out[out_off[k]:out_off[k + 1]].tobytes() for k in range(len(rb))]

    # ---- NM and MD that follow the hard clip: the device functions of the file path's calmd=True, on records brought here
    def calmd_batch(self, records, rs, trim_left, trim_right, out_cap=None):
        """The records clipped as clip_batch clips them, then NM and MD of every record that leaves hard-clipped recomputed
        against the uploaded genome (fadehip_calmd_batch; the rule: tests/calmd_model.py): (list of bytes, uint8[n] with 0
        untouched, 1 updated, 2 skipped — clipped, carrying a field, and not subject to the rule).  out_cap None: room for the
        clipped records and 64 bytes of longer fields each; a call that needs more says how much and is made again with that."""
        rb = [bytes(r) for r in records]
        n = len(rb)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rb], out=off[1:])
        cat = np.frombuffer(b"".join(rb), dtype=np.uint8) if off[-1] else np.zeros(0, np.uint8)
        rs = np.ascontiguousarray(rs, dtype=np.uint8)
        tl = np.ascontiguousarray(trim_left, dtype=np.int32)
        tr = np.ascontiguousarray(trim_right, dtype=np.int32)
        if not (len(rs) == len(tl) == len(tr) == n):
            raise ValueError("rs, trim_left and trim_right hold one entry per record")
        out_off = np.zeros(n + 1, dtype=np.int64)
        updated = np.zeros(n, dtype=np.uint8)

        def call(cap):
            out = np.zeros(cap, dtype=np.uint8)
            self._chk(self._L.fadehip_calmd_batch(self._h, n, cat.ctypes.data, off.ctypes.data, rs.ctypes.data, tl.ctypes.data, tr.ctypes.data,
                                                  out.ctypes.data, cap, out_off.ctypes.data, updated.ctypes.data))
            return out

        if out_cap is not None:
            out = call(out_cap)
        else:
            try:
                out = call(len(cat) + 72 * n + 8)
            except FadeHipError as e:
                need = re.search(r"records take (\d+) bytes", str(e))
                if e.code != -1 or not need:
                    raise
                out = call(int(need.group(1)))
        return [out[out_off[k]:out_off[k + 1]].tobytes() for k in range(n)], updated

    # ---- filter.d:209-265 (plain `fade out`): the kernels of the file path's eject=..., on records brought here
    def eject_batch_packed(self, recs, rec_off, rs, grouped):
        """keep (uint8[n]): 1 where `fade out` would write the record.  grouped: the records are name-sorted, and a run of
        consecutive records with equal names leaves as a whole when one of them has rs & 6; otherwise record by record."""
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        rs = np.ascontiguousarray(rs, dtype=np.uint8)
        n = len(rec_off) - 1
        if len(rs) != n:
            raise ValueError("rs holds one entry per record")
        keep = np.zeros(n, dtype=np.uint8)
        self._chk(self._L.fadehip_eject_batch(self._h, n, recs.ctypes.data, rec_off.ctypes.data, rs.ctypes.data, 1 if grouped else 0,
                                              keep.ctypes.data))
        return keep

    def eject_batch(self, records, rs, grouped):
        """Which of the BAM records (bytes, block_size first) plain `fade out` writes, given their rs: a bool array."""
        rb = [bytes(r) for r in records]
        off = np.zeros(len(rb) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rb], out=off[1:])
        cat = np.frombuffer(b"".join(rb), dtype=np.uint8) if off[-1] else np.zeros(0, np.uint8)
        return self.eject_batch_packed(cat, off, rs, grouped).astype(bool)

    # ---- a set of read names on the device (`fade out --fragments`): the kernels of the file path's collect_names= / eject_named=
    def nameset(self):
        """An exact, growing set of read names resident on the device (fadehip_nameset_*): NameSet.add / contains / count."""
        return NameSet(self)

    # ---- mate fields that follow the hard clip: a map from (name, segment) to the record's placement as it leaves
    def recstore(self):
        """A store of BAM records on this context's device (fadehip_recstore_*): see RecStore."""
        return RecStore(self)

    def intervalset(self, names):
        """A set of genomic intervals resident on the device over the contigs `names` (fadehip_intervals_*):
        IntervalSet.add / seal / overlaps / count."""
        return IntervalSet(self, names)

    def load_bed(self, path):
        """A sealed IntervalSet of a BED file (fadehip_intervals_load_bed): plain text, names in order of first appearance."""
        return IntervalSet(self, None, bed=path)

    def mateset(self):
        """A map resident on the device from (read name, segment) to where `fade out -c` leaves that record
        (fadehip_mateset_*): MateSet.add_batch / fix_batch / count."""
        return MateSet(self)

    # ---- remap.d:11-87 (`fade extract`): the device function of the file path's extract=True, on records brought here
    def extract_batch_packed(self, recs, rec_off, rs, art_tid, art_pos, cig_off, cig, out_cap=None):
        """Side 2k is the left side of record k (built when rs[k] & 2), side 2k + 1 the right (rs[k] & 4); art_tid and art_pos
        hold 2n entries, cig_off 2n + 1 offsets into cig (BAM-encoded ops).  Returns (bytes as uint8, out_off int64[2n + 1])."""
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        rs = np.ascontiguousarray(rs, dtype=np.uint8)
        tid = np.ascontiguousarray(art_tid, dtype=np.int32)
        pos = np.ascontiguousarray(art_pos, dtype=np.int64)
        cig_off = np.ascontiguousarray(cig_off, dtype=np.int64)
        cig = np.ascontiguousarray(cig, dtype=np.uint32)
        n = len(rec_off) - 1
        if not (len(rs) == n and len(tid) == len(pos) == 2 * n and len(cig_off) == 2 * n + 1):
            raise ValueError("rs holds one entry per record, art_tid and art_pos two, cig_off 2n + 1")
        if out_cap is None:  # (every side built, with every op of cig: more than any call can take)
            out_cap = 2 * (len(recs) + 36 * n) + 4 * len(cig) + 8
        out = np.zeros(int(out_cap), dtype=np.uint8)
        out_off = np.zeros(2 * n + 1, dtype=np.int64)
        self._chk(self._L.fadehip_extract_batch(self._h, n, recs.ctypes.data, rec_off.ctypes.data, rs.ctypes.data, tid.ctypes.data,
                                                pos.ctypes.data, cig_off.ctypes.data, cig.ctypes.data, out.ctypes.data, len(out),
                                                out_off.ctypes.data))
        return out[:out_off[2 * n]], out_off

    def extract_batch(self, records, rs, sides):
        """`fade extract`'s records of BAM records (bytes, block_size first): sides[k] = (left, right), each None or
        (tid, pos, ops) with pos 0-based and ops BAM-encoded (len << 4 | op); the left one is built when rs[k] & 2, the
        right one when rs[k] & 4.  Returns the new records as a list of bytes: left before right, in input order."""
        rb = [bytes(r) for r in records]
        n = len(rb)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rb], out=off[1:])
        cat = np.frombuffer(b"".join(rb), dtype=np.uint8) if off[-1] else np.zeros(0, np.uint8)
        tid, pos, cig_off, cig = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.int64), np.zeros(2 * n + 1, np.int64), []
        for k in range(n):
            for side in range(2):
                s = sides[k][side] if sides[k] is not None else None
                if s is not None:
                    tid[2 * k + side], pos[2 * k + side] = s[0], s[1]
                    cig.extend(int(o) for o in s[2])
                cig_off[2 * k + side + 1] = len(cig)
        out, out_off = self.extract_batch_packed(cat, off, rs, tid, pos, cig_off, np.array(cig, dtype=np.uint32))
        return [out[out_off[s]:out_off[s + 1]].tobytes() for s in range(2 * n) if out_off[s + 1] > out_off[s]]

    # ---- remap.d:31-50, filter.d:24-25,58-59,190-196: rs and am read back on the device, in the shapes the three calls above take
    def tags_batch_packed(self, recs, rec_off, ref_names, cig_cap=None):
        """rs and am out of BAM records annotated earlier.  Returns a dict: rs, have (uint8[n]; have bit 0 an integer rs, bit 1
        an am:Z, bits 2 / 3 its left / right side well-formed), trim_left, trim_right (int32[n]), art_tid (int32[2n]), art_pos
        (int64[2n]), cig_off (int64[2n + 1]) and cig (uint32, BAM-encoded ops) — side 2k is record k's left one, 2k + 1 its
        right one.  cig_cap: the ops cig may hold (default: as many as the records' bytes could spell)."""
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        n = len(rec_off) - 1
        if cig_cap is None:  # (an op takes at least two bytes of am's text)
            cig_cap = len(recs) // 2 + 1
        names = [x.encode() if isinstance(x, str) else bytes(x) for x in ref_names]
        arr = (C.c_char_p * max(len(names), 1))(*names)
        o = dict(rs=np.zeros(n, np.uint8), have=np.zeros(n, np.uint8), trim_left=np.zeros(n, np.int32), trim_right=np.zeros(n, np.int32),
                 art_tid=np.zeros(2 * n, np.int32), art_pos=np.zeros(2 * n, np.int64), cig_off=np.zeros(2 * n + 1, np.int64),
                 cig=np.zeros(int(cig_cap), np.uint32))
        self._chk(self._L.fadehip_tags_batch(self._h, n, recs.ctypes.data, rec_off.ctypes.data, len(names), arr, o["rs"].ctypes.data,
                                             o["have"].ctypes.data, o["trim_left"].ctypes.data, o["trim_right"].ctypes.data,
                                             o["art_tid"].ctypes.data, o["art_pos"].ctypes.data, o["cig_off"].ctypes.data,
                                             o["cig"].ctypes.data, int(cig_cap)))
        o["cig"] = o["cig"][:o["cig_off"][2 * n]]
        return o

    def tags_batch(self, records, ref_names):
        """tags_batch_packed over BAM records given as a list of bytes (block_size first); ref_names: the header's contigs."""
        rb = [bytes(r) for r in records]
        off = np.zeros(len(rb) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rb], out=off[1:])
        cat = np.frombuffer(b"".join(rb), dtype=np.uint8) if off[-1] else np.zeros(0, np.uint8)
        return self.tags_batch_packed(cat, off, ref_names)

    # ---- stats.d:75-186, noclip.d:17-73: the rows of `fade stats` / `fade stats-clip` over annotated records, written on the device
    def report_batch_packed(self, recs, rec_off, ref_names, which, out_cap=None, repeats=None):
        """fadehip_report_batch: which is "stats" or "clip".  Returns (text, row_off): the TSV rows without a header line as
        bytes, and int64[2n + 1] offsets into them — slot 2k is record k's left side, 2k + 1 its right side, a slot without a
        row takes no bytes.  out_cap: the bytes the rows may take (default: a bound from the records' bytes).  repeats (a sealed
        IntervalSet; with "stats"): fadehip_report_batch_repeats — every row gains read_rpm and art_rpm."""
        flag = {"stats": _lib.BAM_REPORT_STATS, "clip": _lib.BAM_REPORT_CLIP}[which]
        if repeats is not None and which != "stats":
            raise ValueError('repeats goes with which="stats"')
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        n = len(rec_off) - 1
        if out_cap is None:  # (a row's long columns are copies of bytes of its record, at most seven of them)
            out_cap = 16 * len(recs) + 1024 * max(n, 0) + 1024
        names = [x.encode() if isinstance(x, str) else bytes(x) for x in ref_names]
        arr = (C.c_char_p * max(len(names), 1))(*names)
        out = np.zeros(int(out_cap), np.uint8)
        row_off = np.zeros(2 * max(n, 0) + 1, np.int64)
        if repeats is not None:
            self._chk(self._L.fadehip_report_batch_repeats(self._h, n, recs.ctypes.data if recs.nbytes else None, rec_off.ctypes.data, len(names), arr, repeats._h,
                                                           out.ctypes.data if out_cap else None, int(out_cap), row_off.ctypes.data))
        else:
            self._chk(self._L.fadehip_report_batch(self._h, flag, n, recs.ctypes.data if recs.nbytes else None, rec_off.ctypes.data, len(names), arr,
                                                   out.ctypes.data if out_cap else None, int(out_cap), row_off.ctypes.data))
        return out[:row_off[-1]].tobytes(), row_off

    def report_batch(self, records, ref_names, which, repeats=None):
        """report_batch_packed over BAM records given as a list of bytes (block_size first).  which: "stats" or "clip" gives
        the report's rows as bytes; "both" gives the pair (stats, clip), each what the call for it alone gives.  repeats (a
        sealed IntervalSet): the stats rows gain read_rpm and art_rpm; the clip rows stay as they are."""
        rb = [bytes(r) for r in records]
        off = np.zeros(len(rb) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rb], out=off[1:])
        cat = np.frombuffer(b"".join(rb), dtype=np.uint8) if off[-1] else np.zeros(0, np.uint8)
        if which == "both":
            return tuple(self.report_batch_packed(cat, off, ref_names, w, repeats=repeats if w == "stats" else None)[0] for w in ("stats", "clip"))
        return self.report_batch_packed(cat, off, ref_names, which, repeats=repeats)[0]

    def coord_order_batch(self, recs, rec_off):
        """fadehip_coord_order_batch: the stable coordinate order of BAM records (recs: uint8, concatenated; rec_off: n + 1
        offsets) by (refID, pos + 1) as unsigned.  Returns int32[n]: order[j] is the record that comes j-th."""
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        n = len(rec_off) - 1
        order = np.zeros(max(n, 0), np.int32)
        self._chk(self._L.fadehip_coord_order_batch(self._h, n, recs.ctypes.data if recs.nbytes else None, rec_off.ctypes.data,
                                                    order.ctypes.data if n > 0 else None))
        return order

    def index_batch(self, recs, rec_off, voff, csi=None):
        """fadehip_index_batch: the .bai entries of coordinate-sorted BAM records (recs: uint8, concatenated; rec_off: n + 1
        offsets) at the virtual offsets voff (n + 1: record k lies in voff[k] .. voff[k + 1]).  Returns the call's entries as
        index_call_dict gives them.  Keys that step back: FadeHipError -1; a record ending beyond 2^29: -5.
        csi=(min_shift, depth): fadehip_index_batch_csi, the entries of a CSI of that geometry (CsiBuilder takes them); a
        geometry that is not valid: -1; a record ending beyond 2^(min_shift + 3 * depth): -5."""
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        voff = np.ascontiguousarray(voff, dtype=np.uint64)
        n = len(rec_off) - 1
        if len(voff) != n + 1:
            raise ValueError("voff holds n + 1 virtual offsets")
        c = _lib.IndexCall()
        if csi is not None:
            self._chk(self._L.fadehip_index_batch_csi(self._h, n, recs.ctypes.data if recs.nbytes else None, rec_off.ctypes.data, voff.ctypes.data,
                                                      int(csi[0]), int(csi[1]), C.byref(c)))
            return index_call_dict(c)
        self._chk(self._L.fadehip_index_batch(self._h, n, recs.ctypes.data if recs.nbytes else None, rec_off.ctypes.data, voff.ctypes.data, C.byref(c)))
        return index_call_dict(c)

    # ---- level 2: annotateTask over a batch (anno.d:55-110)
    def genome_upload(self, names, seqs):
        """seqs: list of bytes / uint8 arrays (raw FASTA residues)."""
        arrs = [np.frombuffer(s.encode() if isinstance(s, str) else s, dtype=np.uint8) if not isinstance(s, np.ndarray)
                else np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        n = len(arrs)
        lens = (C.c_int64 * n)(*[len(a) for a in arrs])
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        self._chk(self._L.fadehip_genome_upload(self._h, n, C.cast(lens, C.c_void_p), C.cast(ptrs, C.c_void_p)))
        self.contig_names = [x.decode() if isinstance(x, bytes) else x for x in names]

    def genome_upload_fasta(self, path, names=None):
        """The genome from an indexed FASTA file (plain or bgzip-compressed): the library reads the file through path + ".fai"
        and packs it on the device.  names: the contigs to take, in this order (default: every contig, in the index's order)."""
        from . import fasta_index
        fai = fasta_index.read_fai(os.fspath(path) + ".fai")
        if names is None:
            picked = fai
        else:
            by_name = {e.name: e for e in fai}
            picked = [by_name[n.decode() if isinstance(n, bytes) else n] for n in names]
        ents = (_lib.FaiEntry * max(len(picked), 1))()
        for k, e in enumerate(picked):
            ents[k].length, ents[k].offset, ents[k].line_bases, ents[k].line_width = e.length, e.offset, e.line_bases, e.line_width
        self._chk(self._L.fadehip_genome_upload_fasta(self._h, os.fsencode(path), len(picked), ents))
        self.contig_names = [e.name for e in picked]

    def genome_fetch(self, tid, start, n):
        """n upper-case letters of contig tid from the 0-based start, as the device holds them (fetchSequence, analysis.d:63)."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        self._chk(self._L.fadehip_genome_fetch(self._h, int(tid), int(start), int(n), out.ctypes.data))
        return out[:max(int(n), 0)].tobytes()

    _ARRAYS = (("tid", np.int32), ("pos", np.int32), ("l_seq", np.int32), ("cigar_off", np.uint32), ("seq_off", np.uint32),
               ("flag", np.uint16), ("has_sa", np.uint8), ("cigar_ops", np.uint32), ("seq_packed", np.uint8))

    def _c_batch(self, batch):
        keep = {k: np.ascontiguousarray(batch[k], dtype=dt) for k, dt in self._ARRAYS}
        n = len(keep["pos"])
        b = _lib.ReadBatch()
        b.n_reads = n
        for k, _ in self._ARRAYS:
            setattr(b, k, keep[k].ctypes.data)
        self._hints(b, batch)
        return b, keep, n

    @staticmethod
    def _hints(b, batch):
        """What the caller knows about the batch travels with it (include/fadehip.h: n_skipped, ref_span_bound and the
        ABI-3 bounds n_with_seq / l_seq_min / l_seq_max; see with_bounds)."""
        b.n_skipped = int(batch.get("n_skipped", 0))
        b.ref_span_bound = int(batch.get("ref_span_bound", 0))
        b.n_with_seq = int(batch.get("n_with_seq", 0))
        b.l_seq_min = int(batch.get("l_seq_min", 0))
        b.l_seq_max = int(batch.get("l_seq_max", 0))

    def pinned_batch(self, batch):
        """The batch as ONE pinned block in the canonical layout (fadehip_batch_bytes / fadehip_batch_bind), what a
        reader thread would fill in place: annotate_upload of the returned object is a single hipMemcpyAsync.
        `n_skipped` / `ref_span_bound` of the dict travel along (see clipped_only)."""
        arrs = {k: np.ascontiguousarray(batch[k], dtype=dt) for k, dt in self._ARRAYS}
        n = len(arrs["pos"])
        n_cig, n_seq = int(arrs["cigar_off"][n]) if n else 0, int(arrs["seq_off"][n]) if n else 0
        nbytes = self._L.fadehip_batch_bytes(n, n_cig, n_seq)
        ptr = C.c_void_p()
        self._chk(self._L.fadehip_host_alloc(self._h, nbytes, C.byref(ptr)))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(ptr)
        b = _lib.ReadBatch()
        self._chk(self._L.fadehip_batch_bind(ptr, n, n_cig, n_seq, C.byref(b)))
        for k, dt in self._ARRAYS:
            a = arrs[k]
            if a.nbytes:
                C.memmove(getattr(b, k), a.ctypes.data, a.nbytes)
        self._hints(b, batch)
        return PinnedBatch(b, n, ptr, nbytes)

    @staticmethod
    def clipped_only(batch, ref_span_bound=True):
        """anno.d:61-65 gives an unmapped record, or one without an S op, rs = 0 before anything else is looked at:
        such records need not be sent.  Returns (sub_batch, sent_idx): the records that must be sent, with
        `n_skipped` (counted into read_count by the device path) and, optionally, `ref_span_bound` (max
        cigar.alignedLength, which a reader knows from parsing); rs / read_idx of the results index sent_idx."""
        from . import synth
        co = np.asarray(batch["cigar_off"], dtype=np.int64)
        ops = np.asarray(batch["cigar_ops"])
        is_s = np.concatenate([(ops & 15) == 4, [False]]).astype(np.int64)
        cs = np.concatenate([[0], np.cumsum(is_s)])
        has_s = (cs[co[1:]] - cs[co[:-1]]) > 0
        keep = has_s & ((np.asarray(batch["flag"]) & 4) == 0)
        idx = np.nonzero(keep)[0]
        sub = synth.take(batch, idx)
        sub["n_skipped"] = int(len(keep) - len(idx))
        if ref_span_bound:
            ref = np.isin(ops & 15, _lib.REF_CONSUMING_OPS) * (ops >> 4).astype(np.int64)
            cr = np.concatenate([[0], np.cumsum(ref)])
            al = cr[co[1:]] - cr[co[:-1]]
            sub["ref_span_bound"] = int(al[idx].max()) if len(idx) else 1
        return sub, idx

    @staticmethod
    def compact_sequences(batch):
        """Drop the packed bases of records the device never reads (unmapped, or no S op in the CIGAR; anno.d:61):
        they get an empty slice (seq_off[i+1] == seq_off[i]).  A tenth of the upload for 10 % clipped reads."""
        co = np.asarray(batch["cigar_off"], dtype=np.int64)
        is_s = np.concatenate([(np.asarray(batch["cigar_ops"]) & 15) == 4, [False]]).astype(np.int64)
        cs = np.concatenate([[0], np.cumsum(is_s)])
        has_s = (cs[co[1:]] - cs[co[:-1]]) > 0
        keep = has_s & ((np.asarray(batch["flag"]) & 4) == 0)
        so = np.asarray(batch["seq_off"], dtype=np.int64)
        lens = (so[1:] - so[:-1]) * keep
        out = dict(batch)
        out["seq_packed"] = np.asarray(batch["seq_packed"])[np.repeat(keep, so[1:] - so[:-1])]
        out["seq_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        return out

    @staticmethod
    def with_bounds(batch):
        """What a packing thread knows when it has filled a block, passed along so that upload does no per-record host
        work (ABI 3): every record is sent, the ones the device never aligns (unmapped, or no S op; anno.d:61) without
        their bases; `ref_span_bound` = max cigar.alignedLength over the records that carry bases, `n_with_seq` their
        number, `l_seq_min` / `l_seq_max` their shortest / longest read."""
        out = Context.compact_sequences(batch)
        so = np.asarray(out["seq_off"], dtype=np.int64)
        has = (so[1:] - so[:-1]) > 0
        ls = np.asarray(out["l_seq"])[has]
        out["n_with_seq"] = int(has.sum())
        out["l_seq_min"] = int(ls.min()) if len(ls) else 0
        out["l_seq_max"] = int(ls.max()) if len(ls) else 0
        co = np.asarray(out["cigar_off"], dtype=np.int64)
        ops = np.asarray(out["cigar_ops"])
        ref = np.isin(ops & 15, _lib.REF_CONSUMING_OPS) * (ops >> 4).astype(np.int64)
        cr = np.concatenate([[0], np.cumsum(ref)])
        al = (cr[co[1:]] - cr[co[:-1]])[has]
        out["ref_span_bound"] = int(al.max()) if len(al) else 1
        out["n_skipped"] = 0
        return out

    def annotate_upload(self, slot, batch):
        """batch: a dict of numpy arrays (gathered into the slot's staging block) or a PinnedBatch (one DMA).
        Never waits for the slot's run in flight: upload the batch of the slot's NEXT run right after annotate_run."""
        # (the arrays of the batch in flight and of the batch uploaded for the next run are both kept alive)
        if isinstance(batch, PinnedBatch):
            self._keep[slot] = (self._keep.get(slot, (None,))[-1], batch)
            self._chk(self._L.fadehip_annotate_upload(self._h, slot, C.byref(batch.c)))
            return
        b, keep, n = self._c_batch(batch)
        self._keep[slot] = (self._keep.get(slot, (None,))[-1], keep)
        self._chk(self._L.fadehip_annotate_upload(self._h, slot, C.byref(b)))

    def annotate_run(self, slot, floor_len=5, window=300):
        """Enqueues the whole device path of the slot's batch and returns (errors of the batch surface at results)."""
        self._chk(self._L.fadehip_annotate_run(self._h, slot, floor_len, window))

    def _view(self, addr, count, dtype):
        """numpy view of `count` items at a device-library address; the (address, size) pairs of a streaming run repeat,
        and building a ctypes array type per call costs tens of microseconds."""
        key = (addr, count, np.dtype(dtype).itemsize)
        arr = self._views.get(key)
        if arr is None:
            nbytes = count * np.dtype(dtype).itemsize
            arr = np.frombuffer((C.c_uint8 * nbytes).from_address(addr), dtype=dtype)
            if len(self._views) > 256:
                self._views.clear()
            self._views[key] = arr
        return arr

    def annotate_results(self, slot):
        """Waits for the slot; rs [n], alignments [n_aln], stats [8] as views into the slot's pinned result block
        (valid until the slot is run again), plus n_oversize."""
        v = _lib.AnnoView()
        self._chk(self._L.fadehip_annotate_results(self._h, slot, C.byref(v)))
        n, n_aln = v.n_reads, v.n_aln
        rs = self._view(v.rs, n, np.uint8) if n else np.zeros(0, np.uint8)
        aln = self._view(v.aln, n_aln, ALN_DTYPE) if n_aln else np.zeros(0, ALN_DTYPE)
        self.last_oversize = int(v.n_oversize)
        return rs, aln, np.array(list(v.stats), dtype=np.int64)

    def annotate_collect(self, slot, copy=True):
        """rs [n], alignments [n_aln], stats [8]; with copy=False the arrays are views that the slot's next run
        invalidates."""
        rs, aln, stats = self.annotate_results(slot)
        if copy:
            return rs.copy(), aln.copy(), stats
        return rs, aln, stats

    def annotate(self, batch, floor_len=5, window=300, slot=0):
        self.annotate_upload(slot, batch)
        self.annotate_run(slot, floor_len, window)
        return self.annotate_collect(slot)

    # ---- BGZF compression of an output stream (util.d:65-76, anno.d:47-49)
    def bgzf_deflate_submit(self, lane, data):
        """data: bytes / uint8 array (kept alive until bgzf_deflate_wait)."""
        arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        self._keep[("bgzf", lane)] = arr
        self._chk(self._L.fadehip_bgzf_deflate_submit(self._h, lane, arr.ctypes.data, arr.nbytes))

    def bgzf_deflate_wait(self, lane):
        """The BGZF members of the submitted bytes (no end-of-file marker), as bytes."""
        ptr, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fadehip_bgzf_deflate_wait(self._h, lane, C.byref(ptr), C.byref(n)))
        self._keep.pop(("bgzf", lane), None)
        return C.string_at(ptr.value, n.value)

    def bgzf_deflate(self, data, lane=0):
        self.bgzf_deflate_submit(lane, data)
        return self.bgzf_deflate_wait(lane)

    def bam_stream(self, ref_names, floor_len=5, window=300, first_record=0, stored=False, tail_trim=0, no_output=False, clip=False, extract=False, eject=None, from_tags=False,
                   collect_names=None, eject_named=None, keep_sorted=False, report=None, index=False, collect_mates=None, fix_mates=False, mateset=None, recstore=None, repeats=None, store_output=None, calmd=False):
        """The file path on the device (fadehip_bam_*): BGZF members of a BAM's records in, BGZF members of the annotated
        records out.  ref_names: the BAM header's contigs (the genome must be uploaded).  clip: records called artifacts leave
        hard-clipped (`fade annotate -c`).  extract: every call also builds `fade extract`'s records of its artifact calls
        (`fade annotate --extract`); BamStream.back_extract() fetches them after each back().  eject: "records" — artifact
        calls are not written; "groups" — nor any record of their name group, on name-sorted input (`fade annotate --eject`);
        BamStream.ejected() counts them.  Not with clip.  from_tags: the records were annotated earlier and rs / am come out
        of the records themselves (FADEHIP_BAM_FROM_TAGS): no genome is needed, floor_len and window are ignored, and clip,
        eject and extract are `fade out -c`, plain `fade out` and `fade extract` — a record without an integer rs passes
        clip, is dropped by eject="records" and counts as clean under eject="groups"; a needed am side that is not
        well-formed fails the call at its back().  collect_names / eject_named (a NameSet of this context; with from_tags,
        stored and no_output only): the two passes of `fade out --fragments` — every record with rs & 6 adds its name to the
        set / a record is written exactly when its name is not in the set.  True instead of a set sets the flag alone (the
        first front() then fails: no set is attached).  keep_sorted (with clip; beside it stored, extract and from_tags only):
        coordinate-sorted input leaves in coordinate order — a clipped record at its new position, a reset one at the end —
        with a small tail held on the device between calls; BamStream.held() counts it.  report ("stats", "clip" or "both";
        with from_tags and no_output, beside them stored only): `fade stats` / `fade stats-clip` — every call also leaves the
        rows of the report(s) over its records; BamStream.report(which) fetches them after each back().  index (beside every
        mode that writes output; not with no_output, report or collect_names): every call also leaves the .bai entries of the
        records it writes, at virtual offsets relative to the call's first member; BamStream.back_index() fetches them after
        each back(), BaiBuilder makes the file of them.  collect_mates / fix_mates, with mateset a MateSet of this context:
        mate fields that follow the hard clip, in two passes behind one with collect_names.  collect_mates (that pass's
        NameSet; with from_tags, clip and no_output, beside them stored only): every primary paired-end record whose name is
        in the NameSet stores its placement as it leaves in the MateSet.  fix_mates (with from_tags and clip; beside them
        stored, keep_sorted and index only): every record's mate fields are set from the MateSet; BamStream.mates() counts.
        True for collect_mates, or no mateset, sets the flag alone (the first front() then fails).  recstore (a RecStore of
        this context; with extract, wherever extract stands): the calls' extract records stay on the device, appended to the
        store in stream order — back_extract() then gives no bytes and the number of records the call added — to be sorted
        and drained once the stream has ended (`fade extract --sorted`, `fade annotate --extract-sorted`).  True instead of a
        store sets the flag alone (the first front() then fails).  repeats (a sealed IntervalSet of this context; with
        report "stats" or "both"): the stats rows gain read_rpm and art_rpm (`fade stats --repeats`).  True instead of a set
        sets the flag alone (the first front() then fails).  store_output (a RecStore of this context; with the annotate path
        or from_tags, beside them clip, eject, eject_named and fix_mates only): the records the stream would write stay on the
        device, appended to the store in stream order — back() then gives no bytes — to be sorted and drained once the stream
        has ended: the stream's records in coordinate order as they leave, whatever the input's order.  The store's budget,
        bucket table and window apply (RecStore.set_budget, measure, set_window).  True instead of a store sets the flag alone.
        calmd (with from_tags and clip, the genome uploaded; beside them stored, fix_mates, keep_sorted, index and no_output
        only; not store_output): NM and MD of every record that leaves hard-clipped are recomputed against the genome, the rule of
        calmd_batch; BamStream.calmd() counts.  No other byte of the output changes."""
        return BamStream(self, ref_names, floor_len, window, first_record, stored, tail_trim, no_output, clip, extract, eject, from_tags,
                         collect_names, eject_named, keep_sorted, report, index, collect_mates, fix_mates, mateset, recstore, repeats, store_output, calmd)

    def bgzf_inflate(self, members, out_cap=None):
        """Whole BGZF members (bytes / uint8 array) -> their payloads, inflated on the device (CRC32 and ISIZE checked)."""
        arr = np.frombuffer(members, dtype=np.uint8) if isinstance(members, (bytes, bytearray, memoryview)) else np.ascontiguousarray(members, dtype=np.uint8)
        if out_cap is None:  # ISIZE of every member: at most 64 KiB each, and a member takes at least 28 bytes
            out_cap = 65536 * (arr.nbytes // 28 + 1)
            out_cap = min(out_cap, max(1 << 16, arr.nbytes * 1100))
        out = np.empty(out_cap, dtype=np.uint8)
        n = C.c_size_t(0)
        self._chk(self._L.fadehip_bgzf_inflate(self._h, arr.ctypes.data, arr.nbytes, out.ctypes.data, out_cap, C.byref(n)))
        return out[:n.value]

    def sync(self):
        self._chk(self._L.fadehip_sync(self._h))

    def last_profile(self, slot=0):
        ms = (C.c_float * 4)()
        cnt = (C.c_int64 * 6)()
        self._chk(self._L.fadehip_last_run_profile(self._h, slot, C.byref(ms), C.byref(cnt)))
        return dict(gate_ms=ms[0], forward_ms=ms[1], traceback_ms=ms[2], total_ms=ms[3], alignments=cnt[0],
                    cells=cnt[1], trace_bytes=cnt[2], algorithmic_bytes=cnt[3], snapshot_bytes=cnt[4], candidates=cnt[5])


def index_call_dict(c):
    """A fadehip_index_call copied out of the library's memory: chunks [(tid, bin, beg, end)], linear [(tid, window, off)],
    refs [(tid, off_beg, off_end, n_mapped, n_unmapped)] as lists of int tuples, n (records), first_key, last_key."""
    def arr(p, n, dt):
        return np.frombuffer(C.string_at(p, n * dt.itemsize), dtype=dt) if n else np.zeros(0, dt)
    ch = arr(c.chunks, c.n_chunks, _lib.INDEX_CHUNK_DTYPE)
    li = arr(c.linear, c.n_linear, _lib.INDEX_LINEAR_DTYPE)
    rf = arr(c.refs, c.n_refs, _lib.INDEX_REF_DTYPE)
    return dict(chunks=[(int(x["tid"]), int(x["bin"]), int(x["beg"]), int(x["end"])) for x in ch],
                linear=[(int(x["tid"]), int(x["window"]), int(x["off"])) for x in li],
                refs=[(int(x["tid"]), int(x["off_beg"]), int(x["off_end"]), int(x["n_mapped"]), int(x["n_unmapped"])) for x in rf],
                n=int(c.n_records), first_key=int(c.first_key), last_key=int(c.last_key))


class BaiBuilder:
    """fadehip_bai_*: a .bai out of the calls' index entries (BamStream.back_index(), Context.index_batch()), on the host.
    add(base_file_offset, call) in stream order — call as index_call_dict gives it —, finish() the file's bytes."""

    def __init__(self, n_ref):
        self._L = _lib.load()
        self._h = self._L.fadehip_bai_create(int(n_ref))
        if not self._h:
            raise FadeHipError(-1, "fadehip_bai_create failed")
        self._add, self._finish, self._error, self._destroy = (self._L.fadehip_bai_add, self._L.fadehip_bai_finish, self._L.fadehip_bai_error,
                                                               self._L.fadehip_bai_destroy)

    def _chk(self, rc):
        if rc != 0:
            raise FadeHipError(rc, self._error(self._h).decode())

    def add(self, base_file_offset, call):
        ch = np.array(call["chunks"], dtype=_lib.INDEX_CHUNK_DTYPE) if call["chunks"] else np.zeros(0, _lib.INDEX_CHUNK_DTYPE)
        li = np.array(call["linear"], dtype=_lib.INDEX_LINEAR_DTYPE) if call["linear"] else np.zeros(0, _lib.INDEX_LINEAR_DTYPE)
        rf = np.zeros(len(call["refs"]), _lib.INDEX_REF_DTYPE)
        for k, (tid, u, v, nm, nu) in enumerate(call["refs"]):
            rf[k] = (tid, 0, u, v, nm, nu)
        c = _lib.IndexCall(ch.ctypes.data if len(ch) else None, li.ctypes.data if len(li) else None, rf.ctypes.data if len(rf) else None,
                           len(ch), len(li), len(rf), call["n"], call["first_key"], call["last_key"])
        self._chk(self._add(self._h, int(base_file_offset), C.byref(c)))

    def finish(self):
        p, n = C.c_void_p(), C.c_size_t(0)
        self._chk(self._finish(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def close(self):
        if self._h:
            self._destroy(self._h)
            self._h = None


class CsiBuilder(BaiBuilder):
    """fadehip_csi_*: a .csi out of the calls' index entries made under the geometry (min_shift, depth) —
    BamStream.index_geometry(), RecStore.index_geometry(), Context.index_batch(csi=) —, on the host.  add() as BaiBuilder's;
    finish() the uncompressed payload; file_bytes() the file: the payload in BGZF members of at most 0xff00 payload bytes
    (zlib), then the end-of-file marker."""

    _EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

    def __init__(self, n_ref, min_shift, depth):
        self._L = _lib.load()
        self._h = self._L.fadehip_csi_create(int(n_ref), int(min_shift), int(depth))
        if not self._h:
            raise FadeHipError(-1, "fadehip_csi_create failed (n_ref %d, min_shift %d, depth %d)" % (n_ref, min_shift, depth))
        self._add, self._finish, self._error, self._destroy = (self._L.fadehip_csi_add, self._L.fadehip_csi_finish, self._L.fadehip_csi_error,
                                                               self._L.fadehip_csi_destroy)

    def file_bytes(self, level=6):
        import struct
        import zlib
        payload, out = self.finish(), []
        for at in range(0, len(payload), 0xff00):
            part = payload[at:at + 0xff00]
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            body = co.compress(part) + co.flush()
            out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(part), len(part)))
        return b"".join(out) + self._EOF


class PinnedBatch:
    """A batch in one pinned block (Context.pinned_batch): `c` is the bound fadehip_read_batch."""

    __slots__ = ("c", "n", "ptr", "nbytes")

    def __init__(self, c, n, ptr, nbytes):
        self.c, self.n, self.ptr, self.nbytes = c, n, ptr, nbytes


def stats_allreduce(contexts, counters):
    """Sum per-device counters with one RCCL all-reduce (single process, one Context per device).
    counters: int64 array [n_ctx, count]; returns the reduced copy (every row = the sum)."""
    L = _lib.load()
    arr = np.ascontiguousarray(counters, dtype=np.int64).copy()
    n, count = arr.shape
    assert n == len(contexts)
    hs = (C.c_void_p * n)(*[c._h for c in contexts])
    rc = L.fadehip_stats_allreduce(hs, n, arr.ctypes.data, count)
    if rc != 0:
        raise FadeHipError(rc, L.fadehip_last_error(contexts[0]._h).decode())
    return arr


class SwResult:
    """What FADE reads from a dparasail result (analysis.d:69-113)."""

    __slots__ = ("score", "position", "cigar", "end_query", "end_ref", "beg_query", "n_ops")

    def __init__(self, rec):
        self.score = int(rec["score"])
        self.position = int(rec["beg_ref"])
        self.n_ops = int(rec["n_ops"])
        self.cigar = [int(o) for o in rec["ops"][:min(self.n_ops, _lib.MAX_OPS)]]
        self.end_query = int(rec["end_query"])
        self.end_ref = int(rec["end_ref"])
        self.beg_query = int(rec["beg_query"])

    def cigar_string(self):
        return cigar_str(self.cigar)


class Parasail:
    """Parasail("ACTGN", 10, 2, 2, -3) — anno.d:36 — with the alignment done on the GPU."""

    def __init__(self, alphabet="ACTGN", open=10, ext=2, match=2, mismatch=-3, device=-1, ctx=None):
        if sorted(alphabet.upper()) != sorted("ACTGN"):
            raise ValueError("the gfx950 kernels carry the ACTGN+wildcard matrix of anno.d:36 only")
        self.ctx = ctx or Context(device=device, open=open, ext=ext, match=match, mismatch=mismatch)

    def sw_striped(self, q_seq, ref_seq):
        return SwResult(self.ctx.sw_batch([q_seq], [ref_seq])[0])

    def sw_striped_batch(self, q_seqs, ref_seqs):
        return [SwResult(r) for r in self.ctx.sw_batch(q_seqs, ref_seqs)]


# ---------------------------------------------------------------- tag formatting (host, as in the reference)
def unpack_seq(seq_packed, off, l_seq):
    """BAM 4-bit -> nt16 codes (uint8 array of l_seq)."""
    b = np.asarray(seq_packed[off:off + (l_seq + 1) // 2], dtype=np.uint8)
    codes = np.empty(2 * len(b), dtype=np.uint8)
    codes[0::2] = b >> 4
    codes[1::2] = b & 15
    return codes[:l_seq]


def format_tags(batch, contig_names, rs, aln):
    """am/as/ar/ab for every artifact read: analysis.d:84-92,108-118 + anno.d:98-107.
    Returns {read_idx: dict(rs=, am=, as_=, ar=, ab=)} for reads with art_left|art_right."""
    out = {}
    for a in aln:
        art = int(a["art"])
        if not art:
            continue
        i = int(a["read_idx"])
        lq = int(batch["l_seq"][i])
        codes = unpack_seq(batch["seq_packed"], int(batch["seq_off"][i]), lq)
        seq = _NT16_ARR[codes].tobytes().decode()
        q_seq = _NT16_ARR[_COMP[codes][::-1]].tobytes().decode()  # util.d:23-34
        qo = int(batch["qual_off"][i])
        bq = (np.asarray(batch["qual"][qo:qo + lq], dtype=np.uint8) + 33).astype(np.uint8).tobytes().decode("latin-1")
        sw = a["sw"]
        n_ops = int(sw["n_ops"])
        ops = [int(o) for o in sw["ops"][:n_ops]]
        name = contig_names[int(batch["tid"][i])]
        apos = int(a["win_start"]) + int(sw["beg_ref"])
        pos = int(batch["pos"][i])
        left = ["", "", "", ""]
        right = ["", "", "", ""]
        if art & 1:  # analysis.d:84-92
            clip = int(a["clip_left"])
            overlap = apos - (pos - clip) if apos >= pos - clip else 0
            lead_s = ops[0] >> 4 if (ops[0] & 15) == 4 else 0
            plen = min(lq, (lq - lead_s) + overlap)
            left = ["%s,%d,%s" % (name, apos, cigar_str(ops)), seq[:plen], q_seq[lq - plen:], bq[:plen]]
        if art & 2:  # analysis.d:108-118
            clip = int(a["clip_right"])
            res_aligned = sum(o >> 4 for o in ops if (o & 15) in _lib.REF_CONSUMING_OPS)
            lhs = pos + int(a["aligned_len"]) + clip
            rhs = apos + res_aligned
            overlap = lhs - rhs if lhs >= rhs else 0
            trail_s = ops[-1] >> 4 if (ops[-1] & 15) == 4 else 0
            plen = min(lq, (lq - trail_s) + overlap)
            right = ["%s,%d,%s" % (name, apos, cigar_str(ops)), seq[lq - plen:], q_seq[:plen], bq[lq - plen:]]
        out[i] = dict(rs=int(rs[i]), am=left[0] + ";" + right[0], as_=left[1] + ";" + right[1],
                      ar=left[2] + ";" + right[2], ab=left[3] + ";" + right[3])
    return out


class BamStream:
    def __init__(self, ctx, ref_names, floor_len, window, first_record, stored=False, tail_trim=0, no_output=False, clip=False, extract=False, eject=None, from_tags=False,
                 collect_names=None, eject_named=None, keep_sorted=False, report=None, index=False, collect_mates=None, fix_mates=False, mateset=None, recstore=None, repeats=None, store_output=None, calmd=False):
        self._ctx, self._L = ctx, ctx._L
        if report not in (None, "stats", "clip", "both"):
            raise ValueError('report is None, "stats", "clip" or "both"')
        rp = (_lib.BAM_REPORT_STATS if report in ("stats", "both") else 0) | (_lib.BAM_REPORT_CLIP if report in ("clip", "both") else 0)
        if eject not in (None, False, "records", "groups"):
            raise ValueError('eject is None, "records" or "groups"')
        ej = BAM_EJECT | BAM_EJECT_GROUPS if eject == "groups" else BAM_EJECT if eject == "records" else 0
        names = [n.encode() if isinstance(n, str) else bytes(n) for n in ref_names]
        arr = (C.c_char_p * max(len(names), 1))(*names)
        cfg = _lib.BamConfig(floor_len, window, len(names), (_lib.BAM_STORED if stored else 0) | (_lib.BAM_NO_OUTPUT if no_output else 0) | (_lib.BAM_CLIP if clip else 0) | (_lib.BAM_EXTRACT if extract else 0) | (BAM_FROM_TAGS if from_tags else 0) | ej |
                             (_lib.BAM_COLLECT_NAMES if collect_names else 0) | (_lib.BAM_EJECT_NAMED if eject_named else 0) | (_lib.BAM_KEEP_SORTED if keep_sorted else 0) | rp | (_lib.BAM_INDEX if index else 0) |
                             (_lib.BAM_COLLECT_MATES if collect_mates else 0) | (_lib.BAM_FIX_MATES if fix_mates else 0) | (_lib.BAM_STORE_EXTRACT if recstore else 0) |
                             (_lib.BAM_REPORT_REPEATS if repeats else 0) | (_lib.BAM_STORE_OUTPUT if store_output else 0) | (_lib.BAM_CALMD if calmd else 0), arr, first_record, tail_trim)
        h = C.c_void_p()
        ctx._chk(self._L.fadehip_bam_open(ctx._h, C.byref(cfg), C.byref(h)))
        self._h = h
        self._keep = None
        self._names = None
        for ns in (collect_names, eject_named, collect_mates):
            if isinstance(ns, NameSet):
                rc = self._L.fadehip_bam_use_nameset(self._h, ns._h)
                if rc:
                    self.close()
                    ctx._chk(rc)
                self._names = ns  # (the set outlives the stream)
        self._mates = None
        if isinstance(mateset, MateSet):
            rc = self._L.fadehip_bam_use_mateset(self._h, mateset._h)
            if rc:
                self.close()
                ctx._chk(rc)
            self._mates = mateset
        self._recstore = None
        for store in (recstore, store_output):
            if isinstance(store, RecStore):
                rc = self._L.fadehip_bam_use_recstore(self._h, store._h)
                if rc:
                    self.close()
                    ctx._chk(rc)
                self._recstore = store  # (the store outlives the stream)
        self._repeats = None
        if isinstance(repeats, IntervalSet):
            rc = self._L.fadehip_bam_use_intervals(self._h, repeats._h)
            if rc:
                self.close()
                ctx._chk(rc)
            self._repeats = repeats  # (the set outlives the stream)

    def prepare(self, call_bytes):
        """fadehip_bam_prepare: the streams and buffers of calls of call_bytes inflated bytes, made ahead of the first call."""
        self._ctx._chk(self._L.fadehip_bam_prepare(self._h, int(call_bytes)))

    def front(self, members, last=False):
        arr = np.frombuffer(members, dtype=np.uint8) if isinstance(members, (bytes, bytearray, memoryview)) else np.ascontiguousarray(members, dtype=np.uint8)
        self._ctx._chk(self._L.fadehip_bam_front(self._h, arr.ctypes.data if arr.nbytes else None, arr.nbytes, 1 if last else 0))

    def front_raw(self, payload, last=False):
        arr = np.frombuffer(payload, dtype=np.uint8) if isinstance(payload, (bytes, bytearray, memoryview)) else np.ascontiguousarray(payload, dtype=np.uint8)
        self._ctx._chk(self._L.fadehip_bam_front_raw(self._h, arr.ctypes.data if arr.nbytes else None, arr.nbytes, 1 if last else 0))

    def front_raw_ptr(self, ptr, nbytes, last=False):
        """front_raw on memory the caller owns (pinned memory from fadehip_host_alloc: the H2D then runs at PCIe speed)."""
        self._ctx._chk(self._L.fadehip_bam_front_raw(self._h, ptr, nbytes, 1 if last else 0))

    def back(self):
        p, n = C.c_void_p(), C.c_size_t(0)
        self._ctx._chk(self._L.fadehip_bam_back(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value) if n.value else b""

    def back_extract(self):
        """The extract records of the call the last back() finished: (uncompressed BAM records as bytes, their number)."""
        p, n, nr = C.c_void_p(), C.c_size_t(0), C.c_int64(0)
        self._ctx._chk(self._L.fadehip_bam_back_extract(self._h, C.byref(p), C.byref(n), C.byref(nr)))
        return (C.string_at(p, n.value) if n.value else b""), int(nr.value)

    def report(self, which):
        """The rows ("stats" or "clip") of the call the last back() finished: (TSV lines without a header line as bytes, their number)."""
        p, n, nr = C.c_void_p(), C.c_size_t(0), C.c_int64(0)
        flag = {"stats": _lib.BAM_REPORT_STATS, "clip": _lib.BAM_REPORT_CLIP}[which]
        self._ctx._chk(self._L.fadehip_bam_back_report(self._h, flag, C.byref(p), C.byref(n), C.byref(nr)))
        return (C.string_at(p, n.value) if n.value else b""), int(nr.value)

    def index_geometry(self, min_shift, depth):
        """index=True, before the first front(): the calls leave the entries of a CSI of that geometry (CsiBuilder takes them).
        Later: FadeHipError -6; on a stream without index, or a geometry that is not valid: -1."""
        self._ctx._chk(self._L.fadehip_bam_index_geometry(self._h, int(min_shift), int(depth)))

    def back_index(self):
        """index=True: the .bai entries of the call the last back() finished, as index_call_dict gives them."""
        c = _lib.IndexCall()
        self._ctx._chk(self._L.fadehip_bam_back_index(self._h, C.byref(c)))
        return index_call_dict(c)

    def ejected(self):
        """Records not written (eject=...), over the calls back() has taken."""
        n = C.c_int64(0)
        self._ctx._chk(self._L.fadehip_bam_ejected(self._h, C.byref(n)))
        return int(n.value)

    def calmd(self):
        """calmd: (hard-clipped records whose NM / MD were recomputed, ones left alone because they are not subject to the
        rule) over the calls finished so far."""
        n, sk = C.c_int64(0), C.c_int64(0)
        self._ctx._chk(self._L.fadehip_bam_calmd(self._h, C.byref(n), C.byref(sk)))
        return int(n.value), int(sk.value)

    def mates(self):
        """fix_mates: (records fixed, records left alone because their mate's key is ambiguous) over the calls finished so far."""
        n, amb = C.c_int64(0), C.c_int64(0)
        self._ctx._chk(self._L.fadehip_bam_mates(self._h, C.byref(n), C.byref(amb)))
        return int(n.value), int(amb.value)

    def held(self):
        """keep_sorted: (records, bytes) held back on the device behind the most recent finished call."""
        n, b = C.c_int64(0), C.c_int64(0)
        self._ctx._chk(self._L.fadehip_bam_held(self._h, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def totals(self):
        st, nr, no = (C.c_int64 * 8)(), C.c_int64(0), C.c_int64(0)
        self._ctx._chk(self._L.fadehip_bam_totals(self._h, C.byref(st), C.byref(nr), C.byref(no)))
        return [int(x) for x in st], int(nr.value), int(no.value)

    def close(self):
        if self._h:
            self._L.fadehip_bam_close(self._h)
            self._h = None


class NameSet:
    """Context.nameset(): read names on the device.  Records are BAM records (bytes, block_size first) as eject_batch takes."""

    def __init__(self, ctx):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        ctx._chk(self._L.fadehip_nameset_create(ctx._h, C.byref(h)))
        self._h = h

    @staticmethod
    def _cat(records):
        rb = [bytes(r) for r in records]
        off = np.zeros(len(rb) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rb], out=off[1:])
        return (np.frombuffer(b"".join(rb), dtype=np.uint8) if off[-1] else np.zeros(0, np.uint8)), off

    def add_packed(self, recs, rec_off, pick):
        """The names of the records with pick[k] != 0 go into the set (pick None: every record)."""
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        n = len(rec_off) - 1
        if pick is not None:
            pick = np.ascontiguousarray(pick, dtype=np.uint8)
            if len(pick) != n:
                raise ValueError("pick holds one entry per record")
        self._ctx._chk(self._L.fadehip_nameset_add_batch(self._h, n, recs.ctypes.data, rec_off.ctypes.data, pick.ctypes.data if pick is not None else None))

    def add(self, records, pick=None):
        cat, off = self._cat(records)
        self.add_packed(cat, off, pick)

    def contains_packed(self, recs, rec_off):
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        n = len(rec_off) - 1
        hit = np.zeros(n, dtype=np.uint8)
        self._ctx._chk(self._L.fadehip_nameset_contains_batch(self._h, n, recs.ctypes.data, rec_off.ctypes.data, hit.ctypes.data))
        return hit

    def contains(self, records):
        """uint8[n]: 1 where the record's name is in the set."""
        cat, off = self._cat(records)
        return self.contains_packed(cat, off)

    @property
    def count(self):
        """Distinct names in the set."""
        n = C.c_int64(0)
        self._ctx._chk(self._L.fadehip_nameset_count(self._h, C.byref(n)))
        return int(n.value)

    def close(self):
        if self._h:
            self._L.fadehip_nameset_destroy(self._h)
            self._h = None


class RecStore:
    """Context.recstore(): BAM records (bytes, block_size first) collected on the device in any order, sorted once by
    coordinate — (refID as uint32, pos + 1 as uint32), ties in the order added — and drained in that order.  add_batch() and
    streams opened with recstore=... append; sort() closes the store; drain() hands out the next run of records."""

    def __init__(self, ctx):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        ctx._chk(self._L.fadehip_recstore_create(ctx._h, C.byref(h)))
        self._h = h

    def add_packed(self, recs, rec_off, pick=None):
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        n = len(rec_off) - 1
        if pick is not None:
            pick = np.ascontiguousarray(pick, dtype=np.uint8)
            if len(pick) != n:
                raise ValueError("pick holds one entry per record")
        self._ctx._chk(self._L.fadehip_recstore_add_batch(self._h, n, recs.ctypes.data, rec_off.ctypes.data, pick.ctypes.data if pick is not None else None))

    def add_batch(self, records, pick=None):
        """The records with pick[k] != 0 (pick None: every record) are appended, in the order they come."""
        cat, off = NameSet._cat(records)
        self.add_packed(cat, off, pick)

    def count(self):
        """(records, bytes) added so far."""
        n, b = C.c_int64(0), C.c_int64(0)
        self._ctx._chk(self._L.fadehip_recstore_count(self._h, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def sort(self):
        self._ctx._chk(self._L.fadehip_recstore_sort(self._h))

    def index_geometry(self, min_shift, depth):
        """Before the first drain: drain(index=True) hands out the entries of a CSI of that geometry (CsiBuilder takes them)."""
        self._ctx._chk(self._L.fadehip_recstore_index_geometry(self._h, int(min_shift), int(depth)))

    def drain(self, max_payload, raw=False, stored=False, index=False):
        """The next maximal run of records, in final order, of at most max_payload bytes (at least one record): (bytes,
        records) — the records back to back with raw, else BGZF members (stored: uncompressed ones) —, and with index a
        third item, the run's .bai entries as index_call_dict gives them.  0 records: the store is drained."""
        p, n, nr = C.c_void_p(), C.c_size_t(0), C.c_int64(0)
        c = _lib.IndexCall()
        flags = (_lib.RECSTORE_RAW if raw else 0) | (_lib.RECSTORE_STORED if stored else 0) | (_lib.RECSTORE_INDEX if index else 0)
        self._ctx._chk(self._L.fadehip_recstore_drain(self._h, flags, int(max_payload), C.byref(p), C.byref(n), C.byref(nr), C.byref(c) if index else None))
        out = C.string_at(p, n.value) if n.value else b""
        return (out, int(nr.value), index_call_dict(c)) if index else (out, int(nr.value))

    # ---- the sorted main output (streams opened with store_output=...; DESIGN.md 3.8n, tests/sorted_out_model.py)
    def set_budget(self, nbytes=0):
        """The most the store may cost, bytes + 64 per record; 0: derived from the device's free memory.  FADEHIP_RECSTORE_BUDGET
        in the environment overrides either."""
        self._ctx._chk(self._L.fadehip_recstore_set_budget(self._h, int(nbytes)))

    def budget(self):
        """The budget in force (derived, given or from the environment); 0: none set."""
        v = C.c_uint64(0)
        self._ctx._chk(self._L.fadehip_recstore_budget(self._h, C.byref(v)))
        return int(v.value)

    def measure(self, ref_len):
        """ref_len: the header's contig lengths.  From now until reset(), store_output streams add what they write to the
        bucket table, and a call that would take the store over its budget sends it over() instead of failing."""
        arr = np.ascontiguousarray(ref_len, dtype=np.int64)
        self._ctx._chk(self._L.fadehip_recstore_measure(self._h, len(arr), arr.ctypes.data if len(arr) else None))

    def over(self):
        v = C.c_int32(0)
        self._ctx._chk(self._L.fadehip_recstore_over(self._h, C.byref(v)))
        return bool(v.value)

    def resets(self):
        """Reset records (reads a clip left nothing of) among what store_output streams have finished since create or reset."""
        v = C.c_int64(0)
        self._ctx._chk(self._L.fadehip_recstore_resets(self._h, C.byref(v)))
        return int(v.value)

    def histogram(self):
        """(bytes per bucket, records per bucket), as lists."""
        n = C.c_int64(0)
        self._ctx._chk(self._L.fadehip_recstore_histogram(self._h, None, None, C.byref(n)))
        b, r = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64)
        self._ctx._chk(self._L.fadehip_recstore_histogram(self._h, b.ctypes.data, r.ctypes.data, C.byref(n)))
        return [int(x) for x in b], [int(x) for x in r]

    def set_window(self, lo_key, hi_key):
        """store_output streams keep the records whose key lies in [lo_key, hi_key], both inclusive."""
        self._ctx._chk(self._L.fadehip_recstore_set_window(self._h, int(lo_key), int(hi_key)))

    def reset(self, nbytes=0, records=0):
        """Empties the store, sorted or not, and ends measuring; sized once for what is coming."""
        self._ctx._chk(self._L.fadehip_recstore_reset(self._h, int(nbytes), int(records)))

    def close(self):
        if self._h:
            self._L.fadehip_recstore_destroy(self._h)
            self._h = None


class IntervalSet:
    """Context.intervalset(names) / Context.load_bed(path): genomic intervals on the device (fadehip_intervals_*).  An interval
    is (chrom, start, end): chrom an index into names, start and end 0-based half-open, 0 <= start < end <= 2^31 - 1.  add()
    any number of times, in any order; seal() sorts once; overlaps() then answers queries — 1 where the set holds an interval
    of the query's chrom that shares at least one base with [start, end)."""

    def __init__(self, ctx, names, bed=None):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        if bed is not None:
            ctx._chk(self._L.fadehip_intervals_load_bed(ctx._h, os.fsencode(bed), C.byref(h)))
        else:
            nb = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
            arr = (C.c_char_p * max(len(nb), 1))(*nb)
            ctx._chk(self._L.fadehip_intervals_create(ctx._h, len(nb), arr, C.byref(h)))
        self._h = h

    @staticmethod
    def _arrays(chrom, start, end):
        chrom = np.ascontiguousarray(chrom, dtype=np.int32)
        start = np.ascontiguousarray(start, dtype=np.int64)
        end = np.ascontiguousarray(end, dtype=np.int64)
        if not len(chrom) == len(start) == len(end):
            raise ValueError("chrom, start and end hold one entry each per interval")
        return chrom, start, end

    def add(self, chrom, start, end):
        chrom, start, end = self._arrays(chrom, start, end)
        self._ctx._chk(self._L.fadehip_intervals_add(self._h, len(chrom), chrom.ctypes.data, start.ctypes.data, end.ctypes.data))

    def seal(self):
        self._ctx._chk(self._L.fadehip_intervals_seal(self._h))

    def overlaps(self, chrom, start, end):
        """uint8[n]: 1 where the query (chrom[k], start[k], end[k]) hits.  start and end are int64 and may be negative."""
        chrom, start, end = self._arrays(chrom, start, end)
        hit = np.zeros(len(chrom), dtype=np.uint8)
        self._ctx._chk(self._L.fadehip_intervals_overlap_batch(self._h, len(chrom), chrom.ctypes.data, start.ctypes.data, end.ctypes.data, hit.ctypes.data))
        return hit

    def count(self):
        """(intervals, contig names) of the set."""
        n, c = C.c_int64(0), C.c_int32(0)
        self._ctx._chk(self._L.fadehip_intervals_count(self._h, C.byref(n), C.byref(c)))
        return int(n.value), int(c.value)

    def close(self):
        if self._h:
            self._L.fadehip_intervals_destroy(self._h)
            self._h = None


class MateSet:
    """Context.mateset(): placements of clipped records on the device, and the mate fields set from them.  Records are BAM
    records (bytes, block_size first); rs, trim_left and trim_right are what Context.clip_batch takes."""

    def __init__(self, ctx):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        ctx._chk(self._L.fadehip_mateset_create(ctx._h, C.byref(h)))
        self._h = h

    @staticmethod
    def _arrays(records, rs, trim_left, trim_right):
        cat, off = NameSet._cat(records)
        rs = np.ascontiguousarray(rs, dtype=np.uint8)
        tl = np.ascontiguousarray(trim_left, dtype=np.int32)
        tr = np.ascontiguousarray(trim_right, dtype=np.int32)
        if not (len(rs) == len(tl) == len(tr) == len(off) - 1):
            raise ValueError("rs, trim_left and trim_right hold one entry per record")
        return cat, off, rs, tl, tr

    def add_batch(self, records, rs, trim_left, trim_right, pick=None):
        """Every primary paired-end record with pick[k] != 0 (pick None: every one) stores its placement as it leaves."""
        cat, off, rs, tl, tr = self._arrays(records, rs, trim_left, trim_right)
        if pick is not None:
            pick = np.ascontiguousarray(pick, dtype=np.uint8)
            if len(pick) != len(off) - 1:
                raise ValueError("pick holds one entry per record")
        self._ctx._chk(self._L.fadehip_mateset_add_batch(self._h, len(off) - 1, cat.ctypes.data, off.ctypes.data, rs.ctypes.data, tl.ctypes.data,
                                                         tr.ctypes.data, pick.ctypes.data if pick is not None else None))

    def fix_batch(self, records, rs, trim_left, trim_right, out_cap=None):
        """The records clipped as Context.clip_batch clips them, their mate fields set from the map: (list of bytes,
        uint8[n] with 0 untouched, 1 fixed, 2 the mate's key is ambiguous).  out_cap None: room for the clipped records and
        64 bytes of a longer MC value each; a call that needs more says how much and is made again with that."""
        cat, off, rs, tl, tr = self._arrays(records, rs, trim_left, trim_right)
        n = len(off) - 1
        out_off = np.zeros(n + 1, dtype=np.int64)
        fixed = np.zeros(n, dtype=np.uint8)

        def call(cap):
            out = np.zeros(cap, dtype=np.uint8)
            self._ctx._chk(self._L.fadehip_mates_fix_batch(self._h, n, cat.ctypes.data, off.ctypes.data, rs.ctypes.data, tl.ctypes.data, tr.ctypes.data,
                                                           out.ctypes.data, cap, out_off.ctypes.data, fixed.ctypes.data))
            return out

        if out_cap is not None:
            out = call(out_cap)
        else:
            try:
                out = call(len(cat) + 72 * n + 8)
            except FadeHipError as e:
                need = re.search(r"records take (\d+) bytes", str(e))
                if e.code != -1 or not need:
                    raise
                out = call(int(need.group(1)))
        return [out[out_off[k]:out_off[k + 1]].tobytes() for k in range(n)], fixed

    @property
    def count(self):
        """(keys in the map, how many of them are ambiguous)."""
        n, amb = C.c_int64(0), C.c_int64(0)
        self._ctx._chk(self._L.fadehip_mateset_count(self._h, C.byref(n), C.byref(amb)))
        return int(n.value), int(amb.value)

    def close(self):
        if self._h:
            self._L.fadehip_mateset_destroy(self._h)
            self._h = None


def annotate_records(ctx, batch, floor_len=5, window=300):
    """annotateTask over a batch: returns (rs uint8[n], {read_idx: tags}) — anno.d:55-110."""
    rs, aln, _ = ctx.annotate(batch, floor_len, window)
    return rs, format_tags(batch, ctx.contig_names, rs, aln)
