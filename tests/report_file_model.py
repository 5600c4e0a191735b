"""`fade stats` (stats.d:75-186) and `fade stats-clip` (noclip.d:17-73) over the tags of records annotated EARLIER, stated in
plain Python over raw BAM record bytes (block_size first): which records take part, which are skipped, and which fail the
call where the reference would die of a range or conversion error.  The rows themselves are stats_report_ref's (which this
wraps, over a dict made of the record's bytes); the inverted-repeat search is tests/sw_stats_ref.c.  Written from the rules
(DESIGN §3.8i), not from the kernels; the tests hold fadehip_report_batch to it.

Rows are bytes without the line feed (qualities + 33 are bytes as they come, 0xff gives a space)."""
import struct

import samutil
import stats_report_ref as R
import tags_model as tm

MAX_PIECE = 32768  # include/fadehip.h FADEHIP_MAX_LONG_QUERY
INT32 = (-(1 << 31), (1 << 31) - 1)


class ReportFail(Exception):
    """The call fails at `record` (its index); unsupported: FADEHIP_E_UNSUPPORTED instead of FADEHIP_E_INVALID."""

    def __init__(self, record, what, unsupported=False):
        Exception.__init__(self, "record %d: %s" % (record, what))
        self.record, self.what, self.unsupported = record, what, unsupported


def _fields(rec):
    tid, pos, lname, _mapq, _bin, ncig, flag, lseq = struct.unpack_from("<iiBBHHHi", rec, 4)
    p = 36 + lname
    ops = struct.unpack_from("<%dI" % ncig, rec, p)
    p += 4 * ncig
    sq = rec[p:p + (lseq + 1) // 2]
    p += (lseq + 1) // 2
    return dict(tid=tid, pos=pos, flag=flag, lseq=lseq, qname=rec[36:36 + lname - 1].decode("latin-1"), ops=ops,
                seq="".join(samutil.NT16[(sq[k >> 1] >> (4 if k % 2 == 0 else 0)) & 15] for k in range(lseq)), qual=bytes(rec[p:p + lseq]))


def _as_dict(f, ref_names, rs, tags):
    """The dict stats_report_ref reads (samutil.parse_sam's shape) of a record's fields and the tags given."""
    t = {"rs": ("i", str(rs))}
    t.update({k: ("Z", v.decode("latin-1")) for k, v in tags.items()})
    return dict(qname=f["qname"], flag=f["flag"], rname=ref_names[f["tid"]] if 0 <= f["tid"] < len(ref_names) else "*", pos=f["pos"],
                cigar="".join("%d%s" % (o >> 4, "MIDNSHP=XB"[min(o & 15, 9)]) for o in f["ops"]) or "*", seq=f["seq"] or "*",
                qual="".join(chr(q + 33) for q in f["qual"]), tags=t)


def _tags(k, rec, ref_names):
    t = tm.read_tags(rec, ref_names)
    if t is None:
        raise ReportFail(k, "the aux area is not whole fields")
    first = {}
    for tag, ty, val in tm.aux_fields(bytes(rec[tm.aux_offset(rec):])):
        first.setdefault(tag, (ty, val))
    return t, first


def stats_rows(records, ref_names, sample=None):
    """The rows of `fade stats` over the records, in input order, left before right.  Returns [(record, side, row bytes)]."""
    dicts, slots = [], []
    for k, rec in enumerate(records):
        rec = bytes(rec)
        t, first = _tags(k, rec, ref_names)
        if not t["have"] & 1 or not t["rs"] & 6 or not t["have"] & 2:
            continue  # the reference's `continue`: no integer rs, no artifact bit, no am:Z
        rs, f = t["rs"], _fields(rec)
        z = {}
        for tag in (b"as", b"ar", b"ab"):
            if tag not in first or first[tag][0] != "Z":
                raise ReportFail(k, "as, ar or ab is absent or not of type Z")
            z[tag] = first[tag][1][:-1]
        if not any(o & 15 == 4 for o in f["ops"]):
            raise ReportFail(k, "no S op")
        if not 0 <= f["tid"] < len(ref_names):
            raise ReportFail(k, "refID outside the header")
        am = first[b"am"][1][:-1].split(b";", 1) + [b""]
        sides, pieces = [b"", b""], {b"as": [b"", b""], b"ar": [b"", b""]}
        for side in (0, 1):
            if not rs & (2 << side):
                continue
            s = tm.parse_side(am[side], ref_names)
            if s is None or not INT32[0] <= s[1] <= INT32[1]:
                raise ReportFail(k, "a needed am side is malformed or its position is outside int32")
            name, _, cigar = am[side].split(b",", 2)
            if b";" in name:
                raise NotImplementedError("a contig name with ';' in am (stats_report_ref would cut it)")
            sides[side] = name + b"," + str(s[1]).encode() + b"," + cigar
            for tag in (b"as", b"ar"):
                cut = z[tag].split(b";")
                if len(cut) <= side:
                    raise ReportFail(k, "no piece 1 where the right side is needed")
                pieces[tag][side] = cut[side]
            piece = pieces[b"as"][side]
            if not piece:
                raise ReportFail(k, "an empty as piece")
            if len(piece) > MAX_PIECE or len(pieces[b"ar"][side]) > MAX_PIECE:
                raise ReportFail(k, "a piece longer than FADEHIP_MAX_LONG_QUERY", unsupported=True)
            if len(z[b"ab"]) < len(piece):
                raise ReportFail(k, "ab shorter than the piece")
        dicts.append(_as_dict(f, ref_names, rs, {"am": b";".join(sides), "as": b";".join(pieces[b"as"]), "ar": b";".join(pieces[b"ar"]), "ab": z[b"ab"]}))
        slots += [(k, side) for side in (0, 1) if rs & (2 << side)]
    rows = R.stats_rows(dicts, sample)
    assert len(rows) == len(slots)
    return [(k, side, None if None in row else "\t".join(row).encode("latin-1")) for (k, side), row in zip(slots, rows)]


def clip_rows(records, ref_names):
    """The rows of `fade stats-clip` over the records.  Returns [(record, side, row bytes)]."""
    out = []
    for k, rec in enumerate(records):
        rec = bytes(rec)
        t, _ = _tags(k, rec, ref_names)
        if not t["have"] & 1 or not t["rs"] & 1:
            continue
        f = _fields(rec)
        d = _as_dict(f, ref_names, t["rs"], {})
        clips = R.parse_clips(d["cigar"])
        for n in clips:
            if n is not None and f["lseq"] == 0:
                raise ReportFail(k, "a clip on a record with l_seq 0")
            if n is not None and n > f["lseq"]:
                raise ReportFail(k, "a clip longer than l_seq")
        rows = R.clip_rows([d])
        sides = [side for side in (0, 1) if clips[side] is not None]
        assert len(rows) == len(sides)
        out += [(k, side, row.encode("latin-1")) for side, row in zip(sides, rows)]
    return out


def report_text(records, ref_names, which):
    """The report's text as fadehip_report_batch writes it: the rows with their line feeds, no header line."""
    rows = stats_rows(records, ref_names) if which == "stats" else clip_rows(records, ref_names)
    return b"".join(r + b"\n" for _, _, r in rows)
