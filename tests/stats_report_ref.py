"""Restatement of `fade stats` (stats.d:75-186) and `fade stats-clip` (noclip.d:17-73) over annotated records (the dicts of
samutil.parse_sam / bam_to_sam_records), for the tests of `fade annotate --stats-tsv / --clip-tsv`.  The inverted-repeat
search runs on the CPU restatement tests/sw_stats_ref.c."""
import re

import numpy as np

import sw_stats_ref as S

STATS_HEADER = ("qname\trname\tpos\tcigar\tart_start\tart_end\taln_rname\taln_start\taln_end\tart_cigar\tstemloop\t"
                "stemloop_rc\tpredicted_inverted_repeat\tIR_identity\tavgbq\tart_avgbq\tart_bq\tIR_bq\tflagbinary\tflag\tstrand")
CLIP_HEADER = "qname\tsc_q_scores\tsc_seq\tsc_avg_bq\tavg_bq\tart_status"
REF_OPS = set("MDN=X")  # include/fadehip.h FADEHIP_REF_CONSUMING_OPS


def cigar_ops(c):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", c)] if c != "*" else []


def aligned_length(c):
    return sum(n for n, op in cigar_ops(c) if op in REF_OPS)


def ratio(num, den):
    """D's to!string of float(num) / float(den), printed as %g (nan, inf)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.float32(num) / np.float32(den)
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "inf"
    return "%g" % float(v)


def quals(r):
    n = len(r["seq"]) if r["seq"] != "*" else 0
    return [0xFF] * n if r["qual"] == "*" else [ord(c) - 33 for c in r["qual"]]


def parse_clips(c):
    """util.d:37-62 with its quirk: `first` stays set while the ops are soft clips."""
    clips = [None, None]
    first = True
    for n, op in cigar_ops(c):
        if op == "H":
            continue
        sc = op == "S"
        if first and not sc:
            first = False
        elif first and sc:
            clips[0] = n
        elif sc:
            clips[1] = n
    return clips


def clip_rows(recs):
    out = []
    for r in recs:
        rs = int(r["tags"]["rs"][1])
        if not rs & 1:
            continue
        q = quals(r)
        for side, n in enumerate(parse_clips(r["cigar"])):
            if n is None:
                continue
            sl = slice(0, n) if side == 0 else slice(len(q) - n, len(q))
            sq = q[sl]
            out.append("\t".join([r["qname"], "".join(chr((x + 33) & 0xFF) for x in sq), r["seq"][sl], ratio(sum(sq), n),
                                  ratio(sum(q), len(q)), "true" if rs & (2 if side == 0 else 4) else "false"]))
    return out


def stats_rows(recs, sample=None):
    """Rows in output order.  sample: optional set of row numbers whose SW columns are checked (others get None there)."""
    pend, qs, rfs = [], [], []
    for r in recs:
        t = r["tags"]
        rs = int(t["rs"][1])
        if not rs & 6 or "am" not in t:
            continue
        am = t["am"][1].split(";")
        ops = cigar_ops(r["cigar"])
        s_ops = [n for n, op in ops if op == "S"]
        al = aligned_length(r["cigar"])
        ab = t["ab"][1]
        q = quals(r)
        for side in (0, 1):
            if not rs & (2 << side):
                continue
            f = am[side].split(",")
            sl = t["as"][1].split(";")[side]
            slrc = t["ar"][1].split(";")[side]
            pos = r["pos"]
            if side == 0:
                a0, a1 = pos - s_ops[0], pos
            else:
                a0, a1 = pos + al, pos + al + s_ops[-1]
            bq = ab[:len(sl)] if side == 0 else ab[len(ab) - len(sl):]
            row = [r["qname"], r["rname"], str(pos), r["cigar"], str(a0), str(a1), f[0], f[1],
                   str(int(f[1]) + aligned_length(f[2])), f[2], sl, slrc]
            k = len(pend)
            if sample is None or k in sample:
                qs.append(sl[:(3 * len(sl) + 2) // 4])
                rfs.append(slrc)
            pend.append((row, sl, bq, q, rs, r["flag"], sample is None or k in sample))
    res = S.stats_batch(qs, rfs) if qs else []
    out, j = [], 0
    for row, sl, bq, q, rs, flag, have in pend:
        if have:
            e = int(res[j]["end_query"]) + 1
            ir, ident, irbq = sl[:e], ratio(int(res[j]["matches"]), int(res[j]["length"])), bq[:e]
            j += 1
        else:
            ir = ident = irbq = None
        out.append(row + [ir, ident, ratio(sum(q), len(q)), ratio(sum(bq.encode()), len(sl)), bq, irbq,
                          format(rs, "08b"), str(rs), "+" if flag & 16 else "-"])
    return out
