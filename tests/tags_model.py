"""A plain-Python statement of the tag reader (fadehip_tags_batch): what `fade out` and `fade extract` read back out of a
record annotated earlier — rs as rs_of takes it (tag.to!ubyte of an integer field), am as extract_main cuts it
("left;right" at the first ';', a side "name,pos,cigar"), the CIGAR as parse_cigar_string reads it — and the shapes the clip,
eject and extract calls take.  Written from that grammar, not from the kernel; tests hold both to it.

Beside it, restatements of the three consumers driven by those arrays instead of by the tag text (clip_by_trims,
eject_keep, extract_lines), and the BAM <-> SAM-dict helpers the tests share."""
import os
import random
import re
import struct

import numpy as np

import clip_cases as cc
import samutil

OPS = "MIDNSHP=XB"
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X
INT32_MAX = (1 << 31) - 1
_SIZES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_POS = re.compile(rb"[+-]?[0-9]+")
_PAIR = re.compile(rb"([0-9]+)([MIDNSHP=XB])")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def aux_offset(rec):
    """Where the aux area of a BAM record (bytes, block_size first) starts."""
    lname, = struct.unpack_from("<B", rec, 12)
    ncig, = struct.unpack_from("<H", rec, 16)
    lseq, = struct.unpack_from("<i", rec, 20)
    return 36 + lname + 4 * ncig + (lseq + 1) // 2 + lseq


def aux_fields(aux):
    """[(tag, type, value bytes)] of an aux area, or None when it is not whole fields."""
    out, p, n = [], 0, len(aux)
    while p < n:
        if p + 3 > n:
            return None
        tag, ty = aux[p:p + 2], chr(aux[p + 2])
        q = p + 3
        if ty in _SIZES:
            e = q + _SIZES[ty]
        elif ty in "ZH":
            e = aux.find(b"\0", q)
            if e < 0:
                return None
            e += 1
        elif ty == "B":
            if q + 5 > n or chr(aux[q]) not in _SIZES:  # (the device walker sizes an element by the same table as a scalar)
                return None
            e = q + 5 + _SIZES[chr(aux[q])] * struct.unpack_from("<I", aux, q + 1)[0]
        else:
            return None
        if e > n:
            return None
        out.append((tag, ty, aux[q:e]))
        p = e
    return out


def parse_side(text, ref_names):
    """One side of am (bytes) -> None when it is not well-formed, else (tid, pos, ops)."""
    f = text.split(b",", 2)
    if len(f) < 3:
        return None
    name, pos, cigar = f
    if not _POS.fullmatch(pos) or not -(1 << 63) <= int(pos) < (1 << 63):
        return None
    ops, at = [], 0
    for m in _PAIR.finditer(cigar):
        if m.start() != at or int(m.group(1)) >= 1 << 28:
            return None
        ops.append((int(m.group(1)) << 4) | OPS.index(m.group(2).decode()))
        at = m.end()
    if at != len(cigar):  # a third comma, a lower-case letter, a count without an op, an op without a count
        return None
    names = [x.encode() if isinstance(x, str) else bytes(x) for x in ref_names]
    tid = names.index(name) if name and name in names else -1
    return tid, int(pos), ops


def read_tags(rec, ref_names):
    """One record -> dict(rs, have, sides=[left, right]) with a side None or (tid, pos, ops); None: the aux area is damaged."""
    fields = aux_fields(bytes(rec[aux_offset(rec):]))
    if fields is None:
        return None
    rs, have, sides = 0, 0, [None, None]
    first = {}
    for tag, ty, val in fields:
        first.setdefault(tag, (ty, val))
    if b"rs" in first and first[b"rs"][0] in "cCsSiI":
        rs, have = first[b"rs"][1][0], have | 1
    if b"am" in first and first[b"am"][0] == "Z":
        have |= 2
        am = first[b"am"][1][:-1]
        cut = am.split(b";", 1)
        for side, text in enumerate(cut + [b""] * (2 - len(cut))):
            sides[side] = parse_side(text, ref_names)
            if sides[side] is not None:
                have |= 4 << side
    return dict(rs=rs, have=have, sides=sides)


def tags_batch(records, ref_names):
    """The arrays of fadehip_tags_batch over a list of records."""
    n = len(records)
    o = dict(rs=np.zeros(n, np.uint8), have=np.zeros(n, np.uint8), trim_left=np.zeros(n, np.int32), trim_right=np.zeros(n, np.int32),
             art_tid=np.full(2 * n, -1, np.int32), art_pos=np.zeros(2 * n, np.int64), cig_off=np.zeros(2 * n + 1, np.int64))
    cig = []
    for k, rec in enumerate(records):
        t = read_tags(rec, ref_names)
        if t is None:
            raise ValueError("record %d: the aux area is not whole fields" % k)
        o["rs"][k], o["have"][k] = t["rs"], t["have"]
        for side, s in enumerate(t["sides"]):
            if s is not None:
                o["art_tid"][2 * k + side], o["art_pos"][2 * k + side] = s[0], s[1]
                cig.extend(s[2])
                o["trim_right" if side else "trim_left"][k] = min(sum(x >> 4 for x in s[2] if (x & 15) in REF_OPS), INT32_MAX)
            o["cig_off"][2 * k + side + 1] = len(cig)
    o["cig"] = np.array(cig, dtype=np.uint32)
    return o


# ---------------------------------------------------------------- the consumers, from the arrays
def clip_by_trims(rec, rs, trim_left, trim_right, contig0):
    """filter.d:15-91 on a samutil.parse_sam dict, with the two lengths given instead of parsed from am."""
    ops = [[n, c] for n, c in cc.cigar_ops(rec["cigar"])]
    pos, seq, qual = rec["pos"], rec["seq"], rec["qual"]
    ref = lambda: sum(n for n, c in ops if c in "MDN=X")

    def reset():
        return dict(qname=rec["qname"], flag=0, rname=contig0, pos=0, mapq=0, cigar="*", rnext="=", pnext=1, tlen=0, seq=seq, qual=qual,
                    tags={}, tag_order=[])

    for bit, to_trim, end in ((2, trim_left, 0), (4, trim_right, -1)):
        if not rs & bit:
            continue
        if to_trim >= ref():
            return reset()
        hard = 0
        while to_trim:
            c = ops[end][1]
            if c in "MIS=X":
                seq, qual, hard = (seq[1:], qual[1:], hard + 1) if end == 0 else (seq[:-1], qual[:-1], hard + 1)
            if c in "MDN=X":
                pos += 1 if end == 0 else 0
                to_trim -= 1
            ops[end][0] -= 1
            if ops[end][0] == 0:
                ops.pop(end)
        ops.insert(0, [hard, "H"]) if end == 0 else ops.append([hard, "H"])
    new = dict(rec)
    new["cigar"], new["seq"], new["qual"], new["pos"] = "".join("%d%s" % (n, c) for n, c in ops), seq, qual, pos
    return new


def eject_keep(qnames, rs, have, grouped):
    """filter.d:209-265: which records plain `fade out` writes.  Not grouped, a record without rs is not written; grouped, it
    counts as clean."""
    art = [bool(h & 1) and bool(v & 6) for v, h in zip(rs, have)]
    if not grouped:
        return [bool(h & 1) and not a for a, h in zip(art, have)]
    keep, k = [], 0
    while k < len(qnames):
        e = k
        while e < len(qnames) and qnames[e] == qnames[k]:
            e += 1
        keep += [not any(art[k:e])] * (e - k)
        k = e
    return keep


def extract_lines(recs, t, ref_names):
    """remap.d:29-85 from the arrays: the SAM lines of `fade extract` (parse_sam dicts in, oracle/pyremap's lines out)."""
    from oracle import pyremap
    out = []
    for k, r in enumerate(recs):
        if not t["have"][k] & 1 or not t["rs"][k] & 6 or not t["have"][k] & 2:
            continue
        for side in range(2):
            if not t["rs"][k] & (2 << side):
                continue
            s = 2 * k + side
            if not t["have"][k] & (4 << side):
                raise ValueError("malformed am tag (record %d)" % k)
            tid = int(t["art_tid"][s])
            cigar = "".join("%d%s" % (x >> 4, OPS[x & 15]) for x in t["cig"][t["cig_off"][s]:t["cig_off"][s + 1]])
            out.append("\t".join([r["qname"], str(0 if r["flag"] & 0x10 else 0x10), ref_names[tid], str(int(t["art_pos"][s]) + 1), "0", cigar,
                                  "=" if tid == 0 else ref_names[0], "1", "0", pyremap.reverse_complement(r["seq"]), r["qual"][::-1]]))
    return out


# ---------------------------------------------------------------- BAM bytes <-> parse_sam dicts
def aux_of(rec):
    """The aux bytes of a parse_sam dict's tags (types i, Z, A): integers in the narrowest type, as htslib writes them."""
    out = b""
    for k in rec["tag_order"]:
        ty, v = rec["tags"][k]
        if ty == "i":
            x = int(v)
            for code, lo, hi in (("C", 0, 255), ("c", -128, 127), ("S", 0, 65535), ("s", -32768, 32767), ("I", 0, (1 << 32) - 1), ("i", -(1 << 31), INT32_MAX)):
                if lo <= x <= hi:
                    out += k.encode() + code.encode() + struct.pack("<" + {"C": "B", "c": "b", "S": "H", "s": "h", "I": "I", "i": "i"}[code], x)
                    break
        elif ty == "A":
            out += k.encode() + b"A" + v.encode()
        else:
            assert ty == "Z", ty
            out += k.encode() + b"Z" + v.encode() + b"\0"
    return out


def sam_to_bam(rec, ref_names):
    """A parse_sam dict -> its BAM record (block_size first), laid out by clip_cases.build_rec."""
    tid = ref_names.index(rec["rname"]) if rec["rname"] != "*" else -1
    mtid = tid if rec["rnext"] == "=" else ref_names.index(rec["rnext"]) if rec["rnext"] != "*" else -1
    return cc.build_rec(rec["qname"], tid, rec["pos"], rec["mapq"], rec["flag"], mtid, rec["pnext"] - 1, rec["tlen"], rec["cigar"], rec["seq"],
                        rec["qual"], aux_of(rec))


def bam_to_line(b, ref_names):
    """A BAM record -> the SAM line oracle/pyfilter writes for it."""
    d = cc.decode_rec(b)
    tags = []
    for tag, ty, val in aux_fields(d["aux"]):
        if ty in "cCsSiI":
            tags.append("%s:i:%d" % (tag.decode(), struct.unpack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], val)[0]))
        else:
            assert ty in "ZA", ty
            tags.append("%s:%s:%s" % (tag.decode(), ty, val.rstrip(b"\0").decode()))
    rname = ref_names[d["tid"]] if d["tid"] >= 0 else "*"
    rnext = "*" if d["mtid"] < 0 else "=" if d["mtid"] == d["tid"] else ref_names[d["mtid"]]
    return "\t".join([d["qname"], str(d["flag"]), rname, str(d["pos"] + 1), str(d["mapq"]), d["cigar"], rnext, str(d["mpos"] + 1), str(d["tlen"]),
                      d["seq"], d["qual"]] + tags)


# ---------------------------------------------------------------- the annotated golden sets
def annotated(tag):
    """(contig names, parse_sam dicts, BAM records) of a golden set with its expected tags, as test_cli_extract builds it."""
    lines = open(os.path.join(GOLD, tag + ".sam")).read().splitlines()
    exp = [l.rstrip("\n").split("\t") for l in open(os.path.join(GOLD, tag + ".expected.tsv")) if not l.startswith("#")]
    out, k = [], 0
    for l in lines:
        if not l.startswith("@"):
            e = exp[k]
            k += 1
            l += "\trs:i:%s" % e[2]
            if e[3]:
                l += "\tam:Z:%s\tas:Z:%s\tar:Z:%s\tab:Z:%s" % (e[3], e[4], e[5], e[6])
        out.append(l)
    header, recs = samutil.parse_sam("\n".join(out) + "\n")
    names = [dict(x.split(":", 1) for x in h.split("\t")[1:])["SN"] for h in header if h.startswith("@SQ")]
    return names, recs, [sam_to_bam(r, names) for r in recs]


def orders(recs, bams):
    """The set as it is (name-sorted: `fade out` takes groups) and shuffled until its first ten names are out of order."""
    yield "sorted", recs, bams
    from oracle import pyfilter
    idx = list(range(len(recs)))
    rng = random.Random(20261019)
    while True:
        rng.shuffle(idx)
        first = [recs[i]["qname"] for i in idx[:10]]
        if any(pyfilter.numerically_aware_cmp(first[k], first[k - 1]) < 0 for k in range(1, 10)):
            break
    yield "shuffled", [recs[i] for i in idx], [bams[i] for i in idx]
