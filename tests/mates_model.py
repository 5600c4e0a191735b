"""A plain-Python statement of the rule by which mate fields follow the hard clip (fadehip_mateset_* / fadehip_mates_fix_batch,
bam_mates.hpp).  It is this project's own rule, written from the SAM specification — not Picard's
FixMateInformation and not `samtools fixmate`, and no byte equality with either is claimed.  The device is held to it byte
for byte.

A record is a BAM record (bytes, block_size first) with the rs, left trim and right trim `fade out -c` would read from its
tags.  "As it leaves" is what clipRead (filter.d:15-91) makes of it: the suite's statement of that is oracle/pyfilter.clip_read
over the fields, laid out by clip_cases.build_rec — leave() below only carries a record's bytes there and back.

  paired-end   flag & 0x1 and exactly one of 0x40 / 0x80
  key          (l_read_name, the name bytes, flag & 0xC0); the mate key is the same name with the other segment
  primary      flag & 0x900 == 0
  placement    of a record as it leaves: kind (reset, else unmapped by flag & 4, else mapped), refID, pos, reverse (flag & 0x10),
               end = pos + max(1, reference bases of the leaving CIGAR), the CIGAR as SAM text ("" without ops),
               five = end - 1 when reverse, else pos

  the map      every picked primary paired-end record inserts its placement under its key (paired-end and primary by the
               flag it came in with); a second insert under a key marks the entry ambiguous, whatever the values
  the fix      a record that LEAVES paired-end (a reset record has flag 0) and whose mate key is in the map and not
               ambiguous gets its mate fields from the mate's placement — fix() below says how
"""
import struct

import clip_cases as cc

AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


# ------------------------------------------------------------------------------------------------ a record as it leaves
def leave(rec, rs, tl, tr):
    """(bytes of the record as `fade out -c` writes it, True when it was reset)."""
    if not rs & 6:
        return bytes(rec), False
    from oracle import pyfilter
    d = cc.decode_rec(rec)
    am = ("x,7,%dM" % tl if rs & 2 else "") + ";" + ("x,7,%dM" % tr if rs & 4 else "")
    new = pyfilter.clip_read(dict(qname=d["qname"], flag=d["flag"], rname="x", pos=d["pos"], mapq=d["mapq"], cigar=d["cigar"], seq=d["seq"],
                                  qual=d["qual"], tags={"am": ("Z", am)}, tag_order=["am"]), rs, "x")
    if new["tags"] == {}:  # reset: a zero-filled record that keeps name, bases and qualities, and no aux area
        return cc.build_rec(d["qname"], 0, 0, 0, 0, 0, 0, 0, "*", new["seq"], new["qual"]), True
    return cc.build_rec(d["qname"], d["tid"], new["pos"], d["mapq"], d["flag"], d["mtid"], d["mpos"], d["tlen"], new["cigar"], new["seq"],
                        new["qual"], d["aux"]), False


def flag_of(rec):
    return struct.unpack_from("<H", rec, 18)[0]


def paired_end(flag):
    return bool(flag & 1) and (flag & 0xC0) in (0x40, 0x80)


def key(rec, other=False):
    ln = rec[12]
    return ln, bytes(rec[36:36 + ln]), (flag_of(rec) & 0xC0) ^ (0xC0 if other else 0)


def placement(left, reset):
    """The placement of a record that left as `left`."""
    if reset:
        return dict(kind="reset")
    d = cc.decode_rec(left)
    ops = cc.cigar_ops(d["cigar"])
    reverse = bool(d["flag"] & 0x10)
    end = d["pos"] + max(1, sum(n for n, c in ops if c in "MDN=X"))
    return dict(kind="unmapped" if d["flag"] & 4 else "mapped", tid=d["tid"], pos=d["pos"], reverse=reverse, end=end,
                cigar_text="".join("%d%s" % o for o in ops), five=end - 1 if reverse else d["pos"])


# ------------------------------------------------------------------------------------------------ the map
def insert(mates, records, rs, tl, tr, pick=None):
    """One add call: mates maps key -> placement, or to None once the key is ambiguous."""
    for k, rec in enumerate(records):
        f = flag_of(rec)
        if (pick is not None and not pick[k]) or not paired_end(f) or f & 0x900:
            continue
        mates[key(rec)] = None if key(rec) in mates else placement(*leave(rec, rs[k], tl[k], tr[k]))
    return mates


def count(mates):
    return len(mates), sum(1 for v in mates.values() if v is None)


# ------------------------------------------------------------------------------------------------ the fix
def aux_fields(aux):
    """(start, end) of every whole aux field, in order; the walk ends at a field that is not whole."""
    out, q = [], 0
    while q + 3 <= len(aux):
        t = chr(aux[q + 2])
        if t in AUX_SIZE:
            e = q + 3 + AUX_SIZE[t]
        elif t in "ZH":
            z = aux.find(b"\0", q + 3)
            e = z + 1 if z >= 0 else len(aux) + 1
        elif t == "B" and q + 8 <= len(aux) and chr(aux[q + 3]) in AUX_SIZE:
            e = q + 8 + AUX_SIZE[chr(aux[q + 3])] * struct.unpack_from("<I", aux, q + 4)[0]
        else:
            break
        if e > len(aux):
            break
        out.append((q, e))
        q = e
    return out


def first_mc(aux):
    """(start, end) of the first aux field MC of type Z, or None."""
    return next(((q, e) for q, e in aux_fields(aux) if aux[q:q + 3] == b"MCZ"), None)


def fix(left, v):
    """The record that left as `left` (paired-end, not reset) with its mate fields set from the mate's placement v, and what
    became of its first MC:Z field: None (it has none), "replaced" or "removed"."""
    d = cc.decode_rec(left)
    own = placement(left, False)
    flag, aux = d["flag"], d["aux"]
    if v["kind"] == "reset":
        flag = (flag | 0x8) & ~(0x20 | 0x2)
        mtid, mpos, tlen, text = d["tid"], d["pos"], 0, ""
    else:
        flag = (flag & ~(0x20 | 0x8)) | (0x20 if v["reverse"] else 0) | (0x8 if v["kind"] == "unmapped" else 0)
        mtid, mpos, tlen = v["tid"], v["pos"], 0
        if own["kind"] == "mapped" and v["kind"] == "mapped" and own["tid"] >= 0 and v["tid"] >= 0 and own["tid"] == v["tid"]:
            dist = v["five"] - own["five"]
            tlen = dist + 1 if dist >= 0 else dist - 1
        text = v["cigar_text"] if v["kind"] == "mapped" else ""
    mc = first_mc(aux)
    if mc:
        aux = aux[:mc[0]] + (b"MCZ" + text.encode() + b"\0" if text else b"") + aux[mc[1]:]
    body = bytearray(left[4:len(left) - len(d["aux"])]) + aux
    struct.pack_into("<H", body, 14, flag)
    struct.pack_into("<iii", body, 20, mtid, mpos, ((tlen + (1 << 31)) % (1 << 32)) - (1 << 31))  # (the field's 32 bits)
    return struct.pack("<I", len(body)) + bytes(body), (None if not mc else "replaced" if text else "removed")


CLASSES = ("fixed", "reset_mate", "mc_replaced", "mc_removed", "ambiguous", "untouched")


def fix_batch(mates, records, rs, tl, tr):
    """(the records as they leave with their mate fields set, fixed[] — 0 untouched, 1 fixed, 2 the mate key is ambiguous,
    the number of records in each of CLASSES)."""
    out, fixed = [], []
    classes = dict.fromkeys(CLASSES, 0)
    for k, rec in enumerate(records):
        left, reset = leave(rec, rs[k], tl[k], tr[k])
        mk = key(left, other=True)
        if reset or not paired_end(flag_of(left)) or mk not in mates:
            state = 0
            classes["untouched"] += 1
        elif mates[mk] is None:
            state = 2
            classes["ambiguous"] += 1
        else:
            state = 1
            left, mc = fix(left, mates[mk])
            classes["fixed"] += 1
            classes["reset_mate"] += mates[mk]["kind"] == "reset"
            classes["mc_replaced"] += mc == "replaced"
            classes["mc_removed"] += mc == "removed"
        out.append(left)
        fixed.append(state)
    return out, fixed, classes


# ------------------------------------------------------------------------------------------------ mate information to start from
def pair_up(records, mc=lambda rec: True):
    """The records with mate fields written from UNCLIPPED geometry by the rule above — every primary paired-end record
    inserts with rs 0, then every record is fixed — and, where mc(record) says so and the mate is mapped with a CIGAR, an
    MC:Z field appended to a record that has none.  (The golden SAMs carry RNEXT *, PNEXT 0, TLEN 0 and no MC.)"""
    zero = [0] * len(records)
    mates = insert({}, records, zero, zero, zero)
    out = []
    for rec in records:
        v = mates.get(key(rec, other=True)) if paired_end(flag_of(rec)) else None
        if v is not None:
            rec, had = fix(rec, v)
            if had is None and mc(rec) and v["kind"] == "mapped" and v["cigar_text"]:
                rec = struct.pack("<I", len(rec) + len(v["cigar_text"])) + rec[4:] + b"MCZ" + v["cigar_text"].encode() + b"\0"
        out.append(bytes(rec))
    return out
