"""Constructed records for the hard clip of `fade annotate --clip` / fadehip_clip_batch (filter.d:15-91 clipRead), shared by
tests/test_cli_clip.py (host clip_read, no GPU) and tests/test_gpu_clip_batch.py (the device function).

The arbiter is oracle/pyfilter.clip_read; the BAM bytes are laid out here the way the host's build_rec lays them out
(fixed fields, bin = reg2bin over the span, name, CIGAR, 4-bit bases with a zero pad nibble, qualities, aux)."""
import re
import struct

import numpy as np

NT16 = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=XB"
CONTIGS = ["ctgA", "ctgB"]
_RC, _QC = set("MDN=X"), set("MIS=X")


def reg2bin(beg, end):
    end -= 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return base + (beg >> sh)
    return 0


def cigar_ops(s):
    return [] if s == "*" else [(int(n), c) for n, c in re.findall(r"(\d+)([MIDNSHP=XB])", s)]


def build_rec(qname, tid, pos, mapq, flag, mtid, mpos, tlen, cigar, seq, qual, aux=b""):
    """A BAM record (block_size first).  cigar and seq as SAM text ("*": none), qual as phred+33 text."""
    ops = cigar_ops(cigar)
    seq = "" if seq == "*" else seq
    lq = len(seq)
    reflen = sum(n for n, c in ops if c in _RC)
    p0 = 0 if pos < 0 else pos
    name = qname.encode() + b"\0"
    packed = bytearray((lq + 1) // 2)
    for k, ch in enumerate(seq):
        packed[k >> 1] |= NT16.index(ch) << (4 if k % 2 == 0 else 0)
    # (bin is a 16-bit field: from 997 Mb on a level-14 bin number no longer fits and the field holds its low 16 bits)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), mapq, reg2bin(p0, p0 + (reflen if reflen > 0 else 1)) & 0xffff, len(ops) & 0xffff,
                       flag, lq, mtid, mpos, tlen)
    body += name + b"".join(struct.pack("<I", (n << 4) | OPS.index(c)) for n, c in ops) + bytes(packed)
    body += bytes(ord(c) - 33 for c in qual[:lq]) + aux
    return struct.pack("<I", len(body)) + body


def decode_rec(b):
    """The fields of one BAM record (block_size first) and its aux bytes."""
    bs, = struct.unpack_from("<I", b, 0)
    assert bs + 4 == len(b), (bs, len(b))
    tid, pos, lqn, mapq, bin_, ncig, flag, lseq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", b, 4)
    p = 36
    qname = b[p:p + lqn - 1].decode()
    p += lqn
    cig = "".join("%d%s" % (c >> 4, OPS[c & 15]) for c in struct.unpack_from("<%dI" % ncig, b, p)) or "*"
    p += 4 * ncig
    sq = b[p:p + (lseq + 1) // 2]
    seq = "".join(NT16[(sq[k >> 1] >> (4 if k % 2 == 0 else 0)) & 15] for k in range(lseq))
    pad = (sq[-1] & 15) if lseq % 2 else 0
    p += (lseq + 1) // 2
    qual = "".join(chr(x + 33) for x in b[p:p + lseq])
    p += lseq
    return dict(qname=qname, tid=tid, pos=pos, mapq=mapq, bin=bin_, flag=flag, mtid=mtid, mpos=mpos, tlen=tlen, cigar=cig, seq=seq,
                qual=qual, pad=pad, aux=bytes(b[p:]))


def _big_aux(rng, nbytes):
    text = bytes(rng.integers(33, 127, size=nbytes, dtype=np.uint8))
    arr = rng.integers(0, 60000, size=37)
    return (b"NMC\x05" + b"XZZ" + text + b"\0" + b"XBBS" + struct.pack("<I", len(arr)) + struct.pack("<%dH" % len(arr), *arr) +
            b"XAAq" + b"XIi" + struct.pack("<i", -77))


# (name, cigar, rs, trim_left, trim_right, aux: None / "small" / bytes of a big one, sam: goes through the SAM text of the CLI test)
_SPECS = [
    # one side, odd and even clips, odd and even remaining l_seq
    ("left_odd_clip_odd_rest", "10S40M", 2, 7, 0, "small"),       # 17 bases go, 33 stay
    ("left_even_clip_even_rest", "10S40M", 2, 6, 0, None),        # 16 go, 34 stay
    ("left_odd_clip_even_rest", "10S41M", 2, 7, 0, "small"),      # 17 go, 34 stay
    ("left_even_clip_odd_rest", "10S41M", 2, 6, 0, None),         # 16 go, 35 stay
    ("right_odd", "40M10S", 4, 0, 5, "small"),
    ("right_even", "40M10S", 4, 0, 6, None),
    ("left_zero_trim", "10S40M", 2, 0, 0, "small"),               # 0H in front, nothing eaten
    ("right_zero_trim", "40M10S", 4, 0, 0, None),
    # both sides: the right against what the left step left
    ("both_many_ops", "5S30M2I10M5S", 6, 8, 12, "small"),
    ("both_one_op", "3S20M3S", 6, 5, 5, None),
    ("both_meet_in_one_op", "20M", 6, 12, 7, "small"),            # 8M left after the left step, 7 < 8
    ("both_odd_left_odd_right", "7S31M6S", 6, 4, 3, None),
    # resets
    ("reset_left_equal", "5S10M", 2, 10, 0, "small"),             # to_trim == aligned length
    ("left_aligned_minus_one", "5S10M", 2, 9, 0, "small"),        # to_trim == aligned length - 1
    ("reset_left_beyond", "5S10M3S", 6, 25, 1, None),
    ("reset_right_equal", "10M5S", 4, 0, 10, "small"),
    ("right_aligned_minus_one", "10M5S", 4, 0, 9, None),
    ("reset_right_after_left", "3S20M", 6, 12, 8, "small"),       # alone the right would clip (8 < 20); after the left: 8 == 8
    ("reset_right_after_odd_left", "4S21M2S", 6, 13, 9, None),
    ("reset_no_cigar", "*", 2, 3, 0, "small"),
    # every op at the eaten end
    ("lead_H", "3H5S20M", 2, 4, 0, "small"),
    ("lead_I", "4I20M", 2, 3, 0, None),
    ("lead_S_I", "2S3I20M", 2, 1, 0, "small"),
    ("D_partly", "5S3M2D20M", 2, 4, 0, None),
    ("D_to_zero", "5S3M2D20M", 2, 5, 0, "small"),
    ("M_to_zero_before_D", "5S3M2D20M", 2, 3, 0, None),
    ("M_to_zero_before_I", "5S3M2I20M", 2, 3, 0, "small"),        # the I behind the last base eaten stays
    ("N_partly", "5S3M100N20M", 2, 50, 0, None),
    ("N_whole", "5S3M100N20M", 2, 104, 0, "small"),
    ("lead_P", "5S2P20M", 2, 3, 0, None),
    ("P_and_I_inside", "3M2P3I20M", 2, 4, 0, "small"),
    ("eq_and_X", "5S10=1X10=", 2, 11, 0, None),
    ("trail_H", "20M5S3H", 4, 0, 2, "small"),
    ("trail_D_partly", "20M2D3M5S", 4, 0, 4, None),
    ("trail_D_to_zero", "20M2D3M5S", 4, 0, 5, "small"),
    ("trail_I_P", "20M3I2P3M", 4, 0, 4, None),
    ("trail_N", "20M100N3M5S", 4, 0, 60, "small"),
    ("trail_M_to_zero_before_I", "20M2I3M5S", 4, 0, 3, None),
    # no artifact bits: the record passes as it is
    ("untouched_rs0", "10S40M", 0, 9, 9, "small"),
    ("untouched_rs1", "10S40M", 1, 9, 9, None),
    ("untouched_rs57", "10S40M", 57, 9, 9, "small"),
    # short and long records, no aux and a few KB of it
    ("lseq1_keep", "1M", 2, 0, 0, None),
    ("lseq1_reset", "1M", 2, 1, 0, "small"),
    ("lseq2_left", "2M", 6, 1, 0, None),
    ("lseq2_right", "2M", 4, 0, 1, "small"),
    ("lseq2_S", "1S1M", 2, 0, 0, None),
    ("long_both_big_aux", "100S500M", 6, 33, 44, "big"),
    ("long_odd_left_no_aux", "101S500M77S", 6, 20, 31, None),
    ("long_reset_big_aux", "100S500M", 4, 0, 500, "big"),
    ("long_many_ops", "9S" + "7M1I6M2D" * 40 + "11S", 6, 203, 190, "big"),
]


def cases(sam_only=False):
    """dicts: name, rec (the record as tests/samutil.parse_sam would give it, with an am tag of the two lengths), aux (its
    aux BYTES in the BAM form, unrelated to rec["tags"]), rs, tl, tr."""
    rng = np.random.default_rng(20240517)
    out = []
    for k, (name, cigar, rs, tl, tr, aux) in enumerate(_SPECS):
        ops = cigar_ops(cigar)
        lq = sum(n for n, c in ops if c in _QC) if ops else 9
        seq = "".join("ACGTN"[x] for x in rng.integers(0, 5, size=lq))
        qual = "".join(chr(33 + int(x)) for x in rng.integers(0, 42, size=lq))
        am = ("%s,7,%dM" % (CONTIGS[k % 2], tl) if rs & 2 else "") + ";" + ("%s,7,%dM" % (CONTIGS[k % 2], tr) if rs & 4 else "")
        rec = dict(qname="case_%s" % name, flag=[0, 16, 99, 147, 2048][k % 5], rname=CONTIGS[k % 2], pos=1000 + 17 * k, mapq=10 + k % 50,
                   cigar=cigar, rnext="=", pnext=3000 + k, tlen=(-1) ** k * (100 + k), seq=seq, qual=qual,
                   tags={"rs": ("i", str(rs)), "am": ("Z", am)}, tag_order=["rs", "am"])
        a = b"" if aux is None else b"NMC\x03XSZhello\0" if aux == "small" else _big_aux(rng, 3000 + 111 * k)
        if sam_only and aux == "big":
            a = b""
        out.append(dict(name=name, rec=rec, aux=a, rs=rs, tl=tl, tr=tr))
    return out


def to_bam(rec, aux):
    tid = CONTIGS.index(rec["rname"]) if rec["rname"] != "*" else -1
    mtid = tid if rec["rnext"] == "=" else -1
    return build_rec(rec["qname"], tid, rec["pos"], rec["mapq"], rec["flag"], mtid, rec["pnext"] - 1, rec["tlen"], rec["cigar"],
                     rec["seq"], rec["qual"], aux)


def expected(case):
    """(pyfilter's record, its BAM bytes): the clipped record keeps the aux bytes, the reset one has none."""
    from oracle import pyfilter
    rec = dict(case["rec"])
    new = pyfilter.clip_read(rec, case["rs"], CONTIGS[0]) if case["rs"] & 6 else rec
    is_reset = (case["rs"] & 6) and new["tags"] == {}
    return new, to_bam(new, b"" if is_reset else case["aux"])
