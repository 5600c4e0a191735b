"""Generated records for the hard clip (filter.d:15-91 clipRead): the ground under tests/clip_cases._SPECS' 50 hand-built
ones, for every path that clips — tests/test_gpu_clip_sweep.py (the device function and the file path), the sweep test of
tests/test_cli_clip.py (the host's clip_read), tests/test_clip_sweep.py (what the sweep holds, no GPU).

A case is the dict clip_cases.cases() gives (name, rec, aux, rs, tl, tr): clip_cases.to_bam / expected work on it as they
are, oracle/pyfilter.clip_read stays the arbiter of fields and clip_cases.build_rec / reg2bin of bytes and bin.  Fixed
seeds, no GPU.  Three families:

a  writer()      "{lq}M" at every l_seq / left trim / right trim that sets another (parity of the first surviving base) x
                 (packed bytes mod 4) x (odd or even rest), with a dword loop of one, two and more trips per lane and a byte
                 tail, at every byte alignment of the CIGAR (l_read_name 2..5), all 16 base codes, aux none / small / 3 KB.
b  bins()        spans that end at, one short of and one past 2^s * m for every level shift s of reg2bin, clipped so that the
                 record falls to a finer level, stays, has its new pos cross the line or ends on it; N ops up to 2^27;
                 positions at and above 2^29 (the bin is 16 bits wide there: build_rec keeps the low 16, as the BAM field
                 does); unmapped records (refID -1, pos -1) that carry a CIGAR.
c  random_ops()  1 to 8 ops over M I D N S H P = X in any order, lengths 1..12, both sides, resets a minority, one record
                 in ten with fewer bases than the CIGAR claims.

No op of length zero anywhere: pyfilter.clip_read takes a base at a time and does not terminate on a zero-length op that
consumes no reference, and no BAM writer produces one.  pyfilter walks base by base through what a trim takes, so the trims
of family b that cross a whole N keep that N at 4,096; the N ops of up to 2^27 are only nibbled at."""
import functools
import random

import clip_cases as cc

LN = 2147483647  # @SQ LN of a header that covers every position here
SMALL_AUX = b"NMC\x03XSZhello\0"
A_LQ = list(range(1, 73)) + list(range(120, 141)) + list(range(250, 263)) + list(range(513, 521))
B_SHIFTS = (14, 17, 20, 23, 26, 29)
N_RANDOM = 20000


def _am(rs, tl, tr, contig):
    return ("%s,7,%dM" % (contig, tl) if rs & 2 else "") + ";" + ("%s,7,%dM" % (contig, tr) if rs & 4 else "")


def _case(name, qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual, aux, rs, tl, tr):
    if qual == "*":  # (a lone '*' is SAM's "no qualities")
        qual = "+"
    rec = dict(qname=qname, flag=flag, rname=rname, pos=pos, mapq=mapq, cigar=cigar, rnext=rnext, pnext=pnext, tlen=tlen, seq=seq, qual=qual,
               tags={"rs": ("i", str(rs)), "am": ("Z", _am(rs, tl, tr, cc.CONTIGS[0]))}, tag_order=["rs", "am"])
    return dict(name=name, rec=rec, aux=aux, rs=rs, tl=tl, tr=tr)


def _seq(lq, k):
    return "".join(cc.NT16[(j + k) % 16] for j in range(lq))


def _qual(lq, k):
    return "".join(chr(33 + (j * 7 + k) % 94) for j in range(lq))


# ------------------------------------------------------------------------------------------------ a: the writer
@functools.lru_cache(maxsize=None)
def _writer():
    import numpy as np
    rng = np.random.default_rng(20261020)
    out, k = [], 0
    for lq in A_LQ:
        for hl in range(min(lq - 1, 18) + 1):
            for hr in range(4):
                if hl + hr >= lq:
                    continue
                ok = [6] + ([2] if hr == 0 else []) + ([4] if hl == 0 and hr > 0 else [])
                rs = ok[k % len(ok)]
                aux = cc._big_aux(rng, 3000) if k % 50 == 49 else (b"", SMALL_AUX)[(k // 4) % 2]
                out.append(_case("a_lq%d_hl%d_hr%d_rs%d" % (lq, hl, hr, rs), "wxyz"[:1 + k % 4], (0, 16, 99, 147)[k % 4], cc.CONTIGS[k % 2], 1000 + 3 * k,
                                 k % 61, "%dM" % lq, "=", 3000 + k, (-1) ** k * (100 + k % 400), _seq(lq, k), _qual(lq, k), aux, rs, hl, hr))
                k += 1
    return tuple(out)


# ------------------------------------------------------------------------------------------------ b: the bin
@functools.lru_cache(maxsize=None)
def _bins():
    out = []

    def add(label, pos, cigar, rs, tl, tr, unmapped=False):
        k = len(out)
        lq = sum(n for n, c in cc.cigar_ops(cigar) if c in cc._QC)
        out.append(_case("b%03d_%s_at%d_%s_rs%d_%d_%d" % (k, label, pos, cigar, rs, tl, tr), "b%04d" % k, 4 if unmapped else (0, 16)[k % 2], "*" if unmapped else cc.CONTIGS[k % 2],
                         pos, 0 if unmapped else 20 + k % 40, cigar, "*" if unmapped else "=", 0 if unmapped else 1 + (pos + 200) % (1 << 30), 0 if unmapped else 150,
                         _seq(lq, k), _qual(lq, k), (b"", SMALL_AUX)[k % 2], rs, tl, tr))

    for s in B_SHIFTS:
        for m in (1, 3 if s == 29 else 5):
            line = m << s
            small, big = 4096, min(1 << (s - 1), 1 << 27)
            for e in (-1, 0, 1):  # the incoming span ends at line + e
                lab = "s%d_m%d_e%+d" % (s, m, e)
                cigar = "30M%dN40M" % small
                pos = line + e - (70 + small)
                add(lab + "_right1", pos, cigar, 4, 0, 1)                    # one base less: e = +1 ends on the line, off the coarser level
                add(lab + "_right2", pos, cigar, 4, 0, 2)
                add(lab + "_eatN_right", pos, cigar, 4, 0, 40 + small + 5)   # 25M is left: a finer level
                add(lab + "_eatN_left", pos, cigar, 2, 30 + small + 3, 0)    # 37M in front of the line
                add(lab + "_eatN_both", pos, cigar, 6, 30 + small, 40 - 1)   # one base
                add(lab + "_stays", pos, cigar, 6, 5, 5)
                add(lab + "_untouched", pos, cigar, 0, 5, 5)
                cigar = "30M%dN40M" % big                                    # a coarse record that is only nibbled at
                pos = line + e - (70 + big)
                add(lab + "_big_stays", pos, cigar, 6, 7, 9)
                add(lab + "_big_intoN_left", pos, cigar, 2, 30 + 3, 0)
                add(lab + "_big_intoN_right", pos, cigar, 4, 0, 40 + 2)
                add(lab + "_big_intoN_both", pos, cigar, 6, 30 + 1, 40 + 1)
            lab = "s%d_m%d" % (s, m)
            for tl in (11, 12, 13):  # the new pos one short of, on and one past the line
                add(lab + "_pos_crosses", line - 12, "40M", 2, tl, 0)
                add(lab + "_pos_crosses_both", line - 12, "20M2D18M", 6, tl, 3)
            add(lab + "_pos_crosses_N", line - 5 - small // 2, "5M%dN40M" % small, 2, 5 + small, 0)
            for tr in (9, 10, 11):   # the new end one past, on and one short of the line
                add(lab + "_end_on_line", line - 50, "60M", 4, 0, tr)
                add(lab + "_end_on_line_both", line - 50, "30M1I30M", 6, 17, tr)
    for pos in ((1 << 29) - 1, 1 << 29, (1 << 29) + 1, (1 << 29) + 5000, (1 << 30) - 20, (1 << 30) + 77, 3 << 29):
        add("high", pos, "50M", 2, 10, 0)
        add("high", pos, "10S40M3I7M", 6, 21, 8)
        add("high_reset", pos, "50M", 4, 0, 50)
    for k in (0, 1, 5, 19):
        add("unmapped_left", -1, "20M", 2, k, 0, unmapped=True)      # the new pos is -1 + k
    add("unmapped_left_reset", -1, "20M", 2, 20, 0, unmapped=True)
    add("unmapped_right", -1, "20M", 4, 0, 3, unmapped=True)         # pos stays -1: the span begins at 0
    add("unmapped_right", -1, "3S20M5S", 4, 0, 0, unmapped=True)
    add("unmapped_both", -1, "4S20M", 6, 1, 2, unmapped=True)
    add("unmapped_untouched", -1, "20M", 1, 3, 3, unmapped=True)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ c: random CIGARs
_OPS = "MMMIDNSHP=X"  # (M three times as often as another op: a tenth of all-uniform CIGARs would align nothing)


@functools.lru_cache(maxsize=None)
def _random_ops(n=N_RANDOM):
    rng = random.Random(20261021)
    out = []
    for k in range(n):
        ops = []
        for _ in range(rng.randint(1, 8)):
            c = rng.choice(_OPS)
            ops.append((rng.randint(1, 12), c))
        cigar = "".join("%d%s" % o for o in ops)
        aligned = sum(x for x, c in ops if c in cc._RC)
        claimed = sum(x for x, c in ops if c in cc._QC)
        r = rng.random()
        rs = rng.choice((2, 4, 6, 6)) if r < 0.97 else rng.choice((0, 1))

        def trim(al):  # below the aligned length three times in four
            return rng.randrange(al) if al > 0 and rng.random() < 0.75 else al + rng.randint(0, 2)

        tl = trim(aligned)
        # the right trim of a both-sides call is drawn against what the left step leaves, the length it is compared with
        tr = trim(aligned - tl if rs & 2 and rs & 4 and tl < aligned else aligned)
        lq = claimed
        if rng.random() < 0.1 and claimed > 0:  # fewer bases than the CIGAR claims
            lq = max(0, claimed - rng.randint(1, 3))
            # ... and here a side's trim stops at the last reference base more often, so that the H ops reach the shortage
            if rs & 6 and aligned > 1 and rng.random() < 0.6:
                if rs == 6:
                    tl = rng.randrange(aligned - 1)
                    tr = aligned - tl - 1
                elif rs == 2:
                    tl = aligned - 1
                else:
                    tr = aligned - 1
        name = "c%05d_%s_rs%d_%d_%d%s" % (k, cigar, rs, tl, tr, "_short%d" % (claimed - lq) if lq < claimed else "")
        paired = rng.random() < 0.8
        out.append(_case(name, "c%05d" % k, rng.randrange(1 << 12), cc.CONTIGS[k % 2], rng.randrange(1 << 28), rng.randrange(256), cigar,
                         "=" if paired else "*", rng.randrange(1, 1 << 28) if paired else 0, rng.randint(-(1 << 20), 1 << 20),
                         _seq(lq, rng.randrange(16)), _qual(lq, rng.randrange(94)), (b"", SMALL_AUX, b"XYi\xff\xff\xff\x7f")[k % 3], rs, tl, tr))
    return tuple(out)


FAMILIES = {"writer": _writer, "bins": _bins, "random": _random_ops}


def cases(family, sam_only=False):
    """The family's cases, in a fixed order.  sam_only: without the aux areas of several KB."""
    out = FAMILIES[family]()
    return [dict(c, aux=b"") if sam_only and len(c["aux"]) > 1000 else c for c in out]


@functools.lru_cache(maxsize=None)
def expected(family):
    """clip_cases.expected over the family: a tuple of (pyfilter's record, its BAM bytes), computed once per process."""
    return tuple(cc.expected(c) for c in FAMILIES[family]())


def is_reset(case, new):
    return bool(case["rs"] & 6) and new["tags"] == {}


def level(pos, cigar):
    """Which of reg2bin's six outcomes the record's span takes: the shift of its level, 0 for the fall-through."""
    beg = max(pos, 0)
    ref = sum(n for n, c in cc.cigar_ops(cigar) if c in cc._RC)
    end = beg + (ref if ref > 0 else 1) - 1
    for sh in (14, 17, 20, 23, 26):
        if beg >> sh == end >> sh:
            return sh
    return 0
