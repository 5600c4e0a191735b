"""Hand-built records for the mate map (fadehip_mateset_* / fadehip_mates_fix_batch) against tests/mates_model.py, shared by
tests/test_mates_model.py (no GPU), tests/test_gpu_mates_batch.py and tests/test_gpu_fix_mates.py (the file path and the binary).

A case is a list of records of one or more fragments whose names no other case uses, so that all cases together make one
batch.  A record is a dict: rec (BAM bytes), rs, tl, tr — what `fade out -c` would clip it by."""
import clip_cases as cc

MC50 = b"MCZ50M\0"
NM = b"NMC\x03"
XS = b"XSZhello\0"
XB = b"XBBS\x02\0\0\0\x01\0\x02\0"


def R(name, flag, tid, pos, cigar, aux=b"", rs=0, tl=0, tr=0, mtid=-1, mpos=-1, tlen=0, mapq=30):
    lq = sum(n for n, c in cc.cigar_ops(cigar) if c in "MIS=X") or 7
    seq = "".join("ACGT"[(k + len(name)) % 4] for k in range(lq))
    qual = "".join(chr(33 + (k * 5 + pos) % 40) for k in range(lq))
    return dict(rec=cc.build_rec(name, tid, pos, mapq, flag, mtid, mpos, tlen, cigar, seq, qual, aux), rs=rs, tl=tl, tr=tr)


def _cases():
    c = {}
    # ---- order and clip side
    # the worked example: R1 99 at 100 50M loses 10 bases on the left; R2 147 at 300 50M carries MC:Z:50M
    c["example_mate_behind"] = [R("ex1", 99, 0, 100, "50M", NM, rs=3, tl=10, mtid=0, mpos=300, tlen=250),
                                R("ex1", 147, 0, 300, "50M", MC50, mtid=0, mpos=100, tlen=-250)]
    c["mate_in_front"] = [R("ex2", 147, 0, 300, "50M", MC50, mtid=0, mpos=100, tlen=-250),
                          R("ex2", 99, 0, 100, "50M", MC50, rs=2, tl=10, mtid=0, mpos=300, tlen=250)]
    # both clipped; the right clip of the reverse read moves its 5' end, not its pos
    c["both_clipped_right_of_reverse"] = [R("both", 99, 0, 1000, "5S45M", MC50, rs=2, tl=5, mtid=0, mpos=1200, tlen=250),
                                          R("both", 147, 0, 1200, "50M", MC50 + NM, rs=4, tr=7, mtid=0, mpos=1000, tlen=-250)]
    # the left clip of a reverse read moves its pos, not its 5' end
    c["left_of_reverse"] = [R("lrev", 83, 1, 5000, "50M", MC50, rs=2, tl=8, mtid=1, mpos=4800, tlen=-250),
                            R("lrev", 163, 1, 4800, "50M", XS + MC50, mtid=1, mpos=5000, tlen=250)]
    c["right_of_forward"] = [R("rfwd", 99, 1, 700, "50M", MC50, rs=4, tr=9, mtid=1, mpos=900, tlen=250),
                             R("rfwd", 147, 1, 900, "20M2D30M", MC50, rs=6, tl=3, tr=4, mtid=1, mpos=700, tlen=-250)]
    # ---- mate state
    c["reset_mate"] = [R("rst", 99, 0, 100, "50M", MC50, rs=2, tl=50, mtid=0, mpos=300, tlen=250),
                       R("rst", 147, 0, 300, "50M", NM + MC50 + XS, mtid=0, mpos=100, tlen=-250)]
    c["both_reset"] = [R("rst2", 99, 0, 100, "50M", MC50, rs=2, tl=60), R("rst2", 147, 0, 300, "50M", MC50, rs=4, tr=50)]
    c["unmapped_mate"] = [R("unm", 73, 0, 2000, "10S40M", MC50 + NM, rs=2, tl=6, mtid=0, mpos=2000),
                          R("unm", 133, 0, 2000, "*", MC50, mtid=0, mpos=2000)]
    c["unmapped_mate_in_front"] = [R("unm2", 69, 1, 2000, "*", NM, mtid=1, mpos=2000),
                                   R("unm2", 137, 1, 2000, "40M10S", XS + MC50, rs=4, tr=6, mtid=1, mpos=2000)]
    c["unmapped_with_a_cigar_clipped"] = [R("unm3", 77, -1, -1, "20M", MC50, rs=2, tl=5), R("unm3", 141, -1, -1, "20M", MC50)]
    c["different_contigs"] = [R("chim", 97, 0, 100, "50M", MC50, rs=2, tl=10, mtid=1, mpos=300),
                              R("chim", 145, 1, 300, "50M", MC50, mtid=0, mpos=100)]
    c["refid_minus_one"] = [R("noref", 65, -1, 10, "20M", MC50, rs=2, tl=3), R("noref", 129, -1, 40, "20M", MC50)]
    c["cigar_without_reference_bases"] = [R("noref2", 99, 0, 100, "20S", MC50, mtid=0, mpos=130),
                                          R("noref2", 147, 0, 130, "50M", MC50, rs=2, tl=10, mtid=0, mpos=100)]
    c["mapped_without_cigar"] = [R("nocig", 99, 0, 100, "*", MC50, mtid=0, mpos=130), R("nocig", 147, 0, 130, "50M", MC50, rs=4, tr=10)]
    c["d_zero"] = [R("dzero", 65, 0, 100, "50M", MC50, rs=2, tl=10), R("dzero", 129, 0, 110, "50M", MC50)]
    # ---- which lines take part: secondary and supplementary lines of the other segment are fixed and do not insert
    c["secondary_and_supplementary"] = [R("supp", 99, 0, 100, "50M", MC50, rs=2, tl=10),
                                        R("supp", 147, 0, 300, "50M", MC50),
                                        R("supp", 147 | 0x100, 1, 9000, "50M", MC50),
                                        R("supp", 147 | 0x800, 1, 7000, "30S20M", MC50 + NM, rs=2, tl=4),
                                        R("supp", 99 | 0x800, 0, 7700, "20M30S", MC50, rs=4, tr=4)]
    # ---- keys
    c["duplicated_key"] = [R("dup", 99, 0, 100, "50M", MC50, rs=2, tl=10), R("dup", 99, 0, 120, "50M", MC50),
                           R("dup", 147, 0, 300, "50M", MC50), R("dup", 147 | 0x800, 1, 300, "50M", MC50)]
    c["unpaired_and_odd_segment_bits"] = [R("odd", 0, 0, 100, "50M", MC50, rs=2, tl=10), R("odd", 16, 0, 300, "50M", MC50),
                                          R("odd", 1 | 0xC0, 0, 100, "50M", MC50, rs=2, tl=10), R("odd", 1, 0, 300, "50M", MC50, rs=4, tr=3),
                                          R("odd", 0x40, 0, 100, "50M", MC50), R("odd", 0x80, 0, 300, "50M", MC50)]
    c["mate_absent"] = [R("lonely", 99, 0, 100, "50M", MC50, rs=2, tl=10, mtid=0, mpos=300, tlen=250)]
    # ---- MC fields
    c["mc_first_middle_last"] = [R("mc1", 99, 0, 100, "50M", rs=2, tl=10), R("mc1", 147, 0, 300, "50M", MC50 + NM + XB + XS),
                                 R("mc2", 99, 0, 100, "50M", rs=2, tl=11), R("mc2", 147, 0, 300, "50M", NM + XB + MC50 + XS),
                                 R("mc3", 99, 0, 100, "50M", rs=2, tl=12), R("mc3", 147, 0, 300, "50M", NM + XS + XB + MC50)]
    c["mc_grows_and_shrinks"] = [R("mcg", 99, 0, 100, "9S" + "7M1I6M2D" * 40 + "11S", MC50, rs=6, tl=203, tr=190),
                                 R("mcg", 147, 0, 300, "50M", b"MCZ*\0" + NM),
                                 R("mcs", 99, 0, 100, "50M", b"MCZ" + b"7M1I6M2D" * 30 + b"\0"),
                                 R("mcs", 147, 0, 300, "50M", b"MCZ5S10M2I33M5S\0" + NM + b"MCZ\0")]
    c["mc_of_another_type"] = [R("mci", 99, 0, 100, "50M", rs=2, tl=10), R("mci", 147, 0, 300, "50M", NM + b"MCi\x05\0\0\0" + XS),
                               R("mch", 99, 0, 100, "50M", rs=2, tl=10), R("mch", 147, 0, 300, "50M", b"MCH1AE3\0" + MC50)]
    c["two_mc_fields"] = [R("mc2z", 99, 0, 100, "50M", rs=2, tl=10), R("mc2z", 147, 0, 300, "50M", NM + MC50 + XS + b"MCZ49M1S\0")]
    c["mc_absent"] = [R("nomc", 99, 0, 100, "50M", rs=2, tl=10), R("nomc", 147, 0, 300, "50M", NM + XS), R("nomc2", 99, 0, 100, "50M", rs=2, tl=10),
                      R("nomc2", 147, 0, 300, "50M")]
    c["aux_not_whole_in_front_of_mc"] = [R("brk", 99, 0, 100, "50M", rs=2, tl=10), R("brk", 147, 0, 300, "50M", NM + b"XQ?" + MC50),
                                         R("brk2", 99, 0, 100, "50M", rs=2, tl=10), R("brk2", 147, 0, 300, "50M", MC50 + b"XZZnever ends")]
    # ---- names
    long_name = "".join(chr(65 + k % 26) for k in range(254))
    c["names"] = [R("a", 99, 0, 100, "50M", MC50, rs=2, tl=10), R("a", 147, 0, 300, "50M", MC50),
                  R(long_name, 99, 0, 100, "50M", MC50, rs=2, tl=11), R(long_name, 147, 0, 300, "50M", MC50),
                  R(long_name[:-1] + "!", 99, 0, 100, "50M", MC50, rs=2, tl=12), R(long_name[:-1] + "!", 147, 0, 300, "50M", MC50),
                  R("frag", 99, 0, 100, "50M", MC50, rs=2, tl=13), R("fragm", 147, 0, 300, "50M", MC50),
                  R("fragm", 99, 0, 100, "50M", MC50, rs=2, tl=14), R("frag", 147, 0, 300, "50M", MC50),
                  R("abc", 99, 0, 100, "50M", MC50, rs=2, tl=15), R("abc", 147, 0, 300, "50M", MC50),     # the segment byte at every
                  R("abcd", 99, 0, 100, "50M", MC50, rs=2, tl=16), R("abcd", 147, 0, 300, "50M", MC50),   # place of a dword
                  R("abcde", 99, 0, 100, "50M", MC50, rs=2, tl=17), R("abcde", 147, 0, 300, "50M", MC50),
                  R("abcdef", 99, 0, 100, "50M", MC50, rs=2, tl=18), R("abcdef", 147, 0, 300, "50M", MC50)]
    return c


CASES = _cases()


def flat(cases=None):
    """Every case's records, in order, as (records, rs, tl, tr)."""
    rows = [r for name in (cases or CASES) for r in CASES[name]]
    return [r["rec"] for r in rows], [r["rs"] for r in rows], [r["tl"] for r in rows], [r["tr"] for r in rows]


def filler(k):
    """An unpaired record that neither inserts nor is fixed."""
    return R("filler%d" % k, 16 * (k % 2), 0, 100 + k, "30M", NM)


def tagged(row):
    """The record with the rs and am fields `fade out -c` reads the row's rs and trims back from (none for rs 0)."""
    if not row["rs"]:
        return row["rec"]
    am = ("ctgA,7,%dM" % row["tl"] if row["rs"] & 2 else "") + ";" + ("ctgA,7,%dM" % row["tr"] if row["rs"] & 4 else "")
    rec = row["rec"] + b"rsC" + bytes([row["rs"]]) + b"amZ" + am.encode() + b"\0"
    return len(rec[4:]).to_bytes(4, "little") + rec[4:]


def flat_tagged(cases=None):
    """flat() with every record carrying its rs and am, as a file holds them."""
    rows = [r for name in (cases or CASES) for r in CASES[name]]
    return [tagged(r) for r in rows], [r["rs"] for r in rows], [r["tl"] for r in rows], [r["tr"] for r in rows]
