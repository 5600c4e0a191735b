"""tests/report_file_model.py (the rules of `fade stats` / `fade stats-clip` over tags read back, in plain Python over BAM
record bytes) against stats_report_ref over the annotated golden sets, the skip and fail rules on hand-built records, and
fmt_g6.hpp — the text of the reports' float columns as the device compiles it — against libc's %g under ASan + UBSan.
Runs without a GPU."""
import os
import subprocess

import pytest

import report_cases as rc
import report_file_model as M
import stats_report_ref as R
import tags_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fade_amd", "csrc")


def test_fmt_g6_agrees_with_libc_on_every_ratio_and_two_million_random_floats():
    """Every num / den with den 1 .. 256, num 0 .. 255 den, the named edges and the seeded random bit patterns: the
    reference is snprintf("%g") of the same float, never the function's earlier output."""
    subprocess.check_call(["make", "-C", CSRC, "-s", "build/fmt_g6_selftest"])
    p = subprocess.run([os.path.join(CSRC, "build", "fmt_g6_selftest")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    words = p.stdout.decode().split()
    assert words[0] == "fmt_g6_selftest:" and int(words[1]) >= 255 * 256 * 257 // 2 + 2000000 and words[3:] == ["0", "differences"]


@pytest.mark.parametrize("tag,n_stats,n_clip", [("anno_c1", 24, 48), ("anno_c2", 24, 50), ("anno_c5", 51, 115)])
def test_model_over_bam_bytes_gives_the_rows_of_stats_report_ref(tag, n_stats, n_clip):
    names, recs, bams = tm.annotated(tag)
    want = ["\t".join(r).encode() for r in R.stats_rows(recs)]
    got = M.stats_rows(bams, names)
    assert [r for _, _, r in got] == want and len(want) == n_stats
    assert all(len(r.split(b"\t")) == 21 for r in want)
    want = [r.encode("latin-1") for r in R.clip_rows(recs)]
    got = M.clip_rows(bams, names)
    assert [r for _, _, r in got] == want and len(want) == n_clip
    assert M.report_text(bams, names, "clip") == b"".join(r + b"\n" for r in want)
    # slots come in input order, left before right
    assert [(k, s) for k, s, _ in got] == sorted((k, s) for k, s, _ in got)


def test_the_hand_built_cases_are_what_they_say():
    recs = rc.good_records()
    rows = M.stats_rows(recs, rc.NAMES)
    by = {}
    for k, side, row in rows:
        by.setdefault(rc.LABELS[k], []).append((side, row.split(b"\t")))
    assert [s for s, _ in by["both_sides"]] == [0, 1] and [s for s, _ in by["left_only"]] == [0] and [s for s, _ in by["right_only"]] == [1]
    for skipped in ("rs_absent", "rs_Z", "am_absent", "am_i"):
        assert skipped not in by
    for t in "cCsSiI":
        assert "rs_" + t in by
    # the stem loops of every row class and the strip edge, 0.75 n rounded half away from zero
    assert [len(by["stem_%d" % n][0][1][10]) for n in rc.STEMS] == list(rc.STEMS)
    assert [(3 * n + 2) // 4 for n in (1, 2, 3)] == [1, 2, 2]
    # as with three pieces: the right side takes piece 1; ab longer than the piece: the right side takes the tail
    assert by["as_three_pieces"][0][1][10] == b"GGGGCCCC" and by["ab_longer"][0][1][16] == b"KLMNOPQR"
    # the first S anywhere (left), the last S anywhere (right), a negative art_start
    assert by["cigar_5S10S100M"][0][1][4:6] == [b"95", b"100"] and by["cigar_3H5S90M7S2H"][0][1][4:6] == [b"190", b"197"]
    assert by["cigar_inner_S"][0][1][4:6] == [b"96", b"100"] and by["cigar_inner_S"][1][1][4:6] == [b"150", b"156"]
    assert by["pos_0_left_clip"][0][1][2:6] == [b"0", b"8S50M", b"-8", b"0"]
    assert by["name_1"][0][1][1] == b"c" and len(by["name_40"][0][1][1]) == 40
    assert by["qual_ff"][0][1][14] == b"255" and by["long_read"][0][1][14] == b"5e-05"
    assert sorted(k for k, lab in enumerate(rc.LABELS) if lab.startswith("edge_")) == [255, 256, 257, 511, 512] and len(recs) == 600
    clip = M.clip_rows(recs, rc.NAMES)
    q = {rc.LABELS[k]: row.split(b"\t") for k, side, row in clip if side == 0}
    assert q["qual_ff"][1] == b" " * 8 and q["qual_ff"][3] == b"255" and q["cigar_5S10S100M"][1:3] == [b"I" * 10, b"ACGTACGTAC"]
    assert q["pos_0_left_clip"][5] == b"true" and q["right_only"][5] == b"false"


@pytest.mark.parametrize("label", sorted(rc.FAILURES))
def test_each_failure_of_the_rules_fails_the_model_at_its_record(label):
    which, unsupported, rec = rc.FAILURES[label]
    recs = rc.good_records()[:40]
    recs.insert(17, rec)
    with pytest.raises(M.ReportFail) as e:
        (M.stats_rows if which == "stats" else M.clip_rows)(recs, rc.NAMES)
    assert e.value.record == 17 and e.value.unsupported == unsupported, label
    other = M.clip_rows if which == "stats" and label != "aux_damaged" else None
    if other:  # a failure of one report's rules is none of the other's
        other(recs, rc.NAMES)
