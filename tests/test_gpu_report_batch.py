"""fadehip_report_batch / Context.report_batch: the rows of `fade stats` and `fade stats-clip` over records annotated earlier,
written on the device, against tests/report_file_model.py (the rules in plain Python, the rows of stats_report_ref, the
inverted-repeat search of tests/sw_stats_ref.c) byte for byte: the hand-built records of tests/report_cases.py — every row
class of the alignment, the edges of a lane group and of a block of records, each failure of the rules — and the annotated
golden sets."""
import ctypes

import numpy as np
import pytest

import fade_amd
import report_cases as rc
import report_file_model as M
import tags_model as tm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want():
    """the model's reports of the 600 hand-built records: computed once, shared, left unchanged"""
    recs = rc.good_records()
    return {w: (M.stats_rows if w == "stats" else M.clip_rows)(recs, rc.NAMES) for w in ("stats", "clip")}


def _text(rows):
    return b"".join(r + b"\n" for _, _, r in rows)


def _packed(recs):
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    return np.frombuffer(b"".join(recs), dtype=np.uint8), off


@pytest.mark.parametrize("which", ["stats", "clip"])
def test_the_600_hand_built_records_in_one_call(ctx, want, which):
    recs = rc.good_records()
    cat, off = _packed(recs)
    text, row_off = ctx.report_batch_packed(cat, off, rc.NAMES, which)
    rows = want[which]
    got = [l + b"\n" for l in text.split(b"\n")[:-1]]
    for (k, side, row), line in zip(rows, got):
        assert line == row + b"\n", (rc.LABELS[k], side, line, row)
    assert text == _text(rows) and len(rows) >= (45 if which == "stats" else 300)
    # the offsets say which record and side a row is of: a slot without a row takes no bytes
    sizes = np.diff(row_off)
    assert row_off[0] == 0 and row_off[-1] == len(text) and len(row_off) == 2 * len(recs) + 1
    assert [(int(s) >> 1, int(s) & 1) for s in np.nonzero(sizes)[0]] == [(k, side) for k, side, _ in rows]
    assert [int(sizes[2 * k + side]) for k, side, _ in rows] == [len(r) + 1 for _, _, r in rows]


def test_every_named_case_on_its_own_and_both_reports_as_the_two_alone(ctx, want):
    recs = rc.good_records()
    for k, lab in enumerate(rc.LABELS):
        if lab == "filler" and k > 8:
            continue
        st = b"".join(r + b"\n" for j, _, r in want["stats"] if j == k)
        cl = b"".join(r + b"\n" for j, _, r in want["clip"] if j == k)
        assert ctx.report_batch([recs[k]], rc.NAMES, "stats") == st, lab
        assert ctx.report_batch([recs[k]], rc.NAMES, "clip") == cl, lab
    both = ctx.report_batch(recs[:120], rc.NAMES, "both")
    assert both == (ctx.report_batch(recs[:120], rc.NAMES, "stats"), ctx.report_batch(recs[:120], rc.NAMES, "clip"))
    assert both[0] == b"".join(r + b"\n" for j, _, r in want["stats"] if j < 120) and both[0] and both[1]
    assert ctx.report_batch([], rc.NAMES, "stats") == b"" and ctx.report_batch(recs[:1], rc.NAMES, "stats") == b""


@pytest.mark.parametrize("label", sorted(rc.FAILURES))
def test_each_failure_of_the_rules_fails_the_call_at_its_record_and_writes_nothing(ctx, want, label):
    which, unsupported, bad = rc.FAILURES[label]
    recs = rc.good_records()[:40]
    recs.insert(17, bad)
    with pytest.raises(M.ReportFail):
        (M.stats_rows if which == "stats" else M.clip_rows)(recs, rc.NAMES)
    cat, off = _packed(recs)
    arr = (ctypes.c_char_p * len(rc.NAMES))(*[x.encode() for x in rc.NAMES])
    out, row_off = np.full(1 << 20, 0x5a, np.uint8), np.full(2 * len(recs) + 1, 0x5a5a5a5a, np.int64)
    flag = {"stats": 1024, "clip": 2048}[which]
    rcode = ctx._L.fadehip_report_batch(ctx._h, flag, len(recs), cat.ctypes.data, off.ctypes.data, len(rc.NAMES), arr, out.ctypes.data, len(out), row_off.ctypes.data)
    msg = ctx._L.fadehip_last_error(ctx._h).decode()
    assert rcode == (-5 if unsupported else -1) and "record 17:" in msg, (rcode, msg)
    assert (out == 0x5a).all() and (row_off == 0x5a5a5a5a).all()
    # the other report does not look at what failed this one, and the context goes on
    if label != "aux_damaged":
        other = "clip" if which == "stats" else "stats"
        assert ctx.report_batch(recs, rc.NAMES, other) == M.report_text(recs, rc.NAMES, other)
    good = rc.good_records()[:40]
    assert ctx.report_batch(good, rc.NAMES, which) == _text([r for r in want[which] if r[0] < 40])


@pytest.mark.parametrize("which", ["stats", "clip"])
def test_out_cap_one_short_names_the_need_and_the_exact_cap_passes(ctx, want, which):
    recs = rc.good_records()[:200]
    text = _text([r for r in want[which] if r[0] < 200])
    cat, off = _packed(recs)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.report_batch_packed(cat, off, rc.NAMES, which, out_cap=len(text) - 1)
    assert e.value.code == -1 and ("%d bytes" % len(text)) in str(e.value), str(e.value)
    assert ctx.report_batch_packed(cat, off, rc.NAMES, which, out_cap=len(text))[0] == text
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.report_batch_packed(cat, off, rc.NAMES, "stats" if which == "clip" else "clip", out_cap=0)
    assert e.value.code == -1


@pytest.mark.parametrize("tag,n_stats,n_clip", [("anno_c1", 24, 48), ("anno_c2", 24, 50), ("anno_c5", 51, 115)])
def test_the_annotated_golden_sets(ctx, tag, n_stats, n_clip):
    names, _, bams = tm.annotated(tag)
    for which, n in (("stats", n_stats), ("clip", n_clip)):
        text = ctx.report_batch(bams, names, which)
        assert text == M.report_text(bams, names, which) and text.count(b"\n") == n
