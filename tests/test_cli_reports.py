"""`fade annotate --stats-tsv / --clip-tsv` refusals and the stats-mode export (CPU)."""
import os
import subprocess

import pytest

import stats_report_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fade_bin():
    import __graft_entry__ as ge
    ge.build()
    return FADE


def _run(args):
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("flag", ["--stats-tsv", "--clip-tsv"])
def test_reports_refused_with_several_devices(fade_bin, tmp_path, flag):
    sam, fa = os.path.join(GOLD, "anno_c1.sam"), os.path.join(GOLD, "anno_c1.fa")
    out = str(tmp_path / "x.tsv")
    p = _run(["annotate", flag, out, "--gpus", "2", sam, fa])
    assert p.returncode == 1
    assert b"Unrecognized option" not in p.stderr
    assert (flag + " goes with one device").encode() in p.stderr and b"--gpus" in p.stderr
    assert not p.stdout and not os.path.exists(out)
    p = _run(["annotate", "%s=%s" % (flag, out), "--gpus", "2", "--out-shards", str(tmp_path / "s"), sam, fa])
    assert p.returncode == 1 and (flag + " goes with one device").encode() in p.stderr


def test_reports_flags_belong_to_annotate(fade_bin):
    p = _run(["extract", "--stats-tsv", "x.tsv", "in.sam"])
    assert p.returncode == 1 and b"Unrecognized option" in p.stderr
    p = _run(["annotate", "--clip-tsv="])
    assert p.returncode == 1 and b"Invalid value for option --clip-tsv" in p.stderr
    p = _run(["stats", "x.bam"])
    assert p.returncode == 1 and b"outside the MI355X annotate hot path" in p.stderr and b"--stats-tsv" in p.stderr


def test_library_exports_sw_stats_batch(fade_bin):
    from fade_amd import _lib
    L = _lib.load()
    assert hasattr(L, "fadehip_sw_stats_batch") and "fadehip_sw_stats_batch" in _lib.EXPORTS


def test_d_round_and_row_helpers():
    assert [(3 * n + 2) // 4 for n in (1, 2, 3, 6, 10, 150)] == [1, 2, 2, 5, 8, 113]  # D round(0.75 n), half away from 0
    assert R.parse_clips("5S10S100M") == [10, None] and R.parse_clips("3H5S90M7S2H") == [5, 7]
    assert R.aligned_length("5S10M2I3D4=1X") == 18
    assert (R.ratio(1, 3), R.ratio(0, 0), R.ratio(1, 0), R.ratio(30, 1)) == ("0.333333", "nan", "inf", "30")
    rec = dict(qname="r1", flag=16, rname="chr1", pos=100, cigar="3S5M", seq="ACGTACGT", qual="*",
               tags={"rs": ("i", "1")})
    assert R.clip_rows([rec]) == ["r1\t   \tACG\t255\t255\tfalse"]
