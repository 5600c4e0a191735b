"""`fade stats --gpus 1 --repeats PATH`: what the command line answers before any device is opened — every refusal comes by
name, with exit status 1 and nothing on stdout — and the surface the option adds, in the header, the Python binding and the D
binding alike.  Runs without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")
SAM = os.path.join(GOLD, "anno_c1.sam")
NEW = ["fadehip_intervals_create", "fadehip_intervals_add", "fadehip_intervals_seal", "fadehip_intervals_count", "fadehip_intervals_overlap_batch",
       "fadehip_intervals_load_bed", "fadehip_intervals_destroy", "fadehip_report_batch_repeats", "fadehip_bam_use_intervals"]


@pytest.fixture(scope="module")
def fade_bin():
    import __graft_entry__ as ge
    ge.build()
    return FADE


@pytest.fixture()
def bed(tmp_path):
    f = tmp_path / "rmsk.bed"
    f.write_bytes(b"chr1\t10\t20\n")
    return str(f)


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e, **kw)


def _refused(p, who, why):
    assert p.returncode == 1 and p.stdout == b"" and (b"[E::" + who + b"] --repeats: ") in p.stderr and why in p.stderr, p.stderr.decode()


def test_without_gpus_1_there_is_no_host_loop_behind_it(fade_bin, bed):
    _refused(_run(["stats", "--repeats", bed, SAM]), b"fade stats", b"it goes with --gpus 1")
    _refused(_run(["stats", "--repeats=" + bed, SAM, "out.tsv"]), b"fade stats", b"no host loop")
    p = _run(["stats", "--gpus", "2", "--repeats", bed, SAM])
    assert p.returncode == 1 and p.stdout == b"" and b"--gpus 2" in p.stderr and b"one device" in p.stderr


def test_stats_clip_rows_carry_no_coordinates(fade_bin, bed):
    _refused(_run(["stats-clip", "--gpus", "1", "--repeats", bed, SAM]), b"fade stats-clip", b"carry no coordinates")
    _refused(_run(["stats-clip", "--repeats", bed, SAM]), b"fade stats-clip", b"carry no coordinates")


def test_annotate_stats_tsv_is_out_of_scope_and_annotate_alone_does_not_take_it(fade_bin, bed, tmp_path):
    fa = os.path.join(GOLD, "anno_c1.fa")
    out = tmp_path / "never.tsv"
    _refused(_run(["annotate", "--stats-tsv", str(out), "--repeats", bed, SAM, fa]), b"fade-annotate", b"out of scope")
    assert not out.exists()
    _refused(_run(["annotate", "--repeats", bed, SAM, fa]), b"fade-annotate", b"goes with fade stats --gpus 1")


@pytest.mark.parametrize("sub", ["out", "extract"])
def test_the_other_subcommands_do_not_know_it(fade_bin, bed, sub):
    for extra in ([], ["--gpus", "1", "-b"]):
        p = _run([sub] + extra + ["--repeats", bed, SAM])
        assert p.returncode == 1 and p.stdout == b"" and b"Unrecognized option --repeats" in p.stderr and b"goes with fade stats --gpus 1" in p.stderr, p.stderr.decode()


def test_the_bed_path_is_checked_before_any_device_is_opened(fade_bin, bed, tmp_path):
    for name in ("rmsk.bed.gz", "rmsk.bed.bgz"):
        z = tmp_path / name
        z.write_bytes(b"\x1f\x8b")
        p = _run(["stats", "--gpus", "1", "--repeats", str(z), SAM])
        _refused(p, b"fade stats", b"plain text")
        assert name.encode() in p.stderr
    _refused(_run(["stats", "--gpus", "1", "--repeats", str(tmp_path / "missing.bed"), SAM]), b"fade stats", b"not a missing path")
    _refused(_run(["stats", "--gpus", "1", "--repeats", str(tmp_path), SAM]), b"fade stats", b"not a directory")
    p = _run(["stats", "--gpus", "1", "--repeats"])
    assert p.returncode == 1 and p.stdout == b""  # (std.getopt's words: a value is missing; then the plain subcommand's answer)
    p = _run(["stats", "--gpus", "1", "--repeats="])
    assert p.returncode == 1 and p.stdout == b""
    # with a good BED the run goes on to what --gpus 1 refuses by itself: the input, which is SAM text here
    out = tmp_path / "never.tsv"
    p = _run(["stats", "--gpus", "1", "--repeats", bed, SAM, str(out)])
    assert p.returncode == 1 and p.stdout == b"" and b"[E::fade stats] --gpus 1: " in p.stderr and b"not SAM text" in p.stderr and not out.exists()
    p = _run(["stats", "--gpus", "1", "--repeats", bed, SAM], {"FADE_BAM_DEVICE": "0"})
    assert p.returncode == 1 and p.stdout == b"" and b"FADE_BAM_DEVICE=0" in p.stderr


def test_the_help_text_lists_the_option_for_stats_alone(fade_bin):
    p = _run(["stats", "--gpus", "1", "--help"])
    assert p.returncode == 0 and b"--repeats PATH" in p.stderr and b"read_rpm" in p.stderr
    p = _run(["stats-clip", "--gpus", "1", "--help"])
    assert p.returncode == 0 and b"--repeats" not in p.stderr


def test_without_the_option_the_subcommands_answer_as_before(fade_bin):
    p = _run(["stats", "x.bam"])
    assert p.returncode == 1 and p.stdout == b"" and b"outside the MI355X annotate hot path" in p.stderr and b"--repeats" not in p.stderr


def test_the_symbols_and_the_flag_agree_everywhere_and_the_abi_is_the_same(fade_bin):
    from fade_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    d = open(os.path.join(ROOT, "bindings", "d", "fadehip.d")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert re.search(r"\b%s\(" % name, header), name
        assert re.search(r"\b%s\(" % name, d), name
    assert _lib.BAM_REPORT_REPEATS == 65536 and "#define FADEHIP_BAM_REPORT_REPEATS 65536" in header
    assert re.search(r"FADEHIP_BAM_REPORT_REPEATS\s*=\s*65536", d)
    assert "struct fadehip_intervals;" in d
    assert _lib.ABI_VERSION == 3 and L.fadehip_abi_version() == 3 and "#define FADEHIP_ABI_VERSION 3" in header
    import fade_amd
    for attr in ("intervalset", "load_bed"):
        assert hasattr(fade_amd.Context, attr)
    assert hasattr(fade_amd.api, "IntervalSet")
