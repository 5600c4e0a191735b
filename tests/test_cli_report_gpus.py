"""`fade stats --gpus 1` / `fade stats-clip --gpus 1`: what the command line answers before any device is opened — every
refusal comes by name, with exit status 1 and nothing on stdout — and the plain subcommands, which answer as they did.
Runs without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fade_bin():
    import __graft_entry__ as ge
    ge.build()
    return FADE


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e, **kw)


@pytest.mark.parametrize("sub,tsv", [("stats", b"--stats-tsv"), ("stats-clip", b"--clip-tsv")])
def test_without_gpus_the_subcommands_answer_as_before(fade_bin, sub, tsv):
    p = _run([sub, "x.bam"])
    assert p.returncode == 1 and p.stdout == b"" and b"outside the MI355X annotate hot path" in p.stderr and tsv in p.stderr
    assert b"--gpus 1" in p.stderr  # (the sentence the message gained)
    p = _run([sub])
    assert p.returncode == 1 and b"outside the MI355X annotate hot path" in p.stderr


@pytest.mark.parametrize("sub", ["stats", "stats-clip"])
def test_gpus_1_refuses_by_name_what_it_cannot_read_before_any_device_is_opened(fade_bin, sub, tmp_path):
    who = ("[E::fade %s] --gpus 1: " % sub).encode()
    sam = os.path.join(GOLD, "anno_c1.sam")
    for args, env, why in (([sam], None, b"not SAM text"), (["-"], None, b"not a pipe"), ([str(tmp_path / "missing.bam")], None, b"missing.bam"),
                           ([sam], {"FADE_BAM_DEVICE": "0"}, b"FADE_BAM_DEVICE=0")):
        p = _run([sub, "--gpus", "1"] + args, env, stdin=subprocess.DEVNULL)
        assert p.returncode == 1 and p.stdout == b"" and who in p.stderr and why in p.stderr, (args, p.stderr.decode())
    out = tmp_path / "never.tsv"
    p = _run([sub, "--gpus", "1", sam, str(out)])
    assert p.returncode == 1 and not out.exists()  # a refused run leaves no file behind
    p = _run([sub, "--gpus", "2", sam])
    assert p.returncode == 1 and p.stdout == b"" and b"--gpus 2" in p.stderr and b"one device" in p.stderr
    p = _run([sub, "--gpus", "1", "a.bam", "b.tsv", "c"])
    assert p.returncode == 1 and p.stdout == b"" and (b"usage: fade %s --gpus 1" % sub.encode()) in p.stderr
    p = _run([sub, "--gpus", "1"])
    assert p.returncode == 0 and p.stdout == b"" and (b"usage: fade %s --gpus 1" % sub.encode()) in p.stderr
    p = _run([sub, "--gpus", "1", "-b", "a.bam"])
    assert p.returncode == 1 and b"Unrecognized option" in p.stderr


def test_the_new_symbols_and_constants_are_exported(fade_bin):
    from fade_amd import _lib
    assert {"fadehip_report_batch", "fadehip_bam_back_report"} <= set(_lib.EXPORTS)
    assert (_lib.BAM_REPORT_STATS, _lib.BAM_REPORT_CLIP) == (1024, 2048)
    hdr = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    assert "#define FADEHIP_BAM_REPORT_STATS 1024" in hdr and "#define FADEHIP_BAM_REPORT_CLIP 2048" in hdr
