"""`fade annotate --eject`: the option's surface, checked without a device — every refusal comes before one is opened."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")
SAM, FA = os.path.join(GOLD, "anno_c1.sam"), os.path.join(GOLD, "anno_c1.fa")


def _built():
    import __graft_entry__ as ge
    ge.build()


def _run(args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # no device may be needed for any of this
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)


def test_eject_option_refusals(tmp_path):
    _built()
    for clip in ("-c", "--clip"):
        p = _run(["annotate", "-b", "--eject", clip, SAM, FA])
        assert p.returncode == 1 and b"--eject" in p.stderr and b"--clip" in p.stderr and b"one or the other" in p.stderr and not p.stdout
    for flag in ("--stats-tsv", "--clip-tsv"):
        tsv = tmp_path / "report.tsv"
        p = _run(["annotate", "-b", "--eject", flag, str(tsv), SAM, FA])
        assert p.returncode == 1 and (flag + " describes records that --eject drops").encode() in p.stderr and not p.stdout
        assert not tsv.exists()
    p = _run(["annotate", "-b", "--eject", "--gpus", "2", SAM, FA])
    assert p.returncode == 1 and b"--eject goes with one device: not with --gpus N > 1" in p.stderr and b"name groups" in p.stderr and not p.stdout
    p = _run(["annotate", "-b", "--eject", "--gpus", "2", "--out-shards", str(tmp_path / "s"), SAM, FA])
    assert p.returncode == 1 and b"--eject goes with one device" in p.stderr and not p.stdout
    p = _run(["annotate", "-b", "--eject", "--out-shards", str(tmp_path / "s"), SAM, FA])
    assert p.returncode == 1 and b"--eject goes with one device: not with --out-shards" in p.stderr and not p.stdout
    assert not list(tmp_path.iterdir())


def test_eject_option_is_in_the_help_and_is_a_long_option_of_annotate_only():
    _built()
    p = _run(["annotate", "--help"])
    assert p.returncode == 0 and re.search(rb"^ +--eject drop the artifact reads in the same pass", p.stderr, re.M)
    for sub in ("extract", "out"):
        p = _run([sub, "--eject", SAM])
        assert p.returncode == 1 and b"Unrecognized option" in p.stderr and not p.stdout
    p = _run(["annotate", "-be", SAM, FA])  # no short form
    assert p.returncode == 1 and b"Unrecognized option -e" in p.stderr and not p.stdout


def test_eject_is_accepted_in_bundled_and_equals_forms_beside_b():
    """Parsed and accepted: each run gets as far as the check that follows the option's own (`-b` with `-u`, a --gpus value)."""
    _built()
    for args in (["-bu", "--eject"], ["--eject", "-b", "-u"], ["--eject=true", "--bam", "--ubam"], ["-b", "--eject=false", "-u", "-c"]):
        p = _run(["annotate"] + args + [SAM, FA])
        assert p.returncode == 1 and b"only one of the b or u flags" in p.stderr and b"Unrecognized" not in p.stderr and not p.stdout, args
    p = _run(["annotate", "-b", "--eject=false", "--gpus=2", "--out-shards", "", SAM, FA])  # (--eject=false is no --eject: nothing of its own is refused)
    assert p.returncode == 1 and b"--out-shards" in p.stderr and b"--eject" not in p.stderr
    p = _run(["annotate", "-b", "--eject=maybe", SAM, FA])
    assert p.returncode == 1 and b"Invalid value for option --eject: maybe" in p.stderr and not p.stdout
    p = _run(["annotate", "-b", "-w=100", "--eject", "--gpus", "2", SAM, FA])
    assert p.returncode == 1 and b"--eject goes with one device" in p.stderr


def test_eject_symbols_in_the_library_the_header_and_the_bindings():
    _built()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "fade_amd", "libfadehip.so")], stdout=subprocess.PIPE, check=True).stdout.decode()
    header = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    dbind = open(os.path.join(ROOT, "bindings", "d", "fadehip.d")).read()
    for name in ("fadehip_eject_batch", "fadehip_bam_ejected"):
        assert re.search(r" T %s$" % name, syms, re.M), name
        assert re.search(r"\bint %s\(" % name, header) and re.search(r"\bint %s\(" % name, dbind), name
    for name, val in (("FADEHIP_BAM_EJECT", 16), ("FADEHIP_BAM_EJECT_GROUPS", 32)):
        assert re.search(r"#define %s %d\b" % (name, val), header) and re.search(r"enum %s = %d;" % (name, val), dbind)
    assert re.search(r"#define FADEHIP_ABI_VERSION 3\b", header)
    from fade_amd import _lib, api
    assert (_lib.BAM_EJECT, _lib.BAM_EJECT_GROUPS) == (16, 32) == (api.BAM_EJECT, api.BAM_EJECT_GROUPS)
    assert {"fadehip_eject_batch", "fadehip_bam_ejected"} <= set(_lib.EXPORTS)
    assert callable(api.Context.eject_batch) and callable(api.BamStream.ejected)
    assert _lib.load().fadehip_abi_version() == 3
