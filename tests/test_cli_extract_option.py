"""`fade annotate --extract PATH`: the option's surface, checked without a device — every refusal comes before one is opened."""
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


def test_extract_option_refusals(tmp_path):
    _built()
    x = str(tmp_path / "x.bam")
    p = _run(["annotate", "-b", SAM, FA, "--extract"])
    assert p.returncode == 1 and b"--extract" in p.stderr and not p.stdout
    p = _run(["annotate", "-b", "--extract", x, "--gpus", "2", SAM, FA])
    assert p.returncode == 1 and b"--extract" in p.stderr and b"--gpus" in p.stderr and not p.stdout
    p = _run(["annotate", "-b", "--extract", x, "--gpus", "2", "--out-shards", str(tmp_path / "s"), SAM, FA])
    assert p.returncode == 1 and b"--extract" in p.stderr and not p.stdout
    p = _run(["annotate", "-b", "--extract", x, "--out-shards", str(tmp_path / "s"), SAM, FA])
    assert p.returncode == 1 and b"--extract" in p.stderr and b"--out-shards" in p.stderr and not p.stdout
    for path in (SAM, os.path.join(GOLD, ".", "anno_c1.sam"), "-"):
        p = _run(["annotate", "-b", "--extract", path, SAM, FA])
        assert p.returncode == 1 and b"--extract" in p.stderr and not p.stdout, path
    assert not os.path.exists(x)
    assert open(SAM, "rb").read(3) == b"@HD" or open(SAM, "rb").read(1) == b"@"  # the input is still there


def test_extract_option_is_in_the_help_and_the_other_subcommands_do_not_take_it():
    _built()
    p = _run(["annotate", "--help"])
    assert p.returncode == 0 and b"--extract PATH" in p.stderr
    for sub in ("extract", "out"):
        p = _run([sub, "--extract", "x", SAM])
        assert p.returncode == 1


def test_extract_symbols_in_the_library_the_header_and_the_bindings():
    _built()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "fade_amd", "libfadehip.so")], stdout=subprocess.PIPE, check=True).stdout.decode()
    header = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    dbind = open(os.path.join(ROOT, "bindings", "d", "fadehip.d")).read()
    for name in ("fadehip_extract_batch", "fadehip_bam_back_extract"):
        assert re.search(r" T %s$" % name, syms, re.M), name
        assert re.search(r"\bint %s\(" % name, header) and re.search(r"\bint %s\(" % name, dbind), name
    assert re.search(r"#define FADEHIP_BAM_EXTRACT 8\b", header) and re.search(r"enum FADEHIP_BAM_EXTRACT = 8;", dbind)
    assert re.search(r"#define FADEHIP_ABI_VERSION 3\b", header)
    from fade_amd import _lib
    assert _lib.BAM_EXTRACT == 8 and {"fadehip_extract_batch", "fadehip_bam_back_extract"} <= set(_lib.EXPORTS)
    assert _lib.load().fadehip_abi_version() == 3
