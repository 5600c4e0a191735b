"""`fade out --gpus 1 --sort`, `fade annotate --sort` and the sorted main output's library surface, the part that needs no device:
the option has no host loop behind it, so where it cannot run it is refused by name, with its reason, before a device is opened
and with nothing on stdout; both help texts list it and the other subcommands do not take it; the stream flag and the new
exports agree in the header, the D binding and the loader, the ABI stays what it was, and NULL arguments are refused before
any device call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cli_extract import _annotated_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
FA = os.path.join(ROOT, "tests", "golden", "anno_c2.fa")
NEW = ["fadehip_recstore_set_budget", "fadehip_recstore_measure", "fadehip_recstore_over", "fadehip_recstore_histogram", "fadehip_recstore_set_window", "fadehip_recstore_reset",
       "fadehip_recstore_budget", "fadehip_recstore_resets"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from fade_amd import _lib
    return _lib, _lib.load()


@pytest.fixture(scope="module")
def anno(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_sort")
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(_annotated_sam("anno_c2"))
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), str(sam)], stdout=fo)
    return sam, bam, d


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e, **kw)


OUT = {
    "sam_output": (lambda sam, bam: (["out", "--gpus", "1", "--sort", str(bam)], {}), b"the output is SAM text"),
    "sam_input": (lambda sam, bam: (["out", "--gpus", "1", "--sort", "-b", str(sam)], {}), b"not SAM text"),
    "no_device": (lambda sam, bam: (["out", "--gpus", "1", "--sort", "-b", str(bam)], {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "two_devices": (lambda sam, bam: (["out", "--gpus", "2", "--sort", "-u", str(bam)], {}), b"--gpus N other than 1"),
    "no_devices": (lambda sam, bam: (["out", "--gpus", "0", "--sort", "-u", str(bam)], {}), b"--gpus N other than 1"),
    "without_gpus": (lambda sam, bam: (["out", "--sort", "-b", str(bam)], {}), b"it goes with --gpus 1"),
    "keep_sorted": (lambda sam, bam: (["out", "--gpus", "1", "-c", "--keep-sorted", "--sort", "-b", str(bam)], {}), b"not with --keep-sorted"),
    "clip_and_fix_mates_sam_output": (lambda sam, bam: (["out", "--gpus", "1", "-c", "--fix-mates", "--sort", str(bam)], {}), b"the output is SAM text"),
    "fragments_without_gpus": (lambda sam, bam: (["out", "--fragments", "--sort", "-b", str(bam)], {}), b"it goes with --gpus 1"),
}


def _anno(extra, inp, env=None):
    return ["annotate"] + extra + [str(inp), FA], env or {}


ANNOTATE = {
    "sam_output": (lambda sam, bam, x: _anno(["--sort"], bam), b"the output is SAM text"),
    "sam_input": (lambda sam, bam, x: _anno(["--sort", "-b"], sam), b"not SAM text"),
    "no_device": (lambda sam, bam, x: _anno(["--sort", "-u"], bam, {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "two_devices": (lambda sam, bam, x: _anno(["--sort", "-b", "--gpus", "2"], bam), b"--gpus N other than 1"),
    "out_shards": (lambda sam, bam, x: _anno(["--sort", "-b", "--gpus", "2", "--out-shards", x], bam), b"not with --out-shards"),
    "keep_sorted": (lambda sam, bam, x: _anno(["--sort", "-c", "--keep-sorted", "-b"], bam), b"not with --keep-sorted"),
    "extract": (lambda sam, bam, x: _anno(["--sort", "-b", "--extract", x], bam), b"not with --extract "),
    "extract_sorted": (lambda sam, bam, x: _anno(["--sort", "-b", "--extract", x, "--extract-sorted"], bam), b"not with --extract-sorted"),
    "stats_tsv": (lambda sam, bam, x: _anno(["--sort", "-b", "--stats-tsv", x], bam), b"--stats-tsv"),
    "clip_tsv": (lambda sam, bam, x: _anno(["--sort", "-b", "--clip-tsv", x], bam), b"--clip-tsv"),
}


@pytest.mark.parametrize("case", list(ANNOTATE))
def test_sort_of_annotate_is_refused_by_name_where_it_cannot_run(anno, case):
    make, reason = ANNOTATE[case]
    sam, bam, d = anno
    x = str(d / (case + ".side"))
    args, env = make(sam, bam, x)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert reason in p.stderr and b"[E::fade-annotate] --sort: " in p.stderr, p.stderr.decode()
    assert b"[W::" not in p.stderr and not os.path.exists(x) and not os.path.exists(x + ".bai")


def test_piped_input_is_refused_for_annotate(anno):
    sam, bam, d = anno
    with open(bam, "rb") as fi:
        p = _run(["annotate", "--sort", "-b", "-", FA], stdin=fi)
    assert p.returncode == 1 and p.stdout == b"" and b"[E::fade-annotate] --sort: " in p.stderr and b"not a pipe" in p.stderr, p.stderr.decode()


@pytest.mark.parametrize("case", list(OUT))
def test_sort_is_refused_by_name_where_it_cannot_run(anno, case):
    make, reason = OUT[case]
    sam, bam, d = anno
    before = open(bam, "rb").read()
    args, env = make(sam, bam)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert reason in p.stderr and b"[E::fade-out] --sort: " in p.stderr, p.stderr.decode()
    assert b"[W::" not in p.stderr and b"file path on the device" not in p.stderr
    assert open(bam, "rb").read() == before
    if case == "keep_sorted":
        assert b"--sort already gives the order" in p.stderr


def test_write_index_beside_sort_keeps_its_own_refusals(anno):
    sam, bam, d = anno
    for extra, reason in ((["--write-index", str(bam)], b"not the input"), (["--write-index=-"], b"not the standard output")):
        p = _run(["out", "--gpus", "1", "--sort", "-b"] + extra + [str(bam)])
        assert p.returncode == 1 and p.stdout == b"" and b"[E::fade-out] --write-index: " in p.stderr and reason in p.stderr, p.stderr.decode()


def test_piped_input_is_refused(anno):
    sam, bam, d = anno
    with open(bam, "rb") as fi:
        p = _run(["out", "--gpus", "1", "--sort", "-b", "-"], stdin=fi)
    assert p.returncode == 1 and p.stdout == b"" and b"[E::fade-out] --sort: " in p.stderr and b"not a pipe" in p.stderr, p.stderr.decode()


def test_the_help_text_lists_the_option_and_the_other_subcommands_do_not_take_it(anno):
    sam = anno[0]
    h = _run(["out", "--help"])
    assert h.returncode == 0 and b"--sort " in h.stderr and b"coordinate order" in h.stderr and b"in any order" in h.stderr
    h = _run(["annotate", "--help"])
    assert h.returncode == 0 and b"--sort " in h.stderr and b"sort in the fade out step" in h.stderr
    for args in (["extract", "--sort", str(sam)], ["stats", "--gpus", "1", "--sort", str(sam)], ["stats-clip", "--gpus", "1", "--sort", str(sam)]):
        p = _run(args)
        assert p.returncode == 1 and b"Unrecognized option --sort" in p.stderr and not p.stdout, args
    for args in (["out", "--sorted", str(sam)], ["annotate", "--sorted", str(sam), FA]):     # (--sorted stays fade extract's)
        p = _run(args)
        assert p.returncode == 1 and b"Unrecognized option" in p.stderr and not p.stdout, args
    p = _run(["out", "--sort=maybe", str(sam)])
    assert p.returncode == 1 and b"Invalid value for option --sort: maybe" in p.stderr and not p.stdout
    p = _run(["out", "--sort=false", str(sam)])                                              # (a flag, as --eject: false is no option at all)
    q = _run(["out", str(sam)])
    body = lambda out: [l for l in out.split(b"\n") if not l.startswith(b"@PG")]              # (@PG carries the command line)
    assert p.returncode == q.returncode == 0 and body(p.stdout) == body(q.stdout) and len(body(q.stdout)) > 10


def test_the_flag_and_the_exports_agree_everywhere_and_the_abi_stays(lib):
    _lib, L = lib
    header = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    dbind = open(os.path.join(ROOT, "bindings", "d", "fadehip.d")).read()
    assert re.search(r"#define FADEHIP_BAM_STORE_OUTPUT 131072\b", header)
    assert re.search(r"enum FADEHIP_BAM_STORE_OUTPUT = 131072;", dbind)
    assert _lib.BAM_STORE_OUTPUT == 131072
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(r"\bint %s\(" % name, header) and re.search(r"\bint %s\(" % name, dbind), name
        getattr(L, name)
    assert _lib.ABI_VERSION == 3 == L.fadehip_abi_version() and re.search(r"#define FADEHIP_ABI_VERSION 3\b", header)
    assert C.sizeof(_lib.BamConfig) == 32


def test_null_arguments_are_refused_before_any_device_call(lib):
    _lib, L = lib
    v32, v64, u64 = C.c_int32(0), C.c_int64(0), C.c_uint64(0)
    lens = (C.c_int64 * 2)(5, 6)
    assert L.fadehip_recstore_set_budget(None, 5) == -1
    assert L.fadehip_recstore_budget(None, C.byref(u64)) == -1
    assert L.fadehip_recstore_measure(None, 2, lens) == -1
    assert L.fadehip_recstore_over(None, C.byref(v32)) == -1
    assert L.fadehip_recstore_resets(None, C.byref(v64)) == -1
    assert L.fadehip_recstore_histogram(None, None, None, C.byref(v64)) == -1
    assert L.fadehip_recstore_set_window(None, 0, 5) == -1
    assert L.fadehip_recstore_reset(None, 0, 0) == -1
    assert b"recstore is NULL" in L.fadehip_last_error(None)
