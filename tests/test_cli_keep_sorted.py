"""`--keep-sorted` (`fade annotate -c`, `fade out -c`) and its C ABI, the part that needs no device: the flag's value agrees in
the header, the D binding and the loader, the two new exports are there, the ABI version and sizeof(fadehip_bam_config)
stay what they were, NULL arguments are refused before anything reaches a device, and the option — which has no host loop
behind it — is refused by name, with its reason, where it cannot run; `extract` does not know it."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cli_extract import _annotated_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
FA = os.path.join(ROOT, "tests", "golden", "anno_c2.fa")
NEW = ["fadehip_bam_held", "fadehip_coord_order_batch"]
W_OLD = b"[W::fade-out] Using the -c flag means the output SAM/BAM will not be sorted (regardless of prior sorting)"
W_MATES = b"[W::fade-out] You also may need to fix mate information with a tool like Picard FixMateInformation"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from fade_amd import _lib
    return _lib, _lib.load()


@pytest.fixture(scope="module")
def anno(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("keep_sorted")
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(_annotated_sam("anno_c2"))
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), str(sam)], stdout=fo)
    return sam, bam


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e, **kw)


def test_the_flag_and_the_two_symbols_agree_everywhere_and_the_abi_is_the_same(lib):
    _lib, L = lib
    header = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    d = open(os.path.join(ROOT, "bindings", "d", "fadehip.d")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"^int\s+%s\(" % name, header, flags=re.M), name
        assert re.search(r"^int\s+%s\(" % name, d, flags=re.M), name
    assert L.fadehip_abi_version() == 3 and _lib.ABI_VERSION == 3 and "#define FADEHIP_ABI_VERSION 3" in header
    assert C.sizeof(_lib.BamConfig) == 32
    assert "#define FADEHIP_BAM_KEEP_SORTED 512" in header and "enum FADEHIP_BAM_KEEP_SORTED = 512;" in d and _lib.BAM_KEEP_SORTED == 512


def test_null_arguments_are_refused_with_a_message_before_any_device_call(lib):
    _, L = lib
    off = (C.c_int64 * 2)(0, 40)
    buf = (C.c_uint8 * 40)()
    order = (C.c_int32 * 1)()
    n = C.c_int64(0)
    L.fadehip_last_error.restype = C.c_char_p
    for rc in (L.fadehip_bam_held(None, C.byref(n), C.byref(n)),
               L.fadehip_bam_held(None, None, None),
               L.fadehip_coord_order_batch(None, 1, buf, off, order),
               L.fadehip_coord_order_batch(None, 1, None, None, None),
               L.fadehip_coord_order_batch(None, 0, None, None, None)):
        assert rc == -1
        assert L.fadehip_last_error(None), "a message says what was NULL"


def _annotate(extra, inp, env=None):
    return ["annotate"] + extra + [str(inp), FA], env or {}


REFUSALS = {
    "out_without_clip": (lambda sam, bam: (["out", "--keep-sorted", "-b", str(bam)], {}), b"without -c"),
    "out_fragments": (lambda sam, bam: (["out", "-c", "--keep-sorted", "--fragments", "-b", str(bam)], {}), b"not with --fragments"),
    "out_sam_output": (lambda sam, bam: (["out", "-c", "--keep-sorted", str(bam)], {}), b"the output is SAM text"),
    "out_sam_input": (lambda sam, bam: (["out", "-c", "--keep-sorted", "-b", str(sam)], {}), b"not SAM text"),
    "out_no_device": (lambda sam, bam: (["out", "-c", "--keep-sorted", "-b", str(bam)], {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "out_two_devices": (lambda sam, bam: (["out", "-c", "--keep-sorted", "--gpus", "2", "-b", str(bam)], {}), b"--gpus N > 1"),
    "annotate_without_clip": (lambda sam, bam: _annotate(["--keep-sorted", "-b"], bam), b"without -c"),
    "annotate_eject": (lambda sam, bam: _annotate(["-c", "--keep-sorted", "--eject", "-b"], bam), b"--eject"),
    "annotate_sam_output": (lambda sam, bam: _annotate(["-c", "--keep-sorted"], bam), b"the output is SAM text"),
    "annotate_sam_input": (lambda sam, bam: _annotate(["-c", "--keep-sorted", "-u"], sam), b"not SAM text"),
    "annotate_no_device": (lambda sam, bam: _annotate(["-c", "--keep-sorted", "-b"], bam, {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "annotate_two_devices": (lambda sam, bam: _annotate(["-c", "--keep-sorted", "--gpus", "2", "-b"], bam), b"--gpus N > 1"),
    "annotate_out_shards": (lambda sam, bam: _annotate(["-c", "--keep-sorted", "--gpus", "2", "--out-shards", "x", "-b"], bam), b"--out-shards"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_where_the_option_cannot_run_it_is_refused_with_its_reason_and_nothing_on_stdout(anno, case):
    make, reason = REFUSALS[case]
    args, env = make(*anno)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert reason in p.stderr, p.stderr.decode()
    assert (b"[E::fade-out] --keep-sorted: " if case.startswith("out") else b"[E::fade-annotate] --keep-sorted: ") in p.stderr, p.stderr.decode()
    assert b"read count:" not in p.stderr and b"[W::fade-out]" not in p.stderr


def test_piped_input_is_refused(anno):
    for args in (["out", "-c", "--keep-sorted", "-b", "-"], ["annotate", "-c", "--keep-sorted", "-b", "-", FA]):
        with open(anno[1], "rb") as fi:
            p = _run(args, stdin=fi)
        assert p.returncode == 1 and p.stdout == b"" and b"--keep-sorted: " in p.stderr and b"not a pipe" in p.stderr, p.stderr.decode()


def test_extract_does_not_know_the_option_and_the_help_of_annotate_and_out_names_it(anno):
    sam, bam = anno
    p = _run(["extract", "--keep-sorted", "-b", str(bam)])
    assert p.returncode == 1 and b"Unrecognized option" in p.stderr and not p.stdout
    for sub in (["out"], ["annotate"]):
        p = _run(sub + ["-K", str(sam)])
        assert p.returncode == 1 and b"Unrecognized option -K" in p.stderr and not p.stdout
        p = _run(sub + ["--keep-sorted=maybe", str(sam)])
        assert p.returncode == 1 and b"Invalid value for option --keep-sorted" in p.stderr and not p.stdout
        h = _run(sub + ["--help"])
        assert h.returncode == 0 and b"--keep-sorted" in h.stderr
    # --keep-sorted=false is the option not given
    p = _run(["out", "--keep-sorted=false", "-c", str(sam)])
    assert p.returncode == 0 and W_OLD in p.stderr and W_MATES in p.stderr and b"--keep-sorted" not in p.stderr


def test_without_the_option_every_message_is_what_it_was(anno):
    sam, _ = anno
    plain = _run(["out", "-c", str(sam)])
    assert plain.returncode == 0 and plain.stderr.count(W_OLD) == 1 and plain.stderr.count(W_MATES) == 1 and b"--keep-sorted" not in plain.stderr
    assert plain.stdout.count(b"\n") > 100
