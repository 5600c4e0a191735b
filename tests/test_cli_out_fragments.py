"""`fade out --fragments` and the name set's C ABI, the part that needs no device: the six exports are in the library, the
loader, the header and the D binding, the ABI version and sizeof(fadehip_bam_config) stay what they were, NULL arguments
are refused before anything reaches a device, and the option — which has no host loop behind it — is refused by name where
it cannot run; `extract` and `annotate` do not know it."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cli_extract import _annotated_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
NEW = ["fadehip_nameset_create", "fadehip_nameset_add_batch", "fadehip_nameset_contains_batch", "fadehip_nameset_count",
       "fadehip_nameset_destroy", "fadehip_bam_use_nameset"]
W_FRAGMENTS = b"[W::fade-out] --fragments: ejecting every read that shares its name with an artifact read, input in any order (two passes over the file)"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from fade_amd import _lib
    return _lib, _lib.load()


@pytest.fixture(scope="module")
def anno(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("out_fragments")
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(_annotated_sam("anno_c2"))
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), str(sam)], stdout=fo)
    return sam, bam


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e, **kw)


def test_the_six_symbols_are_exported_declared_and_bound_and_the_abi_is_the_same(lib):
    _lib, L = lib
    header = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    d = open(os.path.join(ROOT, "bindings", "d", "fadehip.d")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"^(int|void)\s+%s\(" % name, header, flags=re.M), name
        assert re.search(r"^(int|void)\s+%s\(" % name, d, flags=re.M), name
    assert L.fadehip_abi_version() == 3 and _lib.ABI_VERSION == 3 and "#define FADEHIP_ABI_VERSION 3" in header
    assert C.sizeof(_lib.BamConfig) == 32
    assert "#define FADEHIP_BAM_COLLECT_NAMES 128" in header and "#define FADEHIP_BAM_EJECT_NAMED 256" in header
    assert (_lib.BAM_COLLECT_NAMES, _lib.BAM_EJECT_NAMED) == (128, 256)
    assert "enum FADEHIP_BAM_COLLECT_NAMES = 128;" in d and "enum FADEHIP_BAM_EJECT_NAMED = 256;" in d


def test_null_arguments_are_refused_with_a_message_before_any_device_call(lib):
    _, L = lib
    off = (C.c_int64 * 2)(0, 40)
    buf = (C.c_uint8 * 40)()
    out = C.c_void_p()
    n = C.c_int64(0)
    L.fadehip_last_error.restype = C.c_char_p
    for rc in (L.fadehip_nameset_create(None, C.byref(out)),
               L.fadehip_nameset_add_batch(None, 1, buf, off, None),
               L.fadehip_nameset_add_batch(None, 1, None, None, None),
               L.fadehip_nameset_contains_batch(None, 1, buf, off, buf),
               L.fadehip_nameset_contains_batch(None, 1, None, None, None),
               L.fadehip_nameset_count(None, C.byref(n)),
               L.fadehip_bam_use_nameset(None, None)):
        assert rc == -1
        assert L.fadehip_last_error(None), "a message says what was NULL"
    assert L.fadehip_nameset_destroy(None) is None


REFUSALS = {
    "sam_input": (lambda sam, bam: (["out", "--fragments", "-b", str(sam)], {}), b"not SAM text"),
    "sam_output": (lambda sam, bam: (["out", "--fragments", str(bam)], {}), b"the output is SAM text"),
    "no_device": (lambda sam, bam: (["out", "--fragments", "-b", str(bam)], {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "clip": (lambda sam, bam: (["out", "--fragments", "-c", "-b", str(bam)], {}), b"-c clips"),
    "two_devices": (lambda sam, bam: (["out", "--fragments", "--gpus", "2", "-b", str(bam)], {}), b"--gpus 2"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_where_the_option_cannot_run_it_is_refused_with_its_reason_and_nothing_on_stdout(anno, case):
    make, reason = REFUSALS[case]
    args, env = make(*anno)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert reason in p.stderr, p.stderr.decode()
    assert b"read count:" not in p.stderr


def test_piped_input_is_refused(anno):
    with open(anno[1], "rb") as fi:
        p = _run(["out", "--fragments", "-b", "-"], stdin=fi)
    assert p.returncode == 1 and p.stdout == b"" and b"not a pipe" in p.stderr, p.stderr.decode()


def test_extract_and_annotate_do_not_know_the_option_and_the_help_of_out_names_it(anno):
    sam, bam = anno
    for args in (["extract", "--fragments", "-b", str(bam)], ["annotate", "--fragments", "-b", str(bam), str(sam)]):
        p = _run(args)
        assert p.returncode == 1 and b"Unrecognized option" in p.stderr and not p.stdout, args
    p = _run(["out", "-F", str(sam)])
    assert p.returncode == 1 and b"Unrecognized option -F" in p.stderr and not p.stdout
    p = _run(["out", "--fragments=maybe", str(sam)])
    assert p.returncode == 1 and b"Invalid value for option --fragments" in p.stderr and not p.stdout
    h = _run(["out", "--help"])
    assert h.returncode == 0 and b"--fragments" in h.stderr
    # without the option nothing changes: plain `fade out` of the SAM still runs on the host and says what it said
    plain = _run(["out", str(sam)])
    assert plain.returncode == 0 and W_FRAGMENTS not in plain.stderr and plain.stderr.count(b"read count:") == 1
