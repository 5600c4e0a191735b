"""`fade out -c --fix-mates` and the mate map's C ABI, the part that needs no device: the new exports are in the library, the
loader, the header and the D binding, the ABI version and sizeof(fadehip_bam_config) stay what they were, NULL arguments are
refused with a message before anything reaches a device, and the option — which has no host loop behind it — is refused by
name where it cannot run; `extract` and `annotate` do not know it, and plain `fade out -c` says what it said."""
import ctypes as C
import os
import re

import pytest

from test_cli_out_fragments import ROOT, _run, anno, lib  # noqa: F401  (the fixtures)

NEW = ["fadehip_mateset_create", "fadehip_mateset_add_batch", "fadehip_mates_fix_batch", "fadehip_mateset_count", "fadehip_mateset_destroy",
       "fadehip_bam_use_mateset", "fadehip_bam_mates"]
W_FIX_MATES = (b"[W::fade-out] --fix-mates: mate fields (next position, template length, mate strand and unmapped flags, MC) follow the clip: "
               b"three passes over the file (names of the artifact reads, placements of their fragments, write)")
W_SORT = b"[W::fade-out] Using the -c flag means the output SAM/BAM will not be sorted (regardless of prior sorting)"
W_PICARD = b"[W::fade-out] You also may need to fix mate information with a tool like Picard FixMateInformation"


def test_the_symbols_are_exported_declared_and_bound_and_the_abi_is_the_same(lib):  # noqa: F811
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
    assert "#define FADEHIP_BAM_COLLECT_MATES 8192" in header and "#define FADEHIP_BAM_FIX_MATES 16384" in header
    assert (_lib.BAM_COLLECT_MATES, _lib.BAM_FIX_MATES) == (8192, 16384)
    assert "enum FADEHIP_BAM_COLLECT_MATES = 8192;" in d and "enum FADEHIP_BAM_FIX_MATES = 16384;" in d


def test_null_arguments_are_refused_with_a_message_before_any_device_call(lib):  # noqa: F811
    _, L = lib
    off = (C.c_int64 * 2)(0, 40)
    buf = (C.c_uint8 * 40)()
    i32 = (C.c_int32 * 1)(0)
    out = C.c_void_p()
    n = C.c_int64(0)
    L.fadehip_last_error.restype = C.c_char_p
    for rc in (L.fadehip_mateset_create(None, C.byref(out)),
               L.fadehip_mateset_add_batch(None, 1, buf, off, buf, i32, i32, None),
               L.fadehip_mateset_add_batch(None, 1, None, None, None, None, None, None),
               L.fadehip_mates_fix_batch(None, 1, buf, off, buf, i32, i32, buf, 40, off, buf),
               L.fadehip_mates_fix_batch(None, 1, None, None, None, None, None, None, 0, None, None),
               L.fadehip_mateset_count(None, C.byref(n), C.byref(n)),
               L.fadehip_bam_use_mateset(None, None),
               L.fadehip_bam_mates(None, C.byref(n), C.byref(n))):
        assert rc == -1
        assert L.fadehip_last_error(None), "a message says what was NULL"
    assert L.fadehip_mateset_destroy(None) is None


REFUSALS = {
    "without_clip": (lambda sam, bam: (["out", "--fix-mates", "-b", str(bam)], {}), b"goes with -c"),
    "fragments": (lambda sam, bam: (["out", "-c", "--fix-mates", "--fragments", "-b", str(bam)], {}), b"not with --fragments"),
    "sam_input": (lambda sam, bam: (["out", "-c", "--fix-mates", "-b", str(sam)], {}), b"not SAM text"),
    "sam_output": (lambda sam, bam: (["out", "-c", "--fix-mates", str(bam)], {}), b"the output is SAM text"),
    "no_device": (lambda sam, bam: (["out", "-c", "--fix-mates", "-b", str(bam)], {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "two_devices": (lambda sam, bam: (["out", "-c", "--fix-mates", "--gpus", "2", "-b", str(bam)], {}), b"one device"),
    "no_devices": (lambda sam, bam: (["out", "-c", "--fix-mates", "--gpus", "0", "-b", str(bam)], {}), b"one device"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_where_the_option_cannot_run_it_is_refused_with_its_reason_and_nothing_on_stdout(anno, case):  # noqa: F811
    make, reason = REFUSALS[case]
    args, env = make(*anno)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert b"--fix-mates" in p.stderr and reason in p.stderr, p.stderr.decode()
    assert b"read count:" not in p.stderr


def test_piped_input_is_refused(anno):  # noqa: F811
    with open(anno[1], "rb") as fi:
        p = _run(["out", "-c", "--fix-mates", "-b", "-"], stdin=fi)
    assert p.returncode == 1 and p.stdout == b"" and b"--fix-mates" in p.stderr and b"not a pipe" in p.stderr, p.stderr.decode()


def test_extract_and_annotate_do_not_know_the_option_and_the_help_of_out_names_it(anno):  # noqa: F811
    sam, bam = anno
    for args in (["extract", "--fix-mates", "-b", str(bam)], ["annotate", "-c", "--fix-mates", "-b", str(bam), str(sam)]):
        p = _run(args)
        assert p.returncode == 1 and b"Unrecognized option" in p.stderr and not p.stdout, args
    p = _run(["out", "-c", "--fix-mates=maybe", str(sam)])
    assert p.returncode == 1 and b"Invalid value for option --fix-mates" in p.stderr and not p.stdout
    h = _run(["out", "--help"])
    assert h.returncode == 0 and b"--fix-mates" in h.stderr


def test_plain_fade_out_c_of_a_sam_still_prints_both_reference_warnings(anno):  # noqa: F811
    plain = _run(["out", "-c", str(anno[0])])
    assert plain.returncode == 0 and plain.stderr.count(W_SORT) == 1 and plain.stderr.count(W_PICARD) == 1
    assert W_FIX_MATES not in plain.stderr and plain.stderr.count(b"read count:") == 1
