"""`fade extract --gpus 1 --sorted [--write-index PATH]` and `fade annotate --extract PATH --extract-sorted`, the part that needs
no device: neither option has a host loop behind it, so where it cannot run it is refused by name, with its reason, before
a device is opened and with nothing on stdout; both help texts list the new options; the flag and the new exports agree in
the header, the D binding and the loader, and the ABI stays what it was."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_cli_extract import _annotated_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
FA = os.path.join(ROOT, "tests", "golden", "anno_c2.fa")
NEW = ["fadehip_recstore_create", "fadehip_recstore_add_batch", "fadehip_recstore_count", "fadehip_recstore_sort", "fadehip_recstore_drain", "fadehip_bam_use_recstore"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from fade_amd import _lib
    return _lib, _lib.load()


@pytest.fixture(scope="module")
def anno(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("extract_sorted")
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(_annotated_sam("anno_c2"))
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), str(sam)], stdout=fo)
    return sam, bam, d


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e, **kw)


def _annotate(extra, inp, env=None):
    return ["annotate"] + extra + [str(inp), FA], env or {}


EXTRACT = {
    "sam_output": (lambda sam, bam, x: (["extract", "--gpus", "1", "--sorted", str(bam)], {}), b"the output is SAM text"),
    "sam_input": (lambda sam, bam, x: (["extract", "--gpus", "1", "--sorted", "-b", str(sam)], {}), b"not SAM text"),
    "no_device": (lambda sam, bam, x: (["extract", "--gpus", "1", "--sorted", "-b", str(bam)], {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "two_devices": (lambda sam, bam, x: (["extract", "--gpus", "2", "--sorted", "-u", str(bam)], {}), b"--gpus N > 1"),
    "out_shards": (lambda sam, bam, x: (["extract", "--gpus", "1", "--sorted", "--out-shards", x, "-b", str(bam)], {}), b"--out-shards"),
    "without_gpus": (lambda sam, bam, x: (["extract", "--sorted", "-b", str(bam)], {}), b"it goes with --gpus 1"),
    "index_with_sam_output": (lambda sam, bam, x: (["extract", "--gpus", "1", "--sorted", "--write-index", x, str(bam)], {}), b"the output is SAM text"),
    "index_is_the_input": (lambda sam, bam, x: (["extract", "--gpus", "1", "--sorted", "--write-index", str(bam), "-b", str(bam)], {}), b"not the input"),
    "index_is_stdout": (lambda sam, bam, x: (["extract", "--gpus", "1", "--sorted", "--write-index=-", "-b", str(bam)], {}), b"not the standard output"),
}
ANNOTATE = {
    "sam_output": (lambda sam, bam, x: _annotate(["--extract", x, "--extract-sorted"], bam), b"the output is SAM text"),
    "sam_input": (lambda sam, bam, x: _annotate(["--extract", x, "--extract-sorted", "-b"], sam), b"not SAM text"),
    "no_device": (lambda sam, bam, x: _annotate(["--extract", x, "--extract-sorted", "-u"], bam, {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "without_extract": (lambda sam, bam, x: _annotate(["--extract-sorted", "-b"], bam), b"the option goes with --extract PATH"),
}


@pytest.mark.parametrize("case", list(EXTRACT))
def test_extract_sorted_is_refused_by_name_where_it_cannot_run(anno, case):
    make, reason = EXTRACT[case]
    sam, bam, d = anno
    x = str(d / (case + ".bai"))
    before = open(bam, "rb").read()
    args, env = make(sam, bam, x)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert reason in p.stderr, p.stderr.decode()
    assert (b"[E::fade extract] --write-index: " if case.startswith("index_is") else b"[E::fade extract] --out-shards: " if case == "out_shards" else b"[E::fade extract] --sorted: ") in p.stderr, p.stderr.decode()
    assert b"[W::" not in p.stderr and b"file path on the device" not in p.stderr
    assert not os.path.exists(x) and open(bam, "rb").read() == before


@pytest.mark.parametrize("case", list(ANNOTATE))
def test_extract_sorted_of_annotate_is_refused_by_name_where_it_cannot_run(anno, case):
    make, reason = ANNOTATE[case]
    sam, bam, d = anno
    x = str(d / (case + ".extract.bam"))
    args, env = make(sam, bam, x)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert reason in p.stderr and b"[E::fade-annotate] --extract-sorted: " in p.stderr, p.stderr.decode()
    assert b"[W::" not in p.stderr and not os.path.exists(x) and not os.path.exists(x + ".bai")


def test_more_than_one_device_is_refused_for_annotate_by_the_option_it_meets_first(anno):
    sam, bam, d = anno
    x = str(d / "two.extract.bam")
    for extra in (["--gpus", "2"], ["--gpus", "2", "--out-shards", str(d / "s")], ["--out-shards", str(d / "s")]):
        p = _run(["annotate", "-b", "--extract", x, "--extract-sorted"] + extra + [str(bam), FA])
        # (--extract itself goes with one device, and says so first; without it the new option's own check is met)
        assert p.returncode == 1 and p.stdout == b"" and b"--extract goes with one device" in p.stderr, p.stderr.decode()
        p = _run(["annotate", "-b", "--extract-sorted"] + extra + [str(bam), FA])
        assert p.returncode == 1 and p.stdout == b"" and b"[E::fade-annotate] --extract-sorted: " in p.stderr, p.stderr.decode()
    assert not os.path.exists(x)


def test_write_index_without_sorted_is_refused_by_name(anno):
    sam, bam, d = anno
    x = str(d / "unsorted.bai")
    for extra in ([], ["--gpus", "1"]):
        p = _run(["extract", "--write-index", x, "-b"] + extra + [str(bam)])
        assert p.returncode == 1 and p.stdout == b"" and b"[E::fade extract] --write-index: " in p.stderr and b"the option goes with --sorted" in p.stderr, p.stderr.decode()
    assert not os.path.exists(x)


def test_piped_input_is_refused(anno):
    sam, bam, d = anno
    x = str(d / "piped.extract.bam")
    for args, who in ((["extract", "--gpus", "1", "--sorted", "-b", "-"], b"--sorted: "), (["annotate", "--extract", x, "--extract-sorted", "-b", "-", FA], b"--extract-sorted: ")):
        with open(bam, "rb") as fi:
            p = _run(args, stdin=fi)
        assert p.returncode == 1 and p.stdout == b"" and who in p.stderr and b"not a pipe" in p.stderr, p.stderr.decode()
    assert not os.path.exists(x)


def test_both_help_texts_list_the_new_options_and_the_other_subcommands_do_not_take_them(anno):
    sam = anno[0]
    h = _run(["extract", "--help"])
    assert h.returncode == 0 and b"--sorted" in h.stderr and b"--write-index PATH" in h.stderr
    h = _run(["annotate", "--help"])
    assert h.returncode == 0 and b"--extract-sorted" in h.stderr and b"PATH.bai" in h.stderr
    for args in (["out", "--sorted", str(sam)], ["out", "--extract-sorted", str(sam)], ["annotate", "--sorted", str(sam), FA], ["extract", "--extract-sorted", str(sam)],
                 ["stats", "--gpus", "1", "--sorted", str(sam)]):
        p = _run(args)
        assert p.returncode == 1 and b"Unrecognized option" in p.stderr and not p.stdout, args
    p = _run(["extract", "--sorted=maybe", str(sam)])
    assert p.returncode == 1 and b"Invalid value for option --sorted" in p.stderr and not p.stdout


def test_without_the_options_every_message_is_what_it_was(anno):
    sam = anno[0]
    p = _run(["extract", str(sam)])
    assert p.returncode == 0 and p.stderr.count(b"[W::fade extract] Output SAM/BAM will not be sorted") == 1 and b"--sorted" not in p.stderr and p.stdout.count(b"\n") > 20


def test_the_flag_and_the_symbols_agree_everywhere_and_the_abi_is_the_same(lib):
    _lib, L = lib
    header = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    d = open(os.path.join(ROOT, "bindings", "d", "fadehip.d")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(r"^int\s+%s\(" % name, header, flags=re.M) and re.search(r"^int\s+%s\(" % name, d, flags=re.M), name
    assert hasattr(L, "fadehip_recstore_destroy") and "void fadehip_recstore_destroy(" in header and "void fadehip_recstore_destroy(" in d
    assert L.fadehip_abi_version() == 3 and _lib.ABI_VERSION == 3 and "#define FADEHIP_ABI_VERSION 3" in header
    assert C.sizeof(_lib.BamConfig) == 32
    assert "#define FADEHIP_BAM_STORE_EXTRACT 32768" in header and "enum FADEHIP_BAM_STORE_EXTRACT = 32768;" in d and _lib.BAM_STORE_EXTRACT == 32768
    for name, v in (("RAW", 1), ("STORED", 2), ("INDEX", 4)):
        assert "#define FADEHIP_RECSTORE_%s %d" % (name, v) in header and "enum FADEHIP_RECSTORE_%s = %d;" % (name, v) in d and getattr(_lib, "RECSTORE_" + name) == v


def test_null_arguments_are_refused_with_a_message_before_any_device_call(lib):
    _lib, L = lib
    L.fadehip_last_error.restype = C.c_char_p
    p, n, nr = C.c_void_p(), C.c_size_t(0), C.c_int64(0)
    off = (C.c_int64 * 1)(0)
    for rc in (L.fadehip_recstore_create(None, C.byref(p)), L.fadehip_recstore_add_batch(None, 0, None, off, None), L.fadehip_recstore_count(None, C.byref(nr), C.byref(nr)),
               L.fadehip_recstore_sort(None), L.fadehip_recstore_drain(None, 0, 1, C.byref(p), C.byref(n), C.byref(nr), None), L.fadehip_bam_use_recstore(None, None)):
        assert rc == -1 and L.fadehip_last_error(None)
    L.fadehip_recstore_destroy(None)


def test_python_binds_the_store():
    import inspect
    from fade_amd import api
    assert hasattr(api.Context, "recstore") and all(hasattr(api.RecStore, m) for m in ("add_batch", "count", "sort", "drain", "close"))
    assert "recstore" in inspect.signature(api.Context.bam_stream).parameters
