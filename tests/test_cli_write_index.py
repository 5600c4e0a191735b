"""`--write-index PATH` (`fade annotate`, `fade out`) and its C ABI, the part that needs no device: the flag's value agrees in
the header, the D binding and the loader, the new exports are there, the ABI version and sizeof(fadehip_bam_config) stay what
they were, NULL arguments are refused with a message before anything reaches a device, the host builder behind
fade_amd.BaiBuilder gives the model's bytes, and the option — which has no host loop behind it — is refused by name, with
its reason, where it cannot run; `extract` does not know it."""
import ctypes as C
import os
import re
import subprocess

import pytest

import bai_model as bm
from test_bai_model import laid_out
from test_cli_extract import _annotated_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
FA = os.path.join(ROOT, "tests", "golden", "anno_c2.fa")
NEW_INT = ["fadehip_index_batch", "fadehip_bam_back_index", "fadehip_bai_add", "fadehip_bai_finish"]
NEW_OTHER = ["fadehip_bai_create", "fadehip_bai_error", "fadehip_bai_destroy"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from fade_amd import _lib
    return _lib, _lib.load()


@pytest.fixture(scope="module")
def anno(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("write_index")
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(_annotated_sam("anno_c2"))
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), str(sam)], stdout=fo)
    return sam, bam, d


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e, **kw)


def test_the_flag_and_the_symbols_agree_everywhere_and_the_abi_is_the_same(lib):
    _lib, L = lib
    header = open(os.path.join(ROOT, "include", "fadehip.h")).read()
    d = open(os.path.join(ROOT, "bindings", "d", "fadehip.d")).read()
    for name in NEW_INT + NEW_OTHER:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"^[a-z_ ()*]+\b%s\(" % name, header, flags=re.M), name
        assert re.search(r"^[a-z_ ()*]+\b%s\(" % name, d, flags=re.M), name
    for name in NEW_INT:
        assert re.search(r"^int\s+%s\(" % name, header, flags=re.M) and re.search(r"^int\s+%s\(" % name, d, flags=re.M), name
    assert L.fadehip_abi_version() == 3 and _lib.ABI_VERSION == 3 and "#define FADEHIP_ABI_VERSION 3" in header
    assert C.sizeof(_lib.BamConfig) == 32
    assert "#define FADEHIP_BAM_INDEX 4096" in header and "enum FADEHIP_BAM_INDEX = 4096;" in d and _lib.BAM_INDEX == 4096
    assert C.sizeof(_lib.IndexCall) == 72
    for struct in ("fadehip_index_chunk", "fadehip_index_linear", "fadehip_index_ref", "fadehip_index_call"):
        assert struct in header and "struct " + struct in d


def test_python_binds_the_new_calls():
    import fade_amd
    from fade_amd import api
    assert callable(fade_amd.BaiBuilder) and hasattr(api.Context, "index_batch") and hasattr(api.BamStream, "back_index")
    import inspect
    assert "index" in inspect.signature(api.Context.bam_stream).parameters


def test_null_arguments_are_refused_with_a_message_before_any_device_call(lib):
    _lib, L = lib
    off = (C.c_int64 * 2)(0, 40)
    voff = (C.c_uint64 * 2)(0, 40)
    buf = (C.c_uint8 * 40)()
    call = _lib.IndexCall()
    L.fadehip_last_error.restype = C.c_char_p
    for rc in (L.fadehip_index_batch(None, 1, buf, off, voff, C.byref(call)),
               L.fadehip_index_batch(None, 0, None, None, None, None),
               L.fadehip_bam_back_index(None, C.byref(call)),
               L.fadehip_bam_back_index(None, None)):
        assert rc == -1
        assert L.fadehip_last_error(None), "a message says what was NULL"
    p, n = C.c_void_p(), C.c_size_t(0)
    assert L.fadehip_bai_add(None, 0, C.byref(call)) == -1 and L.fadehip_bai_error(None)
    assert L.fadehip_bai_finish(None, C.byref(p), C.byref(n)) == -1 and L.fadehip_bai_error(None)
    assert not L.fadehip_bai_create(-1)
    b = L.fadehip_bai_create(2)
    try:
        assert L.fadehip_bai_add(b, 0, None) == -1 and b"NULL" in L.fadehip_bai_error(b)
        assert L.fadehip_bai_finish(b, None, None) == -1 and b"NULL" in L.fadehip_bai_error(b)
        bad = _lib.IndexCall(None, None, None, 1, 0, 0, 1, 0, 0)
        assert L.fadehip_bai_add(b, 0, C.byref(bad)) == -1 and b"NULL" in L.fadehip_bai_error(b)
    finally:
        L.fadehip_bai_destroy(b)
    L.fadehip_bai_destroy(None)


def test_the_builder_behind_the_library_gives_the_models_bytes(lib):
    import random
    import fade_amd
    rng = random.Random(2)
    specs, pos = [], 0
    for tid in (0, 3):
        pos = 0
        for _ in range(400):
            pos += rng.choice([0, 3, 200, 9000])
            specs.append((tid, pos, rng.choice([0, 1, 100, 40_000]), 4 if rng.random() < 0.05 else 0))
    specs += [(-1, -1, 0, 4)] * 5
    recs = laid_out(specs, size=211, block=0x7f00, member=9000)
    cuts = [0, 1, 1, 300, 640, len(recs), len(recs)]
    b = fade_amd.BaiBuilder(5)
    try:
        for lo, hi in zip(cuts, cuts[1:]):
            call = bm.per_call(recs[lo:hi])
            # (relative to the call's first member, as the device leaves them)
            base = recs[lo]["u"] >> 16 if hi > lo else 0

            def shift(v, base=base):
                return v - (base << 16)
            call = dict(call, chunks=[(t, bn, shift(u), shift(v)) for t, bn, u, v in call["chunks"]],
                        linear=[(t, w, shift(o)) for t, w, o in call["linear"]],
                        refs=[(t, shift(u), shift(v), nm, nu) for t, u, v, nm, nu in call["refs"]])
            b.add(base, call)
        assert b.finish() == bm.build(5, recs)
        with pytest.raises(fade_amd.FadeHipError) as e:
            b.add(0, bm.per_call(recs[:3]))
        assert e.value.code == -1 and "record %d: not in coordinate order (--write-index needs coordinate-sorted output)" % len(recs) in str(e.value)
    finally:
        b.close()


def _annotate(extra, inp, env=None):
    return ["annotate"] + extra + [str(inp), FA], env or {}


REFUSALS = {
    "out_sam_output": (lambda sam, bam, x: (["out", "--write-index", x, str(bam)], {}), b"the output is SAM text"),
    "out_sam_input": (lambda sam, bam, x: (["out", "--write-index", x, "-b", str(sam)], {}), b"not SAM text"),
    "out_no_device": (lambda sam, bam, x: (["out", "-c", "--write-index", x, "-b", str(bam)], {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "out_two_devices": (lambda sam, bam, x: (["out", "--write-index", x, "--gpus", "2", "-b", str(bam)], {}), b"--gpus N > 1"),
    "out_index_is_the_input": (lambda sam, bam, x: (["out", "--write-index", str(bam), "-b", str(bam)], {}), b"not the input"),
    "out_index_is_stdout": (lambda sam, bam, x: (["out", "--write-index=-", "-u", str(bam)], {}), b"not the standard output"),
    "annotate_sam_output": (lambda sam, bam, x: _annotate(["--write-index", x], bam), b"the output is SAM text"),
    "annotate_sam_input": (lambda sam, bam, x: _annotate(["--write-index", x, "-u"], sam), b"not SAM text"),
    "annotate_no_device": (lambda sam, bam, x: _annotate(["--write-index", x, "-b"], bam, {"FADE_BAM_DEVICE": "0"}), b"FADE_BAM_DEVICE=0"),
    "annotate_two_devices": (lambda sam, bam, x: _annotate(["--write-index", x, "--gpus", "2", "-b"], bam), b"--gpus N > 1"),
    "annotate_out_shards": (lambda sam, bam, x: _annotate(["--write-index", x, "--gpus", "2", "--out-shards", "x", "-b"], bam), b"--gpus N > 1"),
    "annotate_out_shards_alone": (lambda sam, bam, x: _annotate(["--write-index", x, "--out-shards", "x", "-b"], bam), b"--out-shards"),
    "annotate_reports": (lambda sam, bam, x: _annotate(["--write-index", x, "--stats-tsv", x + ".tsv", "-b"], bam), b"--stats-tsv"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_where_the_option_cannot_run_it_is_refused_with_its_reason_and_nothing_is_written(anno, case):
    make, reason = REFUSALS[case]
    sam, bam, d = anno
    x = str(d / (case + ".bai"))
    before = open(bam, "rb").read()
    args, env = make(sam, bam, x)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert reason in p.stderr, p.stderr.decode()
    assert (b"[E::fade-out] --write-index: " if case.startswith("out") else b"[E::fade-annotate] --write-index: ") in p.stderr, p.stderr.decode()
    assert b"read count:" not in p.stderr and b"[W::" not in p.stderr
    assert not os.path.exists(x) and open(bam, "rb").read() == before


def test_piped_input_is_refused(anno):
    x = str(anno[2] / "piped.bai")
    for args in (["out", "--write-index", x, "-b", "-"], ["annotate", "--write-index", x, "-b", "-", FA]):
        with open(anno[1], "rb") as fi:
            p = _run(args, stdin=fi)
        assert p.returncode == 1 and p.stdout == b"" and b"--write-index: " in p.stderr and b"not a pipe" in p.stderr, p.stderr.decode()
    assert not os.path.exists(x)


def test_extract_does_not_know_the_option_and_the_help_of_annotate_and_out_names_it(anno):
    sam, bam, d = anno
    p = _run(["extract", "--write-index", str(d / "x.bai"), "-b", str(bam)])
    assert p.returncode == 1 and b"Unrecognized option" in p.stderr and not p.stdout
    for sub in (["out"], ["annotate"]):
        p = _run(sub + ["-I", str(sam)])
        assert p.returncode == 1 and b"Unrecognized option -I" in p.stderr and not p.stdout
        p = _run(sub + ["--write-index=", str(sam)])
        assert p.returncode == 1 and b"Invalid value for option --write-index" in p.stderr and not p.stdout
        p = _run(sub + [str(sam), "--write-index"])
        assert p.returncode == 1 and b"Missing value for argument --write-index" in p.stderr and not p.stdout
        h = _run(sub + ["--help"])
        assert h.returncode == 0 and b"--write-index PATH" in h.stderr


def test_without_the_option_every_message_is_what_it_was(anno):
    sam = anno[0]
    plain = _run(["out", str(sam)])
    assert plain.returncode == 0 and b"--write-index" not in plain.stderr and plain.stdout.count(b"\n") > 100
