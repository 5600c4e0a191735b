"""`--csi` (`fade annotate`, `fade out`, `fade extract`) and its C ABI, the part that needs no device: the new exports are in the
header, the D binding and the loader, the ABI version stays 3, invalid geometries and NULL arguments are refused before
anything reaches a device, the host builder behind fade_amd.CsiBuilder gives the model's payload and file, the option is
refused by name where there is no index to write, the help texts name it, and without it every message is what it was."""
import ctypes as C
import os
import re
import subprocess

import pytest

import csi_model as cm
from test_cli_extract import _annotated_sam
from test_csi_model import seeded_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
FA = os.path.join(ROOT, "tests", "golden", "anno_c2.fa")
NEW_INT = ["fadehip_index_batch_csi", "fadehip_bam_index_geometry", "fadehip_recstore_index_geometry", "fadehip_csi_add", "fadehip_csi_finish"]
NEW_OTHER = ["fadehip_csi_create", "fadehip_csi_error", "fadehip_csi_destroy"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from fade_amd import _lib
    return _lib, _lib.load()


@pytest.fixture(scope="module")
def anno(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("csi")
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(_annotated_sam("anno_c2"))
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), str(sam)], stdout=fo)
    return sam, bam, d


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e, **kw)


def test_the_symbols_agree_everywhere_and_the_abi_is_the_same(lib):
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
    assert C.sizeof(_lib.BamConfig) == 32 and C.sizeof(_lib.IndexCall) == 72
    assert "struct fadehip_csi;" in d and "typedef struct fadehip_csi fadehip_csi;" in header


def test_python_binds_the_new_calls():
    import inspect
    import fade_amd
    from fade_amd import api
    assert callable(fade_amd.CsiBuilder) and hasattr(api.BamStream, "index_geometry") and hasattr(api.RecStore, "index_geometry")
    assert "csi" in inspect.signature(api.Context.index_batch).parameters
    for name in ("add", "finish", "file_bytes", "close"):
        assert hasattr(fade_amd.CsiBuilder, name), name


def test_null_arguments_and_invalid_geometries_are_refused_before_any_device_call(lib):
    _lib, L = lib
    off = (C.c_int64 * 2)(0, 40)
    voff = (C.c_uint64 * 2)(0, 40)
    buf = (C.c_uint8 * 40)()
    call = _lib.IndexCall()
    L.fadehip_last_error.restype = C.c_char_p
    for rc in (L.fadehip_index_batch_csi(None, 1, buf, off, voff, 14, 6, C.byref(call)),
               L.fadehip_bam_index_geometry(None, 14, 6),
               L.fadehip_recstore_index_geometry(None, 14, 6)):
        assert rc == -1
        assert L.fadehip_last_error(None), "a message says what was NULL"
    p, n = C.c_void_p(), C.c_size_t(0)
    assert L.fadehip_csi_add(None, 0, C.byref(call)) == -1 and L.fadehip_csi_error(None)
    assert L.fadehip_csi_finish(None, C.byref(p), C.byref(n)) == -1 and L.fadehip_csi_error(None)
    assert not L.fadehip_csi_create(-1, 14, 6)
    for ms, d in [(3, 2), (14, 0), (14, 9), (14, 7), (30, 1), (-1, 5)]:
        assert not L.fadehip_csi_create(2, ms, d), (ms, d)
    b = L.fadehip_csi_create(2, 14, 6)
    try:
        assert L.fadehip_csi_add(b, 0, None) == -1 and b"NULL" in L.fadehip_csi_error(b)
        assert L.fadehip_csi_finish(b, None, None) == -1 and b"NULL" in L.fadehip_csi_error(b)
        bad = _lib.IndexCall(None, None, None, 1, 0, 0, 1, 0, 0)
        assert L.fadehip_csi_add(b, 0, C.byref(bad)) == -1 and b"NULL" in L.fadehip_csi_error(b)
    finally:
        L.fadehip_csi_destroy(b)
    L.fadehip_csi_destroy(None)


@pytest.mark.parametrize("geometry", [(4, 2), (14, 6)])
def test_the_builder_behind_the_library_gives_the_models_payload_and_file(lib, geometry):
    import fade_amd
    recs = seeded_records(geometry[0], geometry[1], seed=2)
    cuts = [0, 1, 1, 300, 450, len(recs), len(recs)]
    b = fade_amd.CsiBuilder(3, *geometry)
    try:
        for lo, hi in zip(cuts, cuts[1:]):
            call = cm.per_call(recs[lo:hi], *geometry)
            base = recs[lo]["u"] >> 16 if hi > lo else 0  # (relative to the call's first member, as the device leaves them)

            def shift(v, base=base):
                return v - (base << 16)
            call = dict(call, chunks=[(t, bn, shift(u), shift(v)) for t, bn, u, v in call["chunks"]],
                        linear=[(t, w, shift(o)) for t, w, o in call["linear"]],
                        refs=[(t, shift(u), shift(v), nm, nu) for t, u, v, nm, nu in call["refs"]])
            b.add(base, call)
        want = cm.build(3, recs, *geometry)
        assert b.finish() == want
        data = b.file_bytes()
        assert data.endswith(cm.BGZF_EOF) and cm.payload_of(data) == want
        csi = cm.read_csi(cm.payload_of(data))
        assert (csi["min_shift"], csi["depth"]) == geometry
        with pytest.raises(fade_amd.FadeHipError) as e:
            b.add(0, cm.per_call(recs[:3], *geometry))
        assert e.value.code == -1 and "record %d: not in coordinate order (--write-index needs coordinate-sorted output)" % len(recs) in str(e.value)
        assert b.finish() == want
    finally:
        b.close()
    with pytest.raises(fade_amd.FadeHipError):
        fade_amd.CsiBuilder(3, 14, 7)


def _annotate(extra, inp, env=None):
    return ["annotate"] + extra + [str(inp), FA], env or {}


REFUSALS = {
    "out_no_index": (lambda sam, bam, x: (["out", "--csi", "--gpus", "1", "-b", str(bam)], {}), b"[E::fade-out] --csi: ", b"--write-index PATH"),
    "out_sort_no_index": (lambda sam, bam, x: (["out", "--csi", "--gpus", "1", "--sort", "-b", str(bam)], {}), b"[E::fade-out] --csi: ", b"--write-index PATH"),
    "out_clip_sam": (lambda sam, bam, x: (["out", "-c", "--csi", str(sam)], {}), b"[E::fade-out] --csi: ", b"--write-index PATH"),
    "annotate_no_index": (lambda sam, bam, x: _annotate(["--csi", "-b"], bam), b"[E::fade-annotate] --csi: ", b"--write-index PATH or --extract-sorted"),
    "annotate_extract_unsorted": (lambda sam, bam, x: _annotate(["--csi", "--extract", x, "-b"], bam), b"[E::fade-annotate] --csi: ", b"--extract-sorted"),
    "extract_no_index": (lambda sam, bam, x: (["extract", "--csi", "--gpus", "1", "--sorted", "-b", str(bam)], {}), b"[E::fade extract] --csi: ", b"--write-index PATH"),
    "extract_plain": (lambda sam, bam, x: (["extract", "--csi", str(sam)], {}), b"[E::fade extract] --csi: ", b"--write-index PATH"),
    # with an index to write, the index's own refusals speak, by its name, as they do without --csi
    "out_sam_output": (lambda sam, bam, x: (["out", "--write-index", x, "--csi", str(bam)], {}), b"[E::fade-out] --write-index: ", b"the output is SAM text"),
    "out_two_devices": (lambda sam, bam, x: (["out", "--write-index", x, "--csi", "--gpus", "2", "-b", str(bam)], {}), b"[E::fade-out] --write-index: ", b"--gpus N > 1"),
    "annotate_no_device": (lambda sam, bam, x: _annotate(["--write-index", x, "--csi", "-b"], bam, {"FADE_BAM_DEVICE": "0"}), b"[E::fade-annotate] --write-index: ", b"FADE_BAM_DEVICE=0"),
    "extract_unsorted": (lambda sam, bam, x: (["extract", "--write-index", x, "--csi", "-b", str(bam)], {}), b"[E::fade extract] --write-index: ", b"--sorted"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_where_the_option_cannot_run_it_is_refused_by_name_and_nothing_is_written(anno, case):
    make, who, reason = REFUSALS[case]
    sam, bam, d = anno
    x = str(d / (case + ".csi"))
    before = open(bam, "rb").read()
    args, env = make(sam, bam, x)
    p = _run(args, env)
    assert p.returncode == 1 and p.stdout == b"", p.stderr.decode()
    assert who in p.stderr and reason in p.stderr, p.stderr.decode()
    assert b"read count:" not in p.stderr and b"[W::" not in p.stderr
    assert not os.path.exists(x) and not os.path.exists(x + ".csi") and open(bam, "rb").read() == before


def test_other_subcommands_do_not_know_the_option_and_the_help_texts_name_it(anno):
    sam, bam, d = anno
    for sub in ("stats", "stats-clip"):
        p = _run([sub, "--gpus", "1", "--csi", str(bam)])
        assert p.returncode == 1 and b"Unrecognized option --csi" in p.stderr and not p.stdout, p.stderr.decode()
    for sub in ("out", "annotate", "extract"):
        p = _run([sub, "--csi=maybe", str(sam)])
        assert p.returncode == 1 and b"Invalid value for option --csi" in p.stderr and not p.stdout
        p = _run([sub, "-J", str(sam)])
        assert p.returncode == 1 and b"Unrecognized option -J" in p.stderr and not p.stdout
        h = _run([sub, "--help"])
        assert h.returncode == 0 and re.search(rb"--csi with --write-index.*CSI", h.stderr), h.stderr.decode()


def test_without_the_option_every_message_is_what_it_was(anno):
    sam = anno[0]
    plain = _run(["out", str(sam)])
    assert plain.returncode == 0 and b"csi" not in plain.stderr.lower() and plain.stdout.count(b"\n") > 100
    off = _run(["out", "--csi=false", str(sam)])
    def body(out):  # (the @PG line quotes the command line)
        return [ln for ln in out.split(b"\n") if not ln.startswith(b"@PG")]
    assert off.returncode == 0 and body(off.stdout) == body(plain.stdout) and off.stderr == plain.stderr
