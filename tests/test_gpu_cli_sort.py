"""`fade out --gpus 1 --sort [-c [--fix-mates]] [--fragments] [--write-index PATH]` on the golden annotated BAMs with their
records shuffled and on 30,000 synthetic reads: the records are tests/sorted_out_model.py's order of what the same command
line writes without --sort, byte for byte; the header says SO:coordinate and keeps its @PG lines; the end-of-file marker is
there; the index is tests/bai_model.py's over the written file; stdout may be a file or a pipe; and a budget too small for
the file gives the same records in several windows, with one warning line and one OutStats block.  `fade annotate [-c] --sort
[--write-index PATH]` on the golden inputs is held the same way, and fails with nothing on stdout when its one window does not
fit.  Without --sort the device path writes what the host loops write, which this change does not touch."""
import gzip
import subprocess

import pytest

import bai_model as bm
import bai_reader as br
import recstore_model as rm
import sorted_out_model as sm
import test_gpu_bam_from_tags as ft
import test_gpu_cli_extract_sorted as xs
from test_cli_extract import _annotated_sam
from test_gpu_annotate_clip import FADE, _bam_of, _ok, _run
from test_gpu_bgzf import EOF_MARK
from test_gpu_cli_extract_sorted import gold  # noqa: F401  (the fixture: the golden inputs as BAM, their FASTA and options)
from test_gpu_cli_out_device import _said, big  # noqa: F401  (big: the fixture)
from test_gpu_sorted_out import _is_reset

pytestmark = pytest.mark.gpu

STATS_LINE = b"Artifact rate left only"     # a line of the OutStats block (stats.d)


@pytest.fixture(scope="module", params=["anno_c2", "anno_c5"])
def shuffled(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_sort_" + request.param)
    sam, bam = d / "anno.sam", d / "anno.bam"
    sam.write_text("\n".join(ft._shuffled(_annotated_sam(request.param).splitlines())) + "\n")
    _bam_of(sam, bam)
    return bam, d, sam


def _ref_len(data):
    raw = gzip.decompress(data)
    at = 8 + int.from_bytes(raw[4:8], "little")
    n = int.from_bytes(raw[at:at + 4], "little")
    at += 4
    out = []
    for _ in range(n):
        ln = int.from_bytes(raw[at:at + 4], "little")
        out.append(int.from_bytes(raw[at + 4 + ln:at + 8 + ln], "little"))
        at += 8 + ln
    return out


def _hold(data, plain, src, clip, *options):
    """`data` (the sorted file) against `plain` (what the command writes without --sort) and `src` (the input): the records in
    the model's order, the header, the marker.  Returns (the written records, their reset flags)."""
    want = xs._records(plain)
    reset = [_is_reset(a, b) for a, b in zip(xs._records(src), want)] if clip else None
    assert xs._records(data) == sm.order(want, reset)
    assert data.endswith(EOF_MARK)

    def strip(text):
        for o in options:
            text = text.replace(o, "")
        return text.splitlines()
    assert strip(xs._header_text(data)) == strip(rm.header_sorted(xs._header_text(plain)))
    hd = xs._header_text(data).splitlines()[0].split("\t")
    assert hd[0] == "@HD" and hd.count("SO:coordinate") == 1 and sum(f.startswith("SO:") for f in hd) == 1
    return want, reset


def _hold_index(data, bai):
    n_ref, recs = br.bam_records(data)
    assert len(bm.read_bai(bai)["refs"]) == n_ref and bai == bm.build(n_ref, recs)
    br.check_queries(data, bai, recs, n_ref)


@pytest.mark.parametrize("mode", ["out", "out_u", "fragments", "clip", "clip_fix_mates"])
def test_the_sorted_file_is_the_models_order_of_the_unsorted_one(shuffled, mode):
    bam, d, sam = shuffled
    base = {"out": ["out", "--gpus", "1", "-b"], "out_u": ["out", "--gpus", "1", "-u"], "fragments": ["out", "--gpus", "1", "--fragments", "-u"],
            "clip": ["out", "--gpus", "1", "-c", "-b"], "clip_fix_mates": ["out", "--gpus", "1", "-c", "--fix-mates", "-b"]}[mode]
    src = bam.read_bytes()
    plain = _ok(_run(base + [str(bam)]))
    p = _ok(_run(base + ["--sort", str(bam)]))                               # stdout a pipe
    want, reset = _hold(p.stdout, plain.stdout, src, mode.startswith("clip"), " --sort")
    assert xs._records(p.stdout) != want                                      # (the input was not in coordinate order)
    assert p.stderr.count(STATS_LINE) == 1 and b"windows" not in p.stderr
    said = lambda e: [l for l in _said(e) if "[W::fade-out]" not in l]        # (under -c the warning about the order differs: it is sorted now)
    assert said(p.stderr) == said(plain.stderr)
    if mode.startswith("clip"):
        assert b"[W::fade-out] --sort: the output is written in coordinate order" in p.stderr and b"will not be sorted" not in p.stderr
    with open(d / (mode + ".bam"), "wb") as fo:                               # stdout a file
        _ok(subprocess.run([FADE] + base + ["--sort", str(bam)], stdout=fo, stderr=subprocess.PIPE, timeout=600))
    assert xs._records((d / (mode + ".bam")).read_bytes()) == xs._records(p.stdout)
    # the index of the sorted file, made in the same pass — also under -c without --keep-sorted
    bai = d / (mode + ".bai")
    q = _run(base + ["--sort", "--write-index", str(bai), str(bam)])
    if reset and any(reset):
        # A reset record is written zero-filled (refID 0, pos 0) at the end of the file: by its own bytes that file is not in
        # coordinate order, and no index can be made of it.  The run says so, with the number of such reads, BEFORE a byte is on
        # stdout.  The index itself is then checked on the same input without the reads that reset.
        assert q.returncode == 1 and q.stdout == b"" and not bai.exists(), q.stderr.decode()
        assert (b"[E::fade-out] --sort --write-index: %d reads are clipped to nothing" % sum(reset)) in q.stderr, q.stderr.decode()
        lines = sam.read_text().splitlines()
        head, body = [l for l in lines if l.startswith("@")], [l for l in lines if not l.startswith("@")]
        assert len(body) == len(reset)
        sam2, bam2 = d / (mode + ".noreset.sam"), d / (mode + ".noreset.bam")
        sam2.write_text("\n".join(head + [l for l, r in zip(body, reset) if not r]) + "\n")
        _bam_of(sam2, bam2)
        plain2 = _ok(_run(base + [str(bam2)]))
        q = _ok(_run(base + ["--sort", "--write-index", str(bai), str(bam2)]))
        want2, reset2 = _hold(q.stdout, plain2.stdout, bam2.read_bytes(), True, " --sort --write-index " + str(bai))
        assert not any(reset2) and len(want2) == len(want) - sum(reset)
    else:
        _ok(q)
        assert xs._records(q.stdout) == xs._records(p.stdout)
    _hold_index(q.stdout, bai.read_bytes())


def test_30000_reads_in_one_window_and_in_several(big, tmp_path):  # noqa: F811
    src = big.read_bytes()
    env = {"FADE_BAM_CHUNK_MB": "1", "FADEHIP_RECSTORE_BYTES": "4096"}        # many calls, an arena that grows many times
    for base, clip in ((["out", "--gpus", "1", "--fragments", "-b"], False), (["out", "--gpus", "1", "-c", "-b"], True)):
        plain = _ok(_run(base + [str(big)], env))
        one = _ok(_run(base + ["--sort", "--timing", str(big)], env))
        want, reset = _hold(one.stdout, plain.stdout, src, clip, " --sort", " --timing")
        assert b"in 1 window," in one.stderr and b"windows" not in one.stderr
        lens = _ref_len(src)
        nbytes, nrec = sm.histogram(lens, want, reset)
        total, most = sm.cost(sum(nbytes), sum(nrec)), max(sm.cost(b, n) for b, n in zip(nbytes, nrec))
        budget = max(most, total // 4)
        n_win = len(sm.windows(nbytes, nrec, budget))
        assert n_win >= 3
        bai = tmp_path / ("w%d.bai" % clip)
        extra = [] if (reset and any(reset)) else ["--write-index", str(bai)]     # (reads that reset: the refusal is the golden sets' case above)
        many = _ok(_run(base + ["--sort", "--timing"] + extra + [str(big)], dict(env, FADEHIP_RECSTORE_BUDGET=str(budget))))
        assert xs._records(many.stdout) == xs._records(one.stdout) and many.stdout.endswith(EOF_MARK)
        assert xs._header_text(many.stdout).replace(" --write-index " + str(bai), "") == xs._header_text(one.stdout)
        warn = [l for l in many.stderr.decode().splitlines() if l.startswith("[W::fade-out] --sort: ") and "windows" in l]
        assert len(warn) == 1 and ("written in %d windows" % n_win) in warn[0] and ("budget of %d bytes" % budget) in warn[0], many.stderr.decode()
        assert many.stderr.count(STATS_LINE) == 1 == one.stderr.count(STATS_LINE)
        stats = lambda e: [l for l in _said(e) if not l.startswith("[W::") and not l.startswith("[E::")]
        assert stats(many.stderr) == stats(one.stderr) == stats(plain.stderr)
        if extra:
            _hold_index(many.stdout, bai.read_bytes())
        # a budget below one bucket's cost: refused, the bucket named, nothing of the records on stdout
        p = _run(base + ["--sort", str(big)], dict(env, FADEHIP_RECSTORE_BUDGET=str(most - 1)))
        b = max(range(len(nbytes)), key=lambda k: sm.cost(nbytes[k], nrec[k]))
        assert p.returncode == 1 and p.stdout == b"" and b"[E::fade-out] --sort: " in p.stderr, p.stderr.decode()
        assert (b"%d bytes (%d records)" % (nbytes[b], nrec[b])) in p.stderr and (b"budget of %d bytes" % (most - 1)) in p.stderr, p.stderr.decode()


@pytest.mark.parametrize("clip", [False, True], ids=["annotate", "annotate_clip"])
def test_annotate_sort_on_the_golden_inputs(gold, clip):  # noqa: F811
    d = gold["dir"]
    base = ["annotate", "--timing"] + gold["opts"] + (["-c"] if clip else []) + ["-b"]     # (--timing: the run says which path it took)
    tail = [str(gold["bam"]), gold["fa"]]
    plain = _ok(_run(base + tail))
    bai = d / ("anno%d.bai" % clip)
    p = _run(base + ["--sort", "--write-index", str(bai)] + tail, {"FADEHIP_RECSTORE_BYTES": "4096"})
    want = xs._records(plain.stdout)
    reset = [_is_reset(a, b) for a, b in zip(xs._records(gold["bam"].read_bytes()), want)] if clip else None
    if reset and any(reset):     # (as for fade out: refused before a byte is written; then without the index)
        assert p.returncode == 1 and p.stdout == b"" and not bai.exists(), p.stderr.decode()
        assert (b"[E::fade-annotate] --sort --write-index: %d reads are clipped to nothing" % sum(reset)) in p.stderr, p.stderr.decode()
        p = _ok(_run(base + ["--sort"] + tail))
        _hold(p.stdout, plain.stdout, gold["bam"].read_bytes(), clip, " --sort")
    else:
        _ok(p)
        _hold(p.stdout, plain.stdout, gold["bam"].read_bytes(), clip, " --sort --write-index " + str(bai))
        _hold_index(p.stdout, bai.read_bytes())
    assert b"file path on the device" in p.stderr and p.stderr.count(b"[timing] --sort: ") == 1
    stats = lambda e: [l for l in _said(e) if not l.startswith("[W::")]
    assert stats(p.stderr) == stats(plain.stderr)
    if clip:
        assert b"[W::fade-out] --sort: the output is written in coordinate order" in p.stderr and b"will not be sorted" not in p.stderr
    # over the budget: annotate sorts in one piece, so it fails with nothing on stdout, names the budget and points to fade out
    q = _run(base + ["--sort"] + tail, {"FADEHIP_RECSTORE_BUDGET": "3000"})
    assert q.returncode == 1 and q.stdout == b"", q.stderr.decode()
    assert b"[E::fade-annotate] --sort: " in q.stderr and b"budget of 3000 bytes" in q.stderr and b"fade out --gpus 1 --sort" in q.stderr, q.stderr.decode()


def test_without_the_option_the_device_path_writes_what_the_host_loops_write(gold):  # noqa: F811
    """`fade out -c -b` and `fade annotate -b` without --sort: the driver code this change moved (the totals read earlier, the
    sorted writer in three steps) lies on the device path; the host loops are untouched, and the two agree record for record,
    header for header (but @PG), message for message."""
    def payload(out):
        raw = gzip.decompress(out)
        n = int.from_bytes(raw[4:8], "little")
        return [l for l in raw[8:8 + n].decode().splitlines() if not l.startswith("@PG")], raw[8 + n:]
    dev = _ok(_run(["out", "-c", "-b", "--gpus", "1", "--timing", str(gold["anno"])]))
    host = _ok(_run(["out", "-c", "-b", str(gold["anno"])]))
    assert b"file path on the device" in dev.stderr and b"file path on the device" not in host.stderr
    assert payload(dev.stdout) == payload(host.stdout) and _said(dev.stderr) == _said(host.stderr) and dev.stdout.endswith(EOF_MARK)
    tail = gold["opts"] + ["-b", str(gold["bam"]), gold["fa"]]
    dev = _ok(_run(["annotate", "--timing"] + tail))
    host = _ok(_run(["annotate"] + tail, {"FADE_BAM_DEVICE": "0"}))
    assert b"file path on the device" in dev.stderr and b"file path on the device" not in host.stderr
    assert payload(dev.stdout) == payload(host.stdout) and _said(dev.stderr) == _said(host.stderr) and dev.stdout.endswith(EOF_MARK)
