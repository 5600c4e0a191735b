"""`fade annotate --clip` without a GPU: the option is parsed and refused where it must be, and the host's clip_read
(driven by `fade out -c` on SAM text) agrees with oracle/pyfilter.clip_read on the constructed cases that the device
function is held to in tests/test_gpu_clip_batch.py."""
import os
import re
import subprocess

import pytest

import clip_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fade_bin():
    import __graft_entry__ as ge
    ge.build()
    return FADE


def _run(args):
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_the_cases_cover_what_the_clip_has_to_handle():
    kinds = set()
    for c in cc.cases():
        new, _ = cc.expected(c)
        reset = bool(c["rs"] & 6) and new["tags"] == {}
        kinds.add((c["rs"] & 6, reset))
        if c["rs"] & 6 and not reset:
            if c["rs"] & 2:
                kinds.add(("left_parity", int(re.match(r"(\d+)H", new["cigar"]).group(1)) % 2))
            kinds.add(("rest_parity", len(new["seq"]) % 2))
    for want in [(2, False), (4, False), (6, False), (2, True), (4, True), (6, True), (0, False), ("left_parity", 0), ("left_parity", 1),
                 ("rest_parity", 0), ("rest_parity", 1)]:
        assert want in kinds, want
    lens = {len(c["rec"]["seq"]) for c in cc.cases()}
    assert {1, 2} <= lens and max(lens) > 512
    assert any(len(c["aux"]) > 3000 for c in cc.cases()) and any(not c["aux"] for c in cc.cases())


def test_annotate_accepts_clip_and_shows_it_in_the_help(fade_bin):
    for flag in ("-c", "--clip", "-bc"):
        p = _run(["annotate", flag])
        assert p.returncode == 0 and b"Unrecognized option" not in p.stderr, p.stderr.decode()
        assert b"-c        --clip" in p.stderr
    p = _run(["extract", "-c", "x.sam"])
    assert p.returncode == 1 and b"Unrecognized option" in p.stderr


@pytest.mark.parametrize("flag", ["--stats-tsv", "--clip-tsv"])
def test_reports_are_refused_with_clip(fade_bin, tmp_path, flag):
    sam, fa = os.path.join(GOLD, "anno_c1.sam"), os.path.join(GOLD, "anno_c1.fa")
    out = str(tmp_path / "x.tsv")
    for args in (["annotate", "-c", flag, out, sam, fa], ["annotate", "%s=%s" % (flag, out), "--clip", "-b", sam, fa]):
        p = _run(args)
        assert p.returncode == 1
        assert b"Unrecognized option" not in p.stderr
        assert (flag + " describes unclipped records: not with --clip").encode() in p.stderr
        assert not p.stdout and not os.path.exists(out)


def test_host_clip_read_agrees_with_pyfilter_on_the_constructed_cases(fade_bin, tmp_path):
    from oracle import pyfilter
    cases = cc.cases(sam_only=True)
    recs = [c["rec"] for c in cases]
    head = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:1000000\n" % n for n in cc.CONTIGS)
    src = tmp_path / "cases.sam"
    src.write_text(head + "".join(pyfilter._fmt(r) + "\n" for r in recs))
    p = _run(["out", "-c", str(src)])
    assert p.returncode == 0, p.stderr.decode()
    lines = [l for l in p.stdout.decode().splitlines() if not l.startswith("@")]
    exp, _ = pyfilter.fade_out(recs, cc.CONTIGS[0], clip=True)
    assert len(lines) == len(exp) == len(cases)
    bad = [(c["name"], a, b) for c, a, b in zip(cases, lines, exp) if a != b]
    assert not bad, bad[:5]
    # and the BAM writer lays the clipped records out as tests/clip_cases.build_rec does (what the device is compared with)
    import gzip
    pb = _run(["out", "-c", "-b", str(src)])
    assert pb.returncode == 0, pb.stderr.decode()
    raw = gzip.decompress(pb.stdout)
    at = 8 + int.from_bytes(raw[4:8], "little")
    n_ref = int.from_bytes(raw[at:at + 4], "little")
    at += 4
    for _ in range(n_ref):
        at += 4 + int.from_bytes(raw[at:at + 4], "little") + 4
    for c in cases:
        bs = int.from_bytes(raw[at:at + 4], "little")
        got = raw[at:at + 4 + bs]
        at += 4 + bs
        new = pyfilter.clip_read(c["rec"], c["rs"], cc.CONTIGS[0]) if c["rs"] & 6 else c["rec"]
        aux = b"" if new["tags"] == {} else b"rsC" + bytes([c["rs"]]) + b"amZ" + c["rec"]["tags"]["am"][1].encode() + b"\0"
        assert got == cc.to_bam(new, aux), c["name"]
    assert at == len(raw)


def _sam_line(rec):
    """pyfilter's line as SAM writes it: a record without bases has `*` for them and for the qualities."""
    from oracle import pyfilter
    f = pyfilter._fmt(rec).split("\t")
    if f[9] == "":
        f[9] = f[10] = "*"
    return "\t".join(f)


@pytest.mark.parametrize("family", ["writer", "bins", "random"])
def test_host_clip_read_agrees_with_pyfilter_on_the_sweep(fade_bin, tmp_path, family):
    """tests/clip_sweep.py's generated records through `fade out -c` as SAM text and through `fade out -c -b` as bytes.  The
    SAM reader does not hold l_seq to the CIGAR, so the records with fewer bases than their CIGAR claims go through as well,
    and so do the unmapped records that carry a CIGAR."""
    import gzip
    import clip_sweep as sw
    cases, exp = sw.cases(family, sam_only=True), sw.expected(family)
    head = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, sw.LN) for n in cc.CONTIGS)
    src = tmp_path / "sweep.sam"
    src.write_text(head + "".join(_sam_line(c["rec"]) + "\n" for c in cases))
    p = _run(["out", "-c", str(src)])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if not l.startswith("@")]
    assert len(lines) == len(cases)
    bad = [(c["name"], a, _sam_line(new)) for c, a, (new, _) in zip(cases, lines, exp) if a != _sam_line(new)]
    assert not bad, (len(bad), bad[:5])
    pb = _run(["out", "-c", "-b", str(src)])
    assert pb.returncode == 0, pb.stderr.decode()[-2000:]
    raw = gzip.decompress(pb.stdout)
    at = 8 + int.from_bytes(raw[4:8], "little")
    n_ref = int.from_bytes(raw[at:at + 4], "little")
    at += 4
    for _ in range(n_ref):
        at += 4 + int.from_bytes(raw[at:at + 4], "little") + 4
    bad = []
    for c, (new, _) in zip(cases, exp):
        bs = int.from_bytes(raw[at:at + 4], "little")
        got = raw[at:at + 4 + bs]
        at += 4 + bs
        aux = b"" if sw.is_reset(c, new) else b"rsC" + bytes([c["rs"]]) + b"amZ" + c["rec"]["tags"]["am"][1].encode() + b"\0"
        want = cc.to_bam(new, aux)
        if got != want:
            d, w = cc.decode_rec(got), cc.decode_rec(want)
            bad.append((c["name"],) + next(((k, d[k], w[k]) for k in w if d[k] != w[k]), ("bytes", got[:48].hex(), want[:48].hex())))
    assert not bad, (len(bad), bad[:5])
    assert at == len(raw)
