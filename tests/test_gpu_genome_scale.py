"""annotate on a genome past 2^32 bases (tests/genome_scale.py: 18 contigs of chr1's length, one of 120 Mbp wholly above base
2^32, 3,000 short contigs behind it, ~4.6 Gbp, 2.3 GB packed), every record held to the oracle (rs, am / as / ar / ab).
Reads are planted on windows that straddle base 2^31 and base 2^32, at both ends of the contig above 2^32, at the first
base of the genome, at the last bases of the packed buffer and on a late contig with a long name; their true windows hold
other bases than a truncated offset would read, so a wrapped offset shows up as a wrong tag.  Paths: level 2 on every
score-kernel family, hinted and not, a window beyond 32,000 columns, the thread-per-alignment long kernel, pass-2
re-traces (span slack 0), no forced-diagonal shortcut, the single-pass kernels, the file path on the device with all
3,059 @SQ entries, and the CLI on a FASTA of the short contigs.  Each context uploads the whole genome; one is open at a
time."""
import gzip
import os
import struct
import subprocess
import types

import numpy as np
import pytest

import fade_amd
import genome_scale as GS
import samutil
from fade_amd import format_tags

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")

# read lengths on every score-kernel family: eight-lane (36 .. 150), sixteen-lane classes (200 .. 512), one wave per
# alignment (700 .. 4096), thread per alignment (> 4096)
EIGHT_LANE = (36, 50, 76, 100, 150)
SIXTEEN_LANE = (200, 251, 400, 512)
WAVE_LONG = (700, 2000, 4096)
THREAD_LONG = (5000,)


@pytest.fixture(scope="module")
def scale(oracle):
    G = GS.ScaleGenome()
    H = oracle.GenomeHolder(G.names, G.seqs)
    cache = {}

    def expect(L, W):
        """(batch, site of each record, oracle rs, {record: (am, as, ar, ab)}) for reads of L bases and window W."""
        if (L, W) not in cache:
            b, labels = GS.site_batch(G, L, W, GS.n_per_site(L))
            ors, _ = oracle.annotate_batch_soa(H, b, 5, W, threads=16, want_am=False)
            reads, keep = oracle.make_reads(b)
            tags = {}
            for i in np.nonzero((ors >> 1) & 3)[0]:
                a = oracle.annotate_one(H, reads[int(i)], 5, W)
                tags[int(i)] = (a["am"], a["as_"], a["ar"], a["ab"])
            assert len(tags) >= 0.15 * len(ors), (L, W, len(tags), len(ors))
            for site in ("straddle_2p31", "straddle_2p32", "big_high_start", "big_high_end"):
                assert any(labels[i] == site for i in tags), (L, W, site)
            cache[(L, W)] = (b, labels, ors, tags)
        return cache[(L, W)]

    return types.SimpleNamespace(G=G, H=H, expect=expect)


def _check(scale, L, W, rs, aln, what):
    b, labels, ors, otags = scale.expect(L, W)
    bad = np.nonzero(rs != ors)[0]
    assert len(bad) == 0, (what, L, W, [(int(i), labels[i], int(rs[i]), int(ors[i])) for i in bad[:8]])
    tags = format_tags(b, scale.G.names, rs, aln)
    assert set(tags) == set(otags), (what, L, W, sorted(set(tags) ^ set(otags))[:8])
    for i, t in tags.items():
        assert (t["am"], t["as_"], t["ar"], t["ab"]) == otags[i], (what, L, W, i, labels[i], t["am"], otags[i][0])


def _annotate_both_ways(ctx, scale, L, W, what):
    """The batch as it is (upload walks the records) and with the caller's ABI-3 bounds (the gate trusts nothing)."""
    b = scale.expect(L, W)[0]
    rs, aln, _ = ctx.annotate(b, 5, W)
    _check(scale, L, W, rs, aln, what)
    hb = ctx.with_bounds(b)
    rs, aln, _ = ctx.annotate(hb, 5, W, slot=1)
    _check(scale, L, W, rs, aln, what + " hinted")


def _context(monkeypatch, scale, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = fade_amd.Context(device=0)
    for k in env:
        monkeypatch.delenv(k)
    ctx.genome_upload(scale.G.names, scale.G.seqs)
    return ctx


def test_level2_on_every_score_kernel_family(scale, monkeypatch):
    ctx = _context(monkeypatch, scale)
    try:
        for L in EIGHT_LANE + SIXTEEN_LANE + WAVE_LONG + THREAD_LONG:
            _annotate_both_ways(ctx, scale, L, 100, "default")
        for L in (251, 700):
            _annotate_both_ways(ctx, scale, L, 300, "default")
        _annotate_both_ways(ctx, scale, 150, 17000, "window beyond 32,000 columns")
        monkeypatch.setenv("FADEHIP_LONG_THREAD", "1")  # read per run
        for L in WAVE_LONG:
            _annotate_both_ways(ctx, scale, L, 100, "long thread")
        monkeypatch.delenv("FADEHIP_LONG_THREAD")
        monkeypatch.setenv("FADEHIP_NO_SHORTCUT", "1")  # read per run
        for L in (50, 150, 251, 700):
            _annotate_both_ways(ctx, scale, L, 100, "no shortcut")
        monkeypatch.delenv("FADEHIP_NO_SHORTCUT")
    finally:
        ctx.close()


@pytest.mark.parametrize("env", [dict(FADEHIP_SPAN_SLACK="0"), dict(FADEHIP_KERNEL="pk"), dict(FADEHIP_KERNEL="int32")],
                         ids=["span_slack0", "single_pass_pk", "single_pass_int32"])
def test_level2_on_the_other_paths(scale, monkeypatch, env):
    """Pass-2 re-traces (no slack on the span the score pass leaves), and the single-pass kernels."""
    ctx = _context(monkeypatch, scale, **env)
    try:
        for L in (50, 150, 251, 512, 700):
            _annotate_both_ways(ctx, scale, L, 100, str(env))
        if "FADEHIP_SPAN_SLACK" in env:
            monkeypatch.setenv("FADEHIP_NO_SHORTCUT", "1")
            _annotate_both_ways(ctx, scale, 150, 100, "span slack 0, no shortcut")
            monkeypatch.delenv("FADEHIP_NO_SHORTCUT")
    finally:
        ctx.close()


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)


def _bam(tmp_path, b, names, lengths, qn):
    sam, bam = tmp_path / "in.sam", tmp_path / "in.bam"
    sam.write_text(samutil.batch_to_sam(b, names, [int(x) for x in lengths], qn))
    p = _run(["out", "-b", str(sam)])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    bam.write_bytes(p.stdout)
    return bam


def _members(buf):
    out, at = [], 0
    while at < len(buf):
        bsize = struct.unpack_from("<H", buf, at + 16)[0] + 1
        out.append(buf[at:at + bsize])
        at += bsize
    return out


def _check_records(recs, qn, ors, otags):
    assert [r["qname"] for r in recs] == qn
    for i, r in enumerate(recs):
        t = r["tags"]
        assert int(t["rs"][1]) == int(ors[i]), (r["qname"], t["rs"], int(ors[i]))
        if i in otags:
            assert (t["am"][1], t["as"][1], t["ar"][1], t["ab"][1]) == otags[i], r["qname"]
        else:
            assert "am" not in t


def test_file_path_on_the_device_with_every_contig_in_the_header(scale, monkeypatch, tmp_path):
    """fadehip_bam_*: a BAM whose header lists all 3,059 contigs, records at every site, against the oracle."""
    G = scale.G
    b, labels, ors, otags = scale.expect(150, 100)
    qn = ["q%d_%s" % (i, labels[i]) for i in range(len(labels))]
    raw = _bam(tmp_path, b, G.names, G.lengths, qn).read_bytes()
    payload = gzip.decompress(raw)
    l_text = struct.unpack_from("<i", payload, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", payload, at)[0]
    assert n_ref == len(G.names)
    at += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", payload, at)[0]
        names.append(payload[at + 4:at + 4 + ln - 1].decode())
        at += 4 + ln + 4
    assert names == G.names
    ms = _members(raw)
    cum, k = 0, 0
    while cum + struct.unpack_from("<I", ms[k], len(ms[k]) - 4)[0] <= at:
        cum += struct.unpack_from("<I", ms[k], len(ms[k]) - 4)[0]
        k += 1
    ctx = _context(monkeypatch, scale)
    try:
        st = ctx.bam_stream(names, floor_len=5, window=100, first_record=at - cum)
        st.front(b"".join(ms[k:]), last=True)
        out = st.back()
        totals, n_rec, n_over = st.totals()
        st.close()
    finally:
        ctx.close()
    assert n_rec == len(qn) and n_over == 0
    got = gzip.compress(payload[:at] + gzip.decompress(out))
    _check_records(samutil.bam_to_sam_records(got)[2], qn, ors, otags)


def test_cli_on_a_fasta_of_the_short_contigs(scale, oracle, tmp_path):
    """`fade annotate` on a FASTA of the 3,040 short contigs (the header names them all): reads on the first contig, on the
    last one (the end of the packed buffer) and on late contigs with long names, held to the oracle."""
    G = scale.G
    keep = list(range(GS.N_HEAD)) + list(range(G.big_hi + 1, len(G.names)))
    sub = {c: k for k, c in enumerate(keep)}
    names, seqs = [G.names[c] for c in keep], [G.seqs[c] for c in keep]
    late = [c for c in keep[GS.N_HEAD:] if len(G.names[c]) >= 200 and G.lengths[c] >= 1500][-12:]
    parts = []
    for j, c in enumerate([0, G.last, GS.LATE_LONG] + late):
        L = int(G.lengths[c])
        bj = GS.site_reads(G, (c, L // 2, L // 2, None), 40, 500 + j, 150, 100)
        bj["tid"] = np.where(bj["tid"] >= 0, sub[c], -1).astype(np.int32)
        parts.append(bj)
    from fade_amd import synth
    b = synth.concat(parts)
    assert max(int(t) for t in b["tid"]) == len(keep) - 1 and len(keep) > 3000
    qn = ["r%d" % i for i in range(len(b["pos"]))]
    bam = _bam(tmp_path, b, names, [len(s) for s in seqs], qn)
    fa = tmp_path / "ref.fa"
    with open(fa, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n")
            t = s.tobytes()
            f.write(b"\n".join(t[o:o + 60] for o in range(0, len(t), 60)) + b"\n")
    H = oracle.GenomeHolder(names, seqs)
    ors, _ = oracle.annotate_batch_soa(H, b, 5, 100, threads=16, want_am=False)
    reads, keep_alive = oracle.make_reads(b)
    otags = {}
    for i in np.nonzero((ors >> 1) & 3)[0]:
        a = oracle.annotate_one(H, reads[int(i)], 5, 100)
        otags[int(i)] = (a["am"], a["as_"], a["ar"], a["ab"])
    assert len(otags) >= 40 and any(int(b["tid"][i]) == sub[GS.LATE_LONG] for i in otags)
    p = _run(["annotate", "--min-length", "5", "-w", "100", "-b", str(bam), str(fa)])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _check_records(samutil.bam_to_sam_records(p.stdout)[2], qn, ors, otags)
