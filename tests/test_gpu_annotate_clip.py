"""`fade annotate --clip`: the artifact calls hard-clipped in the pass that writes the tags (FADEHIP_BAM_CLIP on the file
path, the host's clip_read in the host pipeline).  For every record the expectation is
oracle/pyfilter.clip_read(record + the oracle's tags); every output format and path must decode to it, in input order, and
to what the two-step pipeline (`annotate -b` to a file, then `out -c -b`) makes."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import samutil

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")
W1 = b"[W::fade-out] Using the -c flag means the output SAM/BAM will not be sorted (regardless of prior sorting)"
W2 = b"[W::fade-out] You also may need to fix mate information with a tool like Picard FixMateInformation"
STATS = ("read count", "Clipped", "% With", "Artifact")


def _run(args, env=None, **kw):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=e, **kw)


def _ok(p):
    assert p.returncode == 0, p.stderr.decode()[-2500:]
    return p


def _bam_of(sam, path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "sam2bam"])
    with open(path, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), str(sam)], stdout=fo)


def _norm(r, names=None):
    """One form for records from SAM text (parse_sam, pyfilter) and from BAM (bam_to_sam_records)."""
    if "mtid" in r:
        mate = names[r["mtid"]] if r["mtid"] >= 0 else "*"
        pnext = r["mpos"] + 1
    else:
        mate = r["rname"] if r["rnext"] == "=" else r["rnext"]
        pnext = r["pnext"]
    seq = r["seq"] or "*"
    tags = [(k,) + tuple(r["tags"][k]) for k in r["tag_order"]]
    return (r["qname"], r["flag"], r["rname"], r["pos"], r["mapq"], r["cigar"], mate, pnext, r["tlen"], seq, r["qual"] if seq != "*" else "*", tags)


def _decode(out, fmt):
    """(header lines without @PG, normalised records) of a run's stdout."""
    if fmt == "sam":
        header, recs = samutil.parse_sam(out.decode())
        return [h for h in header if not h.startswith("@PG")], [_norm(r) for r in recs]
    text, names, recs = samutil.bam_to_sam_records(out)
    return [h for h in text.splitlines() if not h.startswith("@PG")], [_norm(r, names) for r in recs]


def _pg(out, fmt):
    text = out.decode() if fmt == "sam" else samutil.bam_to_sam_records(out)[0]
    return [h for h in text.splitlines() if h.startswith("@PG")]


def _expect(in_recs, ann, contig0):
    """ann[i] = (rs, am, as, ar, ab) with am '' / None when the record has no artifact strings."""
    from oracle import pyfilter
    out, n_left, n_right, n_reset = [], 0, 0, 0
    for r, (rs, am, as_, ar, ab) in zip(in_recs, ann):
        r = dict(r, tags=dict(r["tags"]), tag_order=list(r["tag_order"]))
        new = [("rs", ("i", str(rs)))] + ([("am", ("Z", am)), ("as", ("Z", as_)), ("ar", ("Z", ar)), ("ab", ("Z", ab))] if am else [])
        for k, v in new:
            assert k not in r["tags"]
            r["tags"][k] = v
            r["tag_order"].append(k)
        if rs & 6:
            c = pyfilter.clip_read(r, rs, contig0)
            n_left += bool(rs & 2)
            n_right += bool(rs & 4)
            n_reset += c["tags"] == {}
            r = c
        out.append(_norm(r))
    return out, (n_left, n_right, n_reset)


def _all_paths(bam, sam, fa, opts, exp, tmp_path, min_counts=None):
    """Every format and path of `annotate -c` on one input against exp, and against the two-step pipeline."""
    base = ["annotate", "--stats", "--timing"] + opts
    runs = {
        "dev_inflate": (_run(base + ["-c", "-b", str(bam), str(fa)], {"FADE_BAM_INFLATE": "device"}), "bam"),
        "host_inflate": (_run(base + ["-c", "-b", str(bam), str(fa)], {"FADE_BAM_INFLATE": "host"}), "bam"),
        "ubam": (_run(base + ["-c", "-u", str(bam), str(fa)]), "bam"),
        "sam": (_run(base + ["--clip", str(bam), str(fa)]), "sam"),
        "sam_in_sam_out": (_run(base + ["-c", str(sam), str(fa)]), "sam"),
        "host_pipeline_bam": (_run(base + ["-c", "-b", str(bam), str(fa)], {"FADE_BAM_DEVICE": "0"}), "bam"),
    }
    plain = _ok(_run(base + ["-b", str(bam), str(fa)]))
    stats = lambda err: [l for l in err.decode().splitlines() if l.startswith(STATS)]
    assert len(stats(plain.stderr)) == 7
    heads = []
    for name, (p, fmt) in runs.items():
        _ok(p)
        if name in ("dev_inflate", "host_inflate", "ubam"):
            assert b"file path on the device" in p.stderr, name
        else:
            assert b"file path on the device" not in p.stderr, name
        head, recs = _decode(p.stdout, fmt)
        heads.append(head)
        assert len(recs) == len(exp), name
        bad = [(name, k, a, b) for k, (a, b) in enumerate(zip(recs, exp)) if a != b]
        assert not bad, bad[:3]
        assert p.stderr.count(W1) == 1 and p.stderr.count(W2) == 1, name
        pg = _pg(p.stdout, fmt)
        mine = [h for h in pg if "ID:fade-annotate" in h]
        assert len(mine) == 1 and (" -c " in mine[0] or " --clip " in mine[0]) and not any("fade-extract" in h for h in pg), pg
        assert stats(p.stderr) == stats(plain.stderr), name  # the counters do not know about the flag
    assert all(h == heads[0] for h in heads)
    # the three device runs write the same record bytes
    body = lambda out: gzip.decompress(out)[8 + int.from_bytes(gzip.decompress(out)[4:8], "little"):]
    assert body(runs["dev_inflate"][0].stdout) == body(runs["host_inflate"][0].stdout) == body(runs["ubam"][0].stdout) == body(runs["host_pipeline_bam"][0].stdout)
    # the two-step product pipeline
    anno = tmp_path / "two_step_anno.bam"
    anno.write_bytes(plain.stdout)
    assert W1 not in plain.stderr
    two = _ok(_run(["out", "-c", "-b", str(anno)]))
    head2, recs2 = _decode(two.stdout, "bam")
    assert head2 == heads[0] and recs2 == exp


def _golden_input(tag):
    from test_gpu_cli import _expected
    gold, floor_len, window = _expected(tag)
    header, recs = samutil.parse_sam(open(os.path.join(GOLD, tag + ".sam")).read())
    contig0 = [h for h in header if h.startswith("@SQ")][0].split("\t")[1][3:]
    assert [(r["qname"], r["flag"]) for r in recs] == [(g[0], g[1]) for g in gold]
    return recs, [g[2:] for g in gold], contig0, floor_len, window


@pytest.mark.parametrize("tag", ["anno_c1", "anno_c2", "anno_c5", "anno_floor0"])
def test_clip_on_the_golden_inputs_every_format_and_path(tmp_path, tag):
    recs, ann, contig0, floor_len, window = _golden_input(tag)
    exp, (n_left, n_right, n_reset) = _expect(recs, ann, contig0)
    assert n_left + n_right >= 6
    bam = tmp_path / "in.bam"
    sam = os.path.join(GOLD, tag + ".sam")
    _bam_of(sam, bam)
    _all_paths(bam, sam, os.path.join(GOLD, tag + ".fa"), ["--min-length", str(floor_len), "-w", str(window)], exp, tmp_path)


@pytest.mark.parametrize("seed,floor_len,window", [(11, 5, 100), (12, 0, 40), (13, 7, 300)])
def test_clip_on_random_reads_against_the_oracle_every_format_and_path(tmp_path, oracle, seed, floor_len, window):
    """The random batches of test_gpu_bam_stream's oracle test (IUPAC reads, every CIGAR op, a soft-masked FASTA): a third of
    the records are artifact calls, and a good part of those reset.  By the oracle and pyfilter, seeds 11 / 12 / 13 hold
    290 / 236 / 294 left clips, 301 / 254 / 287 right clips and 87 / 84 / 96 resets (counted over records; printed below)."""
    from test_gpu_fuzz import _random_batch
    rng = np.random.default_rng(seed)
    contigs = []
    for k in range(3):
        c = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(rng.integers(4000, 9000)))].tobytes())
        for q in rng.integers(0, len(c), size=len(c) // 40):
            c[q] = int(rng.choice(list(b"NNNRYKMacgtn")))
        a = int(rng.integers(0, len(c) - 300))
        c[a:a + 200] = bytes(c[a:a + 200]).lower()
        contigs.append(bytes(c).decode())
    names = ["ctgA", "ctgB", "ctgC"]
    b = _random_batch(rng, contigs, 2500, window)
    qn = ["q%d" % i for i in range(len(b["pos"]))]
    b["qname"] = [x.encode() for x in qn]
    sam, fa, bam = tmp_path / "in.sam", tmp_path / "ref.fa", tmp_path / "in.bam"
    sam.write_text(samutil.batch_to_sam(b, names, [len(c) for c in contigs], qn))
    fa.write_text("".join(">%s\n%s\n" % (n, "\n".join(c[o:o + 70] for o in range(0, len(c), 70))) for n, c in zip(names, contigs)))
    _bam_of(sam, bam)
    G = oracle.GenomeHolder(names, contigs)
    reads, keep = oracle.make_reads(b)
    want = [oracle.annotate_one(G, reads[i], floor_len, window) for i in range(len(qn))]
    ann = [(w["rs"], w["am"], w["as_"], w["ar"], w["ab"]) if w["has_tags"] else (w["rs"], None, None, None, None) for w in want]
    _, in_recs = samutil.parse_sam(sam.read_text())
    exp, (n_left, n_right, n_reset) = _expect(in_recs, ann, names[0])
    print("seed %d: %d left clips, %d right clips, %d resets (oracle)" % (seed, n_left, n_right, n_reset))
    assert n_left >= 100 and n_right >= 100 and n_reset >= 50, (n_left, n_right, n_reset)  # a generator change must not empty the test
    _all_paths(bam, sam, fa, ["--min-length", str(floor_len), "-w", str(window)], exp, tmp_path)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """30,000 reads of C5 (30 % soft-clipped) as a BAM of ~130 BGZF members; `annotate -c -b` by the host pipeline and by one
    lane on the device."""
    from fade_amd import synth
    d = tmp_path_factory.mktemp("clipbig")
    cfg, g, b = synth.make_config("C5", 30000, contig_len=400_000)
    names = ["read%d" % (i // 2) for i in range(len(b["pos"]))]
    b["qname"] = names
    sam, fa, bam = d / "in.sam", d / "ref.fa", d / "in.bam"
    sam.write_text(samutil.batch_to_sam(b, g.names, [int(x) for x in g.lengths], names))
    fa.write_bytes(g.fasta_bytes())
    bam.write_bytes(_ok(_run(["out", "-b", str(sam)])).stdout)
    base = ["annotate", "--stats", "--timing", "-w", "100"]
    host = _ok(_run(base + ["-c", "-b", str(bam), str(fa)], {"FADE_BAM_DEVICE": "0"}))
    one = _ok(_run(base + ["-c", "-b", str(bam), str(fa)]))
    assert b"file path on the device" in one.stderr and b"file path on the device" not in host.stderr
    return dict(dir=d, bam=bam, fa=fa, base=base, host=host, one=one)


def _split(out):
    raw = gzip.decompress(out)
    l_text = int.from_bytes(raw[4:8], "little")
    return [l for l in raw[8:8 + l_text].decode().splitlines() if not l.startswith("@PG")], raw[8 + l_text:]


def test_clip_on_30000_reads_equals_the_host_pipeline_and_the_two_step_pipeline(big):
    assert _split(big["one"].stdout) == _split(big["host"].stdout)
    plain = _ok(_run(big["base"] + ["-b", str(big["bam"]), str(big["fa"])]))
    anno = big["dir"] / "anno.bam"
    anno.write_bytes(plain.stdout)
    two = _ok(_run(["out", "-c", "-b", str(anno)]))
    assert _split(two.stdout) == _split(big["one"].stdout)
    _, _, recs = samutil.bam_to_sam_records(big["one"].stdout)
    n_art = sum(1 for r in recs if "rs" in r["tags"] and int(r["tags"]["rs"][1]) & 6)
    n_h = sum(1 for r in recs if "H" in r["cigar"])
    assert n_h >= n_art > 1000 and len(recs) == 30000  # (a reset record carries no rs)


@pytest.mark.parametrize("inflate", ["device", "host"])
def test_clip_with_records_cut_by_members_and_calls(big, inflate):
    p = _ok(_run(big["base"] + ["-c", "-b", str(big["bam"]), str(big["fa"])], {"FADE_BAM_CHUNK_MB": "1", "FADE_BAM_INFLATE": inflate}))
    assert b"file path on the device" in p.stderr
    assert _split(p.stdout) == _split(big["one"].stdout)


def test_clip_travels_to_the_lanes_and_the_shards(big):
    env = {"FADE_DEVICE_MAP": "0,0"}
    two = _ok(_run(big["base"] + ["-c", "-b", "--gpus", "2", str(big["bam"]), str(big["fa"])], env))
    assert b"lane 1 of 2" in two.stderr and two.stderr.count(W1) == 1 and two.stderr.count(W2) == 1
    assert _split(two.stdout) == _split(big["one"].stdout)
    stats = lambda err: [l for l in err.decode().split("read count:")[1].splitlines() if not l.startswith("[timing]") and l][:7]
    assert stats(two.stderr) == stats(big["one"].stderr)
    prefix = str(big["dir"] / "shard")
    sh = _ok(_run(big["base"] + ["--clip", "-b", "--gpus", "2", "--out-shards", prefix, str(big["bam"]), str(big["fa"])], env))
    assert sh.stdout == b"" and sh.stderr.count(W1) == 1
    head, body = _split(big["one"].stdout)
    got = b""
    for k in range(2):
        h, b = _split(open("%s.%d.bam" % (prefix, k), "rb").read())
        assert h == head
        at = 4
        for _ in range(int.from_bytes(b[:4], "little")):
            at += 4 + int.from_bytes(b[at:at + 4], "little") + 4
        got += b[:at] * (k == 0) + b[at:]
    assert got == body


def test_clip_goes_by_the_computed_result_not_by_tags_the_record_brought(tmp_path):
    """A record that comes in with rs:Z or am:i keeps that tag (htslib's EINVAL) — and is clipped by what this run computed,
    where `fade out -c` behind `fade annotate` would read the stale tag."""
    tag = "anno_c5"
    recs, ann, contig0, floor_len, window = _golden_input(tag)
    arts = [k for k, a in enumerate(ann) if a[0] & 6]
    k_rs, k_am = arts[0], arts[1]
    lines = open(os.path.join(GOLD, tag + ".sam")).read().splitlines()
    body0 = next(i for i, l in enumerate(lines) if not l.startswith("@"))
    lines[body0 + k_rs] += "\trs:Z:stale"
    lines[body0 + k_am] += "\tam:i:5"
    sam, bam = tmp_path / "in.sam", tmp_path / "in.bam"
    sam.write_text("\n".join(lines) + "\n")
    _bam_of(sam, bam)
    exp, _ = _expect(recs, ann, contig0)
    fa = os.path.join(GOLD, tag + ".fa")
    opts = ["annotate", "--timing", "--min-length", str(floor_len), "-w", str(window), "-c"]
    dev = _ok(_run(opts + ["-b", str(bam), fa]))
    host = _ok(_run(opts + ["-b", str(bam), fa], {"FADE_BAM_DEVICE": "0"}))
    assert b"file path on the device" in dev.stderr
    assert _split(dev.stdout) == _split(host.stdout)
    samout = _ok(_run(opts + [str(sam), fa]))
    for out, fmt in ((dev.stdout, "bam"), (samout.stdout, "sam")):
        _, got = _decode(out, fmt)
        assert len(got) == len(exp)
        for k, (g, e) in enumerate(zip(got, exp)):
            if k not in (k_rs, k_am):
                assert g == e, k
        for k in (k_rs, k_am):
            assert got[k][:11] == exp[k][:11], (k, got[k][:11], exp[k][:11])  # clipped by the computed alignment
            assert "H" in got[k][5] or got[k][5] == "*"
        t_rs, t_am = dict((t[0], t[1:]) for t in got[k_rs][11]), dict((t[0], t[1:]) for t in got[k_am][11])
        e_rs, e_am = dict((t[0], t[1:]) for t in exp[k_rs][11]), dict((t[0], t[1:]) for t in exp[k_am][11])
        if e_rs:  # (a reset record has no tags at all)
            assert t_rs["rs"] == ("Z", "stale") and all(t_rs[x] == e_rs[x] for x in ("am", "as", "ar", "ab"))
        if e_am:
            assert t_am["am"] == ("i", "5") and t_am["rs"] == e_am["rs"] and all(t_am[x] == e_am[x] for x in ("as", "ar", "ab"))
        assert e_rs or e_am


def test_clip_refusals():
    sam, fa = os.path.join(GOLD, "anno_c1.sam"), os.path.join(GOLD, "anno_c1.fa")
    for flag in ("--stats-tsv", "--clip-tsv"):
        p = _run(["annotate", "-c", "-b", flag, "/dev/null", sam, fa])
        assert p.returncode == 1 and (flag + " describes unclipped records").encode() in p.stderr and not p.stdout
    p = _run(["annotate", "-c", "-b", "-u", sam, fa])
    assert p.returncode == 1 and b"only one of the b or u flags" in p.stderr
