"""`fade annotate --eject`: the artifact calls — and, on name-sorted input, every record that shares their name — dropped in
the pass that writes the tags (FADEHIP_BAM_EJECT / FADEHIP_BAM_EJECT_GROUPS on the file path, the writer stage's Ejector in
the host pipeline).  The expectation is oracle/pyfilter.fade_out(records + the oracle's tags, clip=False); every output
format and path must decode to it, in input order, and to what the two-step pipeline (`annotate -b`, then `out -b`) makes."""
import functools
import gzip
import os
import struct

import numpy as np
import pytest

import fade_amd
import samutil
from test_gpu_annotate_clip import GOLD, STATS, _bam_of, _decode, _golden_input, _norm, _ok, _pg, _run, _split

pytestmark = pytest.mark.gpu

W_GROUPS = b"[W::fade-out] Output looks name-sorted, ejecting all reads with same readname if any have an artifact"
W_RECORDS = b"[W::fade-out] Output doesn't look name-sorted, ejecting by only reads with an artifact"


def _tagged(in_recs, ann):
    """The input records with annotate's tags on: ann[i] = (rs, am, as, ar, ab), am '' / None without artifact strings."""
    out = []
    for r, (rs, am, as_, ar, ab) in zip(in_recs, ann):
        r = dict(r, tags=dict(r["tags"]), tag_order=list(r["tag_order"]))
        new = [("rs", ("i", str(rs)))] + ([("am", ("Z", am)), ("as", ("Z", as_)), ("ar", ("Z", ar)), ("ab", ("Z", ab))] if am else [])
        for k, v in new:
            assert k not in r["tags"]
            r["tags"][k] = v
            r["tag_order"].append(k)
        out.append(r)
    return out


def _expect(in_recs, ann, contig0):
    """(normalised records `fade out` writes, is it the grouped mode, per input record: is it written) — by the oracle; a tag
    of the test's own carries every record's index through it."""
    from oracle import pyfilter
    tagged = _tagged(in_recs, ann)
    marked = [dict(r, tags=dict(r["tags"], zi=("i", str(k))), tag_order=r["tag_order"] + ["zi"]) for k, r in enumerate(tagged)]
    lines, _ = pyfilter.fade_out(marked, contig0, False)
    first = [r["qname"] for r in in_recs[:10]]
    grouped = all(pyfilter.numerically_aware_cmp(first[k], first[k - 1]) >= 0 for k in range(1, len(first)))
    kept = [int(r["tags"]["zi"][1]) for r in samutil.parse_sam("\n".join(lines) + "\n")[1]]
    assert kept == sorted(set(kept))
    flags = [False] * len(tagged)
    for k in kept:
        flags[k] = True
    return [_norm(tagged[k]) for k in kept], grouped, flags


def _all_paths(bam, sam, fa, opts, exp, grouped, tmp_path):
    """Every format and path of `annotate --eject` on one input against exp, and against the two-step pipeline."""
    base = ["annotate", "--stats", "--timing"] + opts
    runs = {
        "dev_inflate": (_run(base + ["--eject", "-b", str(bam), str(fa)], {"FADE_BAM_INFLATE": "device"}), "bam"),
        "host_inflate": (_run(base + ["-b", "--eject", str(bam), str(fa)], {"FADE_BAM_INFLATE": "host"}), "bam"),
        "ubam": (_run(base + ["--eject", "-u", str(bam), str(fa)]), "bam"),
        "sam": (_run(base + ["--eject", str(bam), str(fa)]), "sam"),
        "sam_in_sam_out": (_run(base + ["--eject=true", str(sam), str(fa)]), "sam"),
        "host_pipeline_bam": (_run(base + ["--eject", "-b", str(bam), str(fa)], {"FADE_BAM_DEVICE": "0"}), "bam"),
    }
    plain = _ok(_run(base + ["-b", str(bam), str(fa)]))
    stats = lambda err: [l for l in err.decode().splitlines() if l.startswith(STATS)]
    assert len(stats(plain.stderr)) == 7
    mine, other = (W_GROUPS, W_RECORDS) if grouped else (W_RECORDS, W_GROUPS)
    heads = []
    for name, (p, fmt) in runs.items():
        _ok(p)
        assert (b"file path on the device" in p.stderr) == (name in ("dev_inflate", "host_inflate", "ubam")), name
        head, recs = _decode(p.stdout, fmt)
        heads.append(head)
        assert len(recs) == len(exp), (name, len(recs), len(exp))
        bad = [(name, k, a, b) for k, (a, b) in enumerate(zip(recs, exp)) if a != b]
        assert not bad, bad[:3]
        assert p.stderr.count(mine) == 1 and other not in p.stderr, name
        pg = _pg(p.stdout, fmt)
        own = [h for h in pg if "ID:fade-annotate" in h]
        assert len(own) == 1 and " --eject" in own[0] and not any("fade-extract" in h for h in pg), pg
        assert stats(p.stderr) == stats(plain.stderr), name  # the counters describe the input
        assert p.stderr.count(b"read count:") == 1, name     # ... and `out`'s own block is not printed
    assert all(h == heads[0] for h in heads)
    body = lambda out: _split(out)[1]
    assert body(runs["dev_inflate"][0].stdout) == body(runs["host_inflate"][0].stdout) == body(runs["ubam"][0].stdout) == body(runs["host_pipeline_bam"][0].stdout)
    # the product's own two-step pipeline
    anno = tmp_path / "two_step_anno.bam"
    anno.write_bytes(plain.stdout)
    assert W_GROUPS not in plain.stderr and W_RECORDS not in plain.stderr
    two = _ok(_run(["out", "-b", str(anno)]))
    assert two.stderr.count(mine) == 1 and other not in two.stderr
    head2, recs2 = _decode(two.stdout, "bam")
    assert head2 == heads[0] and recs2 == exp


@pytest.mark.parametrize("tag", ["anno_c1", "anno_c2", "anno_c5", "anno_floor0"])
def test_eject_on_the_golden_inputs_every_format_and_path(tmp_path, tag):
    recs, ann, contig0, floor_len, window = _golden_input(tag)
    exp, grouped, flags = _expect(recs, ann, contig0)
    assert 0 < len(exp) < len(recs) and sum(1 for a in ann if a[0] & 6) >= 6
    bam = tmp_path / "in.bam"
    sam = os.path.join(GOLD, tag + ".sam")
    _bam_of(sam, bam)
    _all_paths(bam, sam, os.path.join(GOLD, tag + ".fa"), ["--min-length", str(floor_len), "-w", str(window)], exp, grouped, tmp_path)


@functools.lru_cache(maxsize=None)
def _random_annotated(seed, floor_len, window):
    """The random batch of the clip test's seed (IUPAC reads, every CIGAR op, a soft-masked FASTA) and the oracle's tags of it,
    once per seed."""
    from oracle import pyoracle as oracle
    from test_gpu_fuzz import _random_batch
    oracle.build()
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
    G = oracle.GenomeHolder(names, contigs)
    reads, keep = oracle.make_reads(b)
    want = [oracle.annotate_one(G, reads[i], floor_len, window) for i in range(len(b["pos"]))]
    ann = [(w["rs"], w["am"], w["as_"], w["ar"], w["ab"]) if w["has_tags"] else (w["rs"], None, None, None, None) for w in want]
    return names, contigs, b, ann


def _group_names(seed, n, swap):
    """q<group>, the groups 1 to 4 records long (the first one record, so that the first two names differ); swap: the first
    two names change places, and the first ten are no longer non-decreasing."""
    rng = np.random.default_rng(7000 + seed)
    lens = rng.integers(1, 5, size=n)
    lens[0] = 1
    qn = ["q%d" % g for g in np.repeat(np.arange(n), lens)[:n]]
    if swap:
        qn[0], qn[1] = qn[1], qn[0]
    return qn


def _random_case(seed, floor_len, window, swap):
    names, contigs, b, ann = _random_annotated(seed, floor_len, window)
    qn = _group_names(seed, len(b["pos"]), swap)
    b = dict(b, qname=[x.encode() for x in qn])
    text = samutil.batch_to_sam(b, names, [len(c) for c in contigs], qn)
    _, in_recs = samutil.parse_sam(text)
    return names, contigs, text, in_recs, ann, qn


@pytest.mark.parametrize("swap", [False, True], ids=["name_sorted", "first_two_swapped"])
@pytest.mark.parametrize("seed,floor_len,window", [(11, 5, 100), (12, 0, 40), (13, 7, 300)])
def test_eject_on_random_reads_against_the_oracle_every_format_and_path(tmp_path, seed, floor_len, window, swap):
    names, contigs, text, in_recs, ann, qn = _random_case(seed, floor_len, window, swap)
    exp, grouped, flags = _expect(in_recs, ann, names[0])
    # from the oracle alone, before any GPU run: what the grouped mode adds is there, and the two modes differ
    _, _, _, recs_g, _, qn_g = _random_case(seed, floor_len, window, False)
    _, _, _, recs_r, _, _ = _random_case(seed, floor_len, window, True)
    exp_g, is_g, flags_g = _expect(recs_g, ann, names[0])
    exp_r, is_r, flags_r = _expect(recs_r, ann, names[0])
    assert is_g and not is_r and grouped == (not swap)
    innocent = sum(1 for k, f in enumerate(flags_g) if not f and not ann[k][0] & 6)
    starts = [k for k in range(len(qn_g)) if k == 0 or qn_g[k] != qn_g[k - 1]] + [len(qn_g)]
    kept_multi = sum(1 for s, e in zip(starts, starts[1:]) if e - s > 1 and all(flags_g[s:e]))
    print("seed %d: grouped mode ejects %d records that are no artifact calls and keeps %d groups of several records; %d / %d records written" %
          (seed, innocent, kept_multi, len(exp_g), len(exp_r)))
    assert innocent >= 100 and kept_multi >= 100, (innocent, kept_multi)
    assert [r[1:] for r in exp_g] != [r[1:] for r in exp_r] and len(exp_g) < len(exp_r)
    assert flags_r == [not a[0] & 6 for a in ann]
    sam, fa, bam = tmp_path / "in.sam", tmp_path / "ref.fa", tmp_path / "in.bam"
    sam.write_text(text)
    fa.write_text("".join(">%s\n%s\n" % (n, "\n".join(c[o:o + 70] for o in range(0, len(c), 70))) for n, c in zip(names, contigs)))
    _bam_of(sam, bam)
    _all_paths(bam, sam, fa, ["--min-length", str(floor_len), "-w", str(window)], exp, grouped, tmp_path)


# ---------------------------------------------------------------------------------------------- call boundaries
def _offsets(payload):
    off, at = [], 0
    while at < len(payload):
        off.append(at)
        at += 4 + struct.unpack_from("<I", payload, at)[0]
    assert at == len(payload)
    return off + [at]


def _qnames(payload):
    off = _offsets(payload)
    return [bytes(payload[o + 36:o + 36 + payload[o + 12] - 1]) for o in off[:-1]]


@pytest.fixture(scope="module")
def cut2000(tmp_path_factory, oracle):
    """2,000 reads of C5 in name groups of 1 to 4 and one of 40: the records' bytes, the oracle's decision, a context with the
    genome on the device, and the single-call run."""
    from oracle import pyfilter
    from fade_amd import synth
    cfg, g, b = synth.make_config("C5", 2000, contig_len=200_000)
    n = len(b["pos"])
    rng = np.random.default_rng(5)
    lens = list(rng.integers(1, 5, size=n))
    lens[300] = 40
    names = ["read%d" % k for k in np.repeat(np.arange(n), lens)[:n]]
    d = tmp_path_factory.mktemp("eject2000")
    sam = d / "in.sam"
    sam.write_text(samutil.batch_to_sam(dict(b, qname=names), g.names, [int(x) for x in g.lengths], names))
    raw = gzip.decompress(_ok(_run(["out", "-u", str(sam)])).stdout)
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    payload = raw[at:]
    assert [x.decode() for x in _qnames(payload)] == names
    G = oracle.GenomeHolder(g.names, [a.tobytes() for a in g.ascii_contigs()])
    reads, keep = oracle.make_reads(b)
    rs = [oracle.annotate_one(G, reads[i], 5, 100)["rs"] for i in range(n)]
    _, in_recs = samutil.parse_sam(sam.read_text())
    lines, _ = pyfilter.fade_out(_tagged(in_recs, [(v, None, None, None, None) for v in rs]), g.names[0], False)
    ctx = fade_amd.Context(device=0)
    ctx.genome_upload(g.names, g.ascii_contigs())
    s = dict(ctx=ctx, ref_names=g.names, payload=payload, names=names, off=_offsets(payload), rs=rs, want_names=[l.split("\t")[0] for l in lines])
    s["one"] = _cut_run(s, [])
    yield s
    ctx.close()


def _cut_run(s, cuts, eject="groups"):
    """The payload through front_raw, cut at the given offsets: (the output's record bytes, ejected, records per call)."""
    st = s["ctx"].bam_stream(s["ref_names"], floor_len=5, window=100, stored=True, eject=eject)
    try:
        edges = [0] + sorted(cuts) + [len(s["payload"])]
        out, per_call = [], []
        for j, (a, b) in enumerate(zip(edges, edges[1:])):
            st.front_raw(s["payload"][a:b], last=(j == len(edges) - 2))
            piece = st.back()
            piece = gzip.decompress(piece) if piece else b""
            out.append(piece)
            per_call.append(len(_offsets(piece)) - 1)
        return b"".join(out), st.ejected(), per_call, st.totals()
    finally:
        st.close()


def test_the_single_call_run_writes_what_the_oracle_writes(cut2000):
    s = cut2000
    out, n_ej, per_call, (stats, n_rec, _) = s["one"]
    n = len(s["names"])
    art = sum(1 for v in s["rs"] if v & 6)
    assert art >= 100 and len(s["want_names"]) < n - art  # (grouped mode takes more than the artifact calls)
    assert [x.decode() for x in _qnames(out)] == s["want_names"]
    assert n_ej == n - len(s["want_names"]) and per_call == [len(s["want_names"])]
    assert n_rec == n and stats[0] == n  # the totals describe the input
    # per-record mode on the same input: the artifact calls alone
    out_r, n_ej_r, _, _ = _cut_run(s, [], eject="records")
    assert n_ej_r == art and [x.decode() for x in _qnames(out_r)] == [q for q, v in zip(s["names"], s["rs"]) if not v & 6]
    # every record leaves with annotate's tags: the run without the flag holds the same bytes for the records that stay
    plain, n0, _, _ = _cut_run(s, [], eject=None)
    off = _offsets(plain)
    keep_r = [not v & 6 for v in s["rs"]]
    assert n0 == 0 and len(off) - 1 == n
    assert b"".join(plain[off[k]:off[k + 1]] for k in range(n) if keep_r[k]) == out_r


def _cuttings(s):
    names, off, n = s["names"], s["off"], len(s["names"])
    same = [k for k in range(1, n) if names[k] == names[k - 1]]
    head = [k for k in range(1, n) if names[k] != names[k - 1]]
    big = next(k for k in range(n) if names[k:k + 40] == [names[k]] * 40 and (k == 0 or names[k - 1] != names[k]))
    assert len(same) > 200 and len(head) > 200
    return {
        "inside_a_record_of_a_group": [off[k] + 17 for k in same[5::97]] + [off[k + 1] - 1 for k in same[11::131]],
        "between_two_records_of_a_group": [off[k] for k in same[3::61]],
        "at_group_boundaries": [off[k] for k in head[7::53]],
        # the calls between these cuts hold records of the 40-record group only: each is given back whole
        "calls_of_a_single_group": [off[big + 5] + 3, off[big + 20], off[big + 30] + 100, off[big + 38]],
        "a_byte_per_call_for_200_bytes": list(range(1, 201)),
    }


@pytest.mark.parametrize("which", ["inside_a_record_of_a_group", "between_two_records_of_a_group", "at_group_boundaries",
                                   "calls_of_a_single_group", "a_byte_per_call_for_200_bytes"])
def test_a_name_group_is_never_split_between_two_calls(cut2000, which):
    s = cut2000
    cuts = _cuttings(s)[which]
    assert len(cuts) >= 4 and len(set(cuts)) == len(cuts) and 0 < min(cuts) and max(cuts) < len(s["payload"])
    out, n_ej, per_call, (stats, n_rec, _) = _cut_run(s, cuts)
    one, n_ej_one, _, _ = s["one"]
    assert out == one and len(out) > 0
    assert n_ej == n_ej_one == len(s["names"]) - len(s["want_names"])
    assert n_rec == len(s["names"]) and sum(per_call) == len(s["want_names"])
    if which == "calls_of_a_single_group":
        assert per_call[1:4] == [0, 0, 0] and per_call[0] > 0 and per_call[4] > 0, per_call  # the calls inside the group yield nothing
    if which == "a_byte_per_call_for_200_bytes":
        assert per_call[:200] == [0] * 200


def test_eject_does_not_go_with_clip_on_the_stream(cut2000):
    for eject in ("records", "groups"):
        with pytest.raises(fade_amd.FadeHipError) as e:
            cut2000["ctx"].bam_stream(cut2000["ref_names"], clip=True, eject=eject)
        assert e.value.code == -1


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """The 30,000 reads of the clip test's `big` input (C5, names read<i // 2>: name-sorted pairs) as a BAM of ~130 BGZF
    members; `annotate --eject -b` by the host pipeline and on the device."""
    from fade_amd import synth
    d = tmp_path_factory.mktemp("ejectbig")
    cfg, g, b = synth.make_config("C5", 30000, contig_len=400_000)
    names = ["read%d" % (i // 2) for i in range(len(b["pos"]))]
    b["qname"] = names
    sam, fa, bam = d / "in.sam", d / "ref.fa", d / "in.bam"
    sam.write_text(samutil.batch_to_sam(b, g.names, [int(x) for x in g.lengths], names))
    fa.write_bytes(g.fasta_bytes())
    bam.write_bytes(_ok(_run(["out", "-b", str(sam)])).stdout)
    base = ["annotate", "--stats", "--timing", "-w", "100", "--eject"]
    host = _ok(_run(base + ["-b", str(bam), str(fa)], {"FADE_BAM_DEVICE": "0"}))
    one = _ok(_run(base + ["-b", str(bam), str(fa)]))
    assert b"file path on the device" in one.stderr and b"file path on the device" not in host.stderr
    assert one.stderr.count(W_GROUPS) == 1 and host.stderr.count(W_GROUPS) == 1
    return dict(dir=d, bam=bam, fa=fa, base=base, host=host, one=one)


@pytest.mark.parametrize("inflate", ["device", "host"])
def test_eject_on_30000_reads_with_groups_cut_by_members_and_calls(big, inflate):
    p = _ok(_run(big["base"] + ["-b", str(big["bam"]), str(big["fa"])], {"FADE_BAM_CHUNK_MB": "1", "FADE_BAM_INFLATE": inflate}))
    assert b"file path on the device" in p.stderr
    head, body = _split(p.stdout)
    assert (head, body) == _split(big["one"].stdout) == _split(big["host"].stdout)
    at = 4  # (_split's body starts with the reference list: n_ref, then l_name, name, l_ref of each)
    for _ in range(struct.unpack_from("<i", body, 0)[0]):
        at += 8 + struct.unpack_from("<i", body, at)[0]
    names = _qnames(body[at:])
    pairs = sum(1 for k in range(1, len(names)) if names[k] == names[k - 1])
    assert 2000 < len(names) < 30000 and 2 * pairs == len(names)  # a pair stays or leaves as a whole


# ---------------------------------------------------------------------------------------------- the computed result; --extract
def test_eject_goes_by_the_computed_result_not_by_tags_the_record_brought(tmp_path):
    """A record that comes in with rs:Z keeps that tag (htslib's EINVAL) and is judged by what this run computed: the artifact
    call leaves (with its name group on name-sorted input), the clean record stays.  `fade out` behind `fade annotate` cannot
    read such a tag: it would keep the artifact's group, or — record by record — drop both records."""
    tag = "anno_c5"
    recs, ann, contig0, floor_len, window = _golden_input(tag)
    exp, grouped, flags = _expect(recs, ann, contig0)
    k_art = next(k for k, a in enumerate(ann) if a[0] & 6)
    k_clean = next(k for k, a in enumerate(ann) if not a[0] & 6 and flags[k] and k > 10)
    assert not flags[k_art]
    lines = open(os.path.join(GOLD, tag + ".sam")).read().splitlines()
    body0 = next(i for i, l in enumerate(lines) if not l.startswith("@"))
    lines[body0 + k_art] += "\trs:Z:stale"
    lines[body0 + k_clean] += "\trs:Z:stale"
    sam, bam = tmp_path / "in.sam", tmp_path / "in.bam"
    sam.write_text("\n".join(lines) + "\n")
    _bam_of(sam, bam)
    fa = os.path.join(GOLD, tag + ".fa")
    opts = ["annotate", "--timing", "--min-length", str(floor_len), "-w", str(window), "--eject"]
    dev = _ok(_run(opts + ["-b", str(bam), fa]))
    host = _ok(_run(opts + ["-b", str(bam), fa], {"FADE_BAM_DEVICE": "0"}))
    assert b"file path on the device" in dev.stderr and dev.stderr.count(W_GROUPS if grouped else W_RECORDS) == 1
    assert _split(dev.stdout) == _split(host.stdout)
    samout = _ok(_run(opts + [str(sam), fa]))
    i_clean = sum(flags[:k_clean])
    for out, fmt in ((dev.stdout, "bam"), (samout.stdout, "sam")):
        _, got = _decode(out, fmt)
        assert len(got) == len(exp)
        for i, (g, e) in enumerate(zip(got, exp)):
            if i != i_clean:
                assert g == e, i
        assert got[i_clean][:11] == exp[i_clean][:11]
        assert dict((t[0], t[1:]) for t in got[i_clean][11])["rs"] == ("Z", "stale")


def test_eject_with_extract_gives_the_extract_file_of_extract_alone(tmp_path):
    tag = "anno_c2"
    recs, ann, contig0, floor_len, window = _golden_input(tag)
    bam = tmp_path / "in.bam"
    sam = os.path.join(GOLD, tag + ".sam")
    _bam_of(sam, bam)
    fa = os.path.join(GOLD, tag + ".fa")
    opts = ["annotate", "--timing", "--min-length", str(floor_len), "-w", str(window)]
    for args, env, on_device in ((["-b", str(bam), fa], None, True), (["-b", str(bam), fa], {"FADE_BAM_DEVICE": "0"}, False), ([sam, fa], None, False)):
        x1, x2 = tmp_path / "alone.x", tmp_path / "both.x"
        alone = _ok(_run(opts + ["--extract", str(x1)] + args, env))
        both = _ok(_run(opts + ["--eject", "--extract", str(x2)] + args, env))
        eject = _ok(_run(opts + ["--eject"] + args, env))
        assert (b"file path on the device" in both.stderr) == on_device
        strip = (lambda d: _split(d)) if args[0] == "-b" else (lambda d: [l for l in d.decode().splitlines() if not l.startswith("@PG")])
        assert strip(x1.read_bytes()) == strip(x2.read_bytes()) and len(x2.read_bytes()) > 200
        assert strip(both.stdout) == strip(eject.stdout) != strip(alone.stdout)
