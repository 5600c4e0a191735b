"""The early order of a level-2 run: the alignment array is copied to the host right behind the score pass,
pass 2 runs beside the copy, and the entries it wrote follow in a patch list that results lays
over the bulk copy.  Every comparison is byte for byte on rs, the stats and the alignment records (sorted by read_idx and
win_start: the device hands out entries in no fixed order), between FADEHIP_EARLY_COPY=0 and the default in fresh
contexts; one batch is also held to the oracle.  The debug line says which order a run took."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fade_amd
import samutil
from fade_amd import format_tags, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("FADEHIP_EARLY_COPY", "FADEHIP_PATCH_CAP", "FADEHIP_EARLY_TAIL", "FADEHIP_NO_SHORTCUT", "FADEHIP_CKPT", "FADEHIP_KERNEL")
EARLY, LATE = "copy order: early", "copy order: late"


def _bytes(res):
    rs, aln, st = res
    order = np.lexsort((aln["win_start"], aln["read_idx"]))
    return rs.tobytes(), aln[order].tobytes(), tuple(int(x) for x in st)


class _Ctx:
    """A fresh context under the given FADEHIP_* settings (they stay set while it is used: FADEHIP_NO_SHORTCUT is read per run)."""

    def __init__(self, monkeypatch, genome, **env):
        self.mp, self.genome, self.env = monkeypatch, genome, env

    def __enter__(self):
        for k in ENV:
            self.mp.delenv(k, raising=False)
        self.mp.setenv("FADEHIP_DEBUG", "1")
        for k, v in self.env.items():
            self.mp.setenv("FADEHIP_" + k, str(v))
        self.c = fade_amd.Context(device=0)
        self.c.genome_upload(*self.genome)
        return self.c

    def __exit__(self, *exc):
        self.c.close()
        for k in self.env:
            self.mp.delenv("FADEHIP_" + k, raising=False)


def _orders(err):
    return [EARLY if EARLY in l else LATE for l in err.splitlines() if "copy order:" in l]


@pytest.fixture(scope="module")
def rich():
    """4,000 reads of 150 bases on the repeat-rich genome under C6's laws (p_clip_indel), every read clipped and planted, so
    that pass 2 has candidates with the shortcut on and more than half the default patch capacity with it off."""
    cfg = synth.config("C6")
    cfg.update(contig_len=300_000, p_sc=1.0, p_planted=1.0)
    g = synth.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"], kind="repeat_rich")
    b = synth.make_reads(g, 4000, 7, **cfg)
    return cfg, (g.names, g.ascii_contigs()), b


@pytest.fixture(scope="module")
def rich_late(rich):
    """What today's order gives for the rich batch, shortcut on and off, and the candidates of each (computed once)."""
    cfg, genome, b = rich
    mp = pytest.MonkeyPatch()
    try:
        with _Ctx(mp, genome, EARLY_COPY=0) as c:
            on = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
            n_on = c.last_profile(0)["candidates"]
        with _Ctx(mp, genome, EARLY_COPY=0, NO_SHORTCUT=1) as c:
            off = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
            n_off = c.last_profile(0)["candidates"]
    finally:
        mp.undo()
    assert on == off
    return on, int(n_on), int(n_off)


def test_a_few_candidates_against_todays_order_and_the_oracle(rich, rich_late, oracle, monkeypatch, capfd):
    cfg, genome, b = rich
    late, n_on, n_off = rich_late
    capfd.readouterr()
    with _Ctx(monkeypatch, genome) as c:
        res = c.annotate(b, cfg["floor_len"], cfg["window"])
        assert c.last_profile(0)["candidates"] == n_on
    err = capfd.readouterr().err
    assert _orders(err) == [EARLY], err[-600:]
    assert "patch list of %d entries" % n_on in err and n_on > 0, err[-600:]
    assert _bytes(res) == late
    rs, aln, st = res
    names = genome[0]
    tags = format_tags(b, names, rs, aln)
    G = oracle.GenomeHolder(names, [a.tobytes() for a in genome[1]])
    ors, oam = oracle.annotate_batch_soa(G, b, cfg["floor_len"], cfg["window"], threads=8)
    assert np.array_equal(rs, ors), np.nonzero(rs != ors)[0][:10]
    n_art = 0
    for i in range(len(ors)):
        if oam[i] is None:
            assert i not in tags
        else:
            assert tags[i]["am"] == oam[i], i
            n_art += 1
    assert n_art > 100


def test_every_candidate_through_pass2_twice_on_the_slot(rich, rich_late, monkeypatch, capfd):
    """Default capacity: the first run is early (its list is longer than what was sent with the run), it leaves more than half
    the capacity in candidates, so the second run takes today's order."""
    cfg, genome, b = rich
    late, _, n_off = rich_late
    assert 2 * n_off > 4096
    capfd.readouterr()
    with _Ctx(monkeypatch, genome, NO_SHORTCUT=1) as c:
        first = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
        second = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
    err = capfd.readouterr().err
    assert _orders(err) == [EARLY, LATE], err[-800:]
    assert "exceed half the patch list" in err
    assert first == late and second == late


@pytest.mark.parametrize("short", [0, 1], ids=["the_last_fits", "the_first_overflows"])
def test_patch_capacity_at_the_number_of_candidates(rich, rich_late, monkeypatch, capfd, short):
    cfg, genome, b = rich
    late, _, n_off = rich_late
    capfd.readouterr()
    with _Ctx(monkeypatch, genome, NO_SHORTCUT=1, PATCH_CAP=n_off - short) as c:
        got = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
    err = capfd.readouterr().err
    assert _orders(err) == [EARLY], err[-600:]
    assert "patch list of %d entries" % n_off in err, err[-600:]
    assert ("overflow" in err) == bool(short), err[-600:]
    assert got == late


def _both(monkeypatch, genome, run):
    """run(ctx) under today's order and under the default, in fresh contexts."""
    out = []
    for env in (dict(EARLY_COPY=0), {}):
        with _Ctx(monkeypatch, genome, **env) as c:
            out.append(run(c))
    return out


def test_no_candidates_is_an_empty_patch_list(monkeypatch, capfd):
    cfg = synth.config("C2")
    cfg.update(contig_len=300_000, p_sc=0.5, p_planted=0.0, clip_min=20)  # random clips of 20 bases and more: none scores 1.8 x its length
    g = synth.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
    b = synth.make_reads(g, 3000, 11, **cfg)
    capfd.readouterr()

    def run(c):
        r = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
        assert c.last_profile(0)["candidates"] == 0 and c.last_profile(0)["alignments"] > 1000
        return r
    a, e = _both(monkeypatch, (g.names, g.ascii_contigs()), run)
    err = capfd.readouterr().err
    assert _orders(err) == [LATE, EARLY] and "patch list of 0 entries" in err, err[-600:]
    assert a == e


def _one_candidate_batch():
    """16 clipped reads of 150 bases: fifteen with a random clip, one whose 100-base clip is the reverse strand of a window
    segment with one base left out, so that its best path has a gap and the forced-diagonal walk cannot settle it."""
    rng = np.random.default_rng(5)
    n, lq, window = 40_000, 150, 200
    ref = "".join("ACGT"[k] for k in rng.integers(0, 4, size=n))
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    recs, pos = [], 1000
    for i in range(16):
        if i == 9:
            seg = pos - 160
            clip = rc(ref[seg:seg + 50] + ref[seg + 51:seg + 101])
            recs.append(("100S50M", clip + ref[pos:pos + 50], pos))
        else:
            clip = "".join("ACGT"[k] for k in rng.integers(0, 4, size=30))
            recs.append(("30S120M", clip + ref[pos:pos + 120], pos))
        pos += 2000
    lines = ["\t".join(["r%d" % i, "0", "c1", str(p + 1), "60", cig, "*", "0", "0", seq, "I" * lq]) for i, (cig, seq, p) in enumerate(recs)]
    names, lens, batch, qnames = samutil.sam_to_batch("@SQ\tSN:c1\tLN:%d\n" % n + "\n".join(lines) + "\n")
    return (names, [ref.encode()]), batch, window


def test_one_candidate_is_a_single_octet(monkeypatch, capfd, oracle):
    genome, b, window = _one_candidate_batch()
    capfd.readouterr()

    def run(c):
        res = c.annotate(b, 5, window)
        assert c.last_profile(0)["candidates"] == 1 and c.last_profile(0)["alignments"] == 16
        return res
    a, e = _both(monkeypatch, genome, run)
    err = capfd.readouterr().err
    assert _orders(err) == [LATE, EARLY] and "patch list of 1 entries" in err, err[-600:]
    assert _bytes(a) == _bytes(e)
    G = oracle.GenomeHolder(genome[0], [s.decode() for s in genome[1]])
    ors, oam = oracle.annotate_batch_soa(G, b, 5, window, threads=2)
    assert np.array_equal(e[0], ors)
    tags = format_tags(b, genome[0], e[0], e[1])
    for i in range(16):
        assert (oam[i] is None) == (i not in tags) and (oam[i] is None or tags[i]["am"] == oam[i]), i


def test_two_read_lengths_take_todays_order(monkeypatch, capfd):
    cfg = synth.config("C6")
    cfg.update(contig_len=300_000, p_sc=0.5)
    g = synth.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"], kind="repeat_rich")
    b = synth.concat([synth.make_reads(g, 1500, 3, **dict(cfg, read_len=100)), synth.make_reads(g, 1500, 4, **cfg)])
    capfd.readouterr()
    a, e = _both(monkeypatch, (g.names, g.ascii_contigs()), lambda c: _bytes(c.annotate(b, cfg["floor_len"], cfg["window"])))
    err = capfd.readouterr().err
    assert _orders(err) == [LATE, LATE] and "not exactly one class list" in err, err[-600:]
    assert a == e and len(a[1]) > 0


@pytest.fixture(scope="module")
def mild():
    """3,000 reads under C6's laws, half of them clipped: a few hundred alignments a run, some of them pass-2 candidates."""
    cfg = synth.config("C6")
    cfg.update(contig_len=300_000, p_sc=0.5)
    g = synth.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"], kind="repeat_rich")
    return cfg, (g.names, g.ascii_contigs()), synth.make_reads(g, 3000, 21, **cfg)


# (the two tests below run a slot more than once; a slot whose previous run sent more than 1/32 of its alignments to pass 2
# leaves snapshots in the next, which takes today's order: FADEHIP_CKPT=0 pins the snapshots off in both contexts)
def test_the_same_batch_run_again_without_an_upload(mild, monkeypatch, capfd):
    """The results of a run are views into the slot's pinned block, valid and unchanged until the slot is RUN again (§4): the
    patch list is laid over the bulk copy once, when the results are first asked for."""
    cfg, genome, b = mild
    other = synth.take(b, np.arange(1000))
    capfd.readouterr()

    def run(c):
        c.annotate_upload(2, b)
        c.annotate_run(2, cfg["floor_len"], cfg["window"])
        v1 = c.annotate_results(2)
        assert c.last_profile(2)["candidates"] > 0
        keep = (v1[0].copy(), v1[1].copy())
        v1b = c.annotate_results(2)  # asking again changes nothing
        assert v1b[1].ctypes.data == v1[1].ctypes.data and v1b[1].tobytes() == keep[1].tobytes()
        c.annotate_upload(2, other)  # the next batch goes up: run 1's views stay as they are ...
        c.sync()
        assert v1[0].tobytes() == keep[0].tobytes() and v1[1].tobytes() == keep[1].tobytes()
        out = [_bytes((keep[0], keep[1], v1[2]))]
        c.annotate_upload(2, b)
        c.annotate_run(2, cfg["floor_len"], cfg["window"])
        out.append(_bytes(c.annotate_results(2)))
        c.annotate_run(2, cfg["floor_len"], cfg["window"])  # no new upload: the same batch again
        out.append(_bytes(c.annotate_results(2)))
        return out
    a, e = [], []
    for env, out in ((dict(EARLY_COPY=0, CKPT=0), a), (dict(CKPT=0), e)):
        with _Ctx(monkeypatch, genome, **env) as c:
            out.extend(run(c))
    err = capfd.readouterr().err
    assert _orders(err) == [LATE] * 3 + [EARLY] * 3, err[-800:]
    assert a == e and e[0] == e[1] == e[2]


def test_two_slots_in_flight_fetched_in_the_other_order(mild, monkeypatch, capfd):
    cfg, genome, b = mild
    parts = [synth.take(b, np.arange(0, 1500)), synth.take(b, np.arange(1500, 3000))]
    capfd.readouterr()

    def run(c):
        out = []
        for rnd in range(2):  # the second round runs on slots that have a previous run behind them
            for k in (0, 1):
                c.annotate_upload(k, parts[k ^ rnd])
                c.annotate_run(k, cfg["floor_len"], cfg["window"])
            got = {}
            for k in (1, 0):
                got[k] = _bytes(c.annotate_results(k))
            out.append((got[0], got[1]))
        return out
    a, e = [], []
    for env, out in ((dict(EARLY_COPY=0, CKPT=0), a), (dict(CKPT=0), e)):
        with _Ctx(monkeypatch, genome, **env) as c:
            out.extend(run(c))
    err = capfd.readouterr().err
    assert _orders(err) == [LATE] * 4 + [EARLY] * 4, err[-800:]
    assert a == e and a[0][0] == a[1][1] and a[0][0] != a[0][1]


@pytest.mark.parametrize("tail", ["masked", "plain"])
def test_pass2_on_a_tail_stream_of_its_own(mild, monkeypatch, capfd, tail):
    """FADEHIP_EARLY_TAIL: the A/B variants that copy on the slot's stream and run pass 2 on a tail stream."""
    cfg, genome, b = mild
    capfd.readouterr()
    out = []
    for env in (dict(EARLY_COPY=0), dict(EARLY_TAIL=tail)):
        with _Ctx(monkeypatch, genome, **env) as c:
            out.append(_bytes(c.annotate(b, cfg["floor_len"], cfg["window"])))
            assert c.last_profile(0)["candidates"] > 0
    err = capfd.readouterr().err
    assert _orders(err) == [LATE, EARLY] and "pass 2 on" in err, err[-600:]
    assert out[0] == out[1]


def test_the_file_path_keeps_todays_order(tmp_path):
    """device_only runs (fade annotate on a BAM file) leave their results on the device: today's order, the same output."""
    gold = os.path.join(ROOT, "tests", "golden")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "sam2bam"])
    bam = tmp_path / "in.bam"
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), os.path.join(gold, "anno_c2.sam")], stdout=fo)
    p = dict(kv.split("=") for line in open(os.path.join(gold, "anno_c2.expected.tsv")) if line.startswith("#floor_len") for kv in line[1:].split())
    args = [os.path.join(ROOT, "fade_amd", "fade"), "annotate", "--timing", "--min-length", p["floor_len"], "-w", p["window"], "-b", str(bam), os.path.join(gold, "anno_c2.fa")]
    outs = []
    for env in ({}, {"FADEHIP_EARLY_COPY": "0"}):
        e = {k: v for k, v in os.environ.items() if k not in ENV}
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(e, FADEHIP_DEBUG="1", **env))
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        err = r.stderr.decode()
        assert "file path on the device" in err
        assert _orders(err) and set(_orders(err)) == {LATE}, err[-800:]
        assert ("results stay on the device" in err) == (not env)
        outs.append(gzip.decompress(r.stdout))
    assert outs[0] == outs[1] and len(outs[0]) > 1000
