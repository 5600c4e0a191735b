"""The tail of a run in the early order: rs leaves with the alignment array behind the score pass, a pass-2
candidate's final rs byte rides in its patch entry, the run's counter block rides in the patch block, and the slot's other
counter block is zeroed beside the score pass, so that ONE copy ends the run.  Every comparison is byte for byte on rs, the
stats and the alignment records (sorted by read_idx and win_start) between FADEHIP_EARLY_COPY=0 and the default in fresh
contexts, as in test_gpu_early_copy.py; one batch is also held to the oracle."""
import numpy as np
import pytest

import fade_amd
from fade_amd import format_tags, synth

pytestmark = pytest.mark.gpu

ENV = ("FADEHIP_EARLY_COPY", "FADEHIP_PATCH_CAP", "FADEHIP_EARLY_TAIL", "FADEHIP_NO_SHORTCUT", "FADEHIP_CKPT", "FADEHIP_KERNEL")
EARLY, LATE = "copy order: early", "copy order: late"
ART_BITS = 0x1e  # rs bits 1 - 4: set by whoever walks the traceback (with the shortcut off: pass 2 alone)


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


def _profile(c, slot=0):
    p = c.last_profile(slot)
    return int(p["alignments"]), int(p["candidates"]), int(p["cells"])


@pytest.fixture(scope="module")
def rich():
    """test_gpu_early_copy.py's rich recipe: 4,000 reads of 150 bases on the repeat-rich genome under C6's laws, every read
    clipped and planted: pass 2 has candidates with the shortcut on, and sets rs bits on thousands with it off."""
    cfg = synth.config("C6")
    cfg.update(contig_len=300_000, p_sc=1.0, p_planted=1.0)
    g = synth.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"], kind="repeat_rich")
    b = synth.make_reads(g, 4000, 7, **cfg)
    return cfg, (g.names, g.ascii_contigs()), b


@pytest.fixture(scope="module")
def rich_late(rich):
    """Today's order on the rich batch and on its first 700 reads, shortcut on and off, with the runs' profiles (computed once)."""
    cfg, genome, b = rich
    small = synth.take(b, np.arange(700))
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for name, env in (("on", {}), ("off", dict(NO_SHORTCUT=1))):
            with _Ctx(mp, genome, EARLY_COPY=0, **env) as c:
                out[name] = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
                out[name + "_profile"] = _profile(c)
                out[name + "_small"] = _bytes(c.annotate(small, cfg["floor_len"], cfg["window"]))
    finally:
        mp.undo()
    assert out["on"] == out["off"] and out["on_small"] == out["off_small"]
    return out


def _gate_rs(b, floor_len):
    """rs as the gate leaves it (anno.d:61-74), which is what a pass-2 candidate's byte still is when the score pass ends."""
    co = b["cigar_off"].astype(np.int64)
    rs = np.zeros(len(b["pos"]), dtype=np.uint8)
    for i in range(len(rs)):
        ops = b["cigar_ops"][co[i]:co[i + 1]]
        if (int(b["flag"][i]) & 4) or not np.any((ops & 15) == 4):
            continue
        rs[i] = 1 | (32 if b["has_sa"][i] else 0)
    return rs


def test_rs_of_the_candidates_comes_in_the_patch_entries(rich, rich_late, oracle, monkeypatch, capfd):
    """Shortcut off: every artifact call is pass 2's, made after rs has left behind the score pass.  A slot's first run sends 64
    entries with the run, so the rest of the list is fetched too."""
    cfg, genome, b = rich
    n_cand = rich_late["off_profile"][1]
    capfd.readouterr()
    with _Ctx(monkeypatch, genome, NO_SHORTCUT=1) as c:
        res = c.annotate(b, cfg["floor_len"], cfg["window"])
        assert _profile(c) == rich_late["off_profile"]
    err = capfd.readouterr().err
    assert _orders(err) == [EARLY], err[-600:]
    assert "patch list of %d entries (64 sent with the run)" % n_cand in err and n_cand > 64, err[-600:]
    assert _bytes(res) == rich_late["off"]
    rs, aln, st = res
    # the patch is not vacuous: records on the list whose byte pass 2 changed after the score pass
    changed = np.nonzero(rs != _gate_rs(b, cfg["floor_len"]))[0]
    assert len(changed) > 100 and np.all(rs[changed] & ART_BITS)
    # ... and the batch against the oracle
    G = oracle.GenomeHolder(genome[0], [a.tobytes() for a in genome[1]])
    ors, oam = oracle.annotate_batch_soa(G, b, cfg["floor_len"], cfg["window"], threads=8)
    assert np.array_equal(rs, ors), np.nonzero(rs != ors)[0][:10]
    tags = format_tags(b, genome[0], rs, aln)
    for i in range(len(ors)):
        assert (oam[i] is None) == (i not in tags) and (oam[i] is None or tags[i]["am"] == oam[i]), i


def test_a_few_candidates_and_the_same_profile(rich, rich_late, monkeypatch, capfd):
    cfg, genome, b = rich
    capfd.readouterr()
    with _Ctx(monkeypatch, genome) as c:
        res = c.annotate(b, cfg["floor_len"], cfg["window"])
        prof = _profile(c)
    err = capfd.readouterr().err
    assert _orders(err) == [EARLY], err[-600:]
    assert prof == rich_late["on_profile"] and prof[0] > 3000 and prof[1] > 0 and prof[2] > 0
    assert _bytes(res) == rich_late["on"]


def test_no_candidates_at_all(monkeypatch, capfd):
    cfg = synth.config("C2")
    cfg.update(contig_len=300_000, p_sc=0.5, p_planted=0.0, clip_min=20)  # random clips of 20 bases and more: none scores 1.8 x its length
    g = synth.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"])
    b = synth.make_reads(g, 3000, 11, **cfg)
    capfd.readouterr()
    out = []
    for env in (dict(EARLY_COPY=0), {}):
        with _Ctx(monkeypatch, (g.names, g.ascii_contigs()), **env) as c:
            out.append((_bytes(c.annotate(b, cfg["floor_len"], cfg["window"])), _profile(c)))
    err = capfd.readouterr().err
    assert _orders(err) == [LATE, EARLY] and "patch list of 0 entries" in err, err[-600:]
    assert out[0] == out[1] and out[0][1][1] == 0 and out[0][1][0] > 1000


def test_an_overflowing_patch_list_brings_the_array_and_rs_again(rich, rich_late, monkeypatch, capfd):
    """FADEHIP_PATCH_CAP one below the candidates: results copies the array and rs again, and the slot's next run is late."""
    cfg, genome, b = rich
    n_cand = rich_late["off_profile"][1]
    capfd.readouterr()
    with _Ctx(monkeypatch, genome, NO_SHORTCUT=1, PATCH_CAP=n_cand - 1) as c:
        first = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
        second = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
        third = _bytes(c.annotate(synth.take(b, np.arange(700)), cfg["floor_len"], cfg["window"]))
    err = capfd.readouterr().err
    assert _orders(err) == [EARLY, LATE, LATE], err[-800:]
    assert "overflow: the array was copied again" in err and "exceed half the patch list" in err, err[-800:]
    assert first == rich_late["off"] and second == rich_late["off"] and third == rich_late["off_small"]


def test_two_slots_alternate_a_large_and_a_small_batch(rich, rich_late, monkeypatch, capfd):
    """Stale patch entries and stale counter blocks: each slot sees 4,000, 700, 4,000 reads (or the other way round), every
    run early, with the slot's other counter block zeroed by the run before."""
    cfg, genome, b = rich
    parts = [b, synth.take(b, np.arange(700))]
    want = [rich_late["on"], rich_late["on_small"]]
    capfd.readouterr()
    with _Ctx(monkeypatch, genome, CKPT=0) as c:
        for rnd in range(3):
            for k in (0, 1):
                c.annotate_upload(k, parts[(k + rnd) & 1])
                c.annotate_run(k, cfg["floor_len"], cfg["window"])
            for k in (1, 0):
                assert _bytes(c.annotate_results(k)) == want[(k + rnd) & 1], (rnd, k)
    err = capfd.readouterr().err
    assert _orders(err) == [EARLY] * 6, err[-800:]


def test_two_read_lengths_take_todays_order(monkeypatch, capfd):
    cfg = synth.config("C6")
    cfg.update(contig_len=300_000, p_sc=0.5)
    g = synth.Genome(cfg["n_contigs"], cfg["contig_len"], cfg["genome_seed"], kind="repeat_rich")
    b = synth.concat([synth.make_reads(g, 1500, 3, **dict(cfg, read_len=100)), synth.make_reads(g, 1500, 4, **cfg)])
    capfd.readouterr()
    out = []
    for env in (dict(EARLY_COPY=0), {}):
        with _Ctx(monkeypatch, (g.names, g.ascii_contigs()), **env) as c:
            first = _bytes(c.annotate(b, cfg["floor_len"], cfg["window"]))
            out.append((first, _bytes(c.annotate(b, cfg["floor_len"], cfg["window"])), _profile(c)))
    err = capfd.readouterr().err
    assert _orders(err) == [LATE] * 4 and "not exactly one class list" in err, err[-600:]
    assert out[0] == out[1] and out[0][0] == out[0][1] and len(out[0][0][1]) > 0
