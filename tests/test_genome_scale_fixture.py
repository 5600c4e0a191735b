"""The large-genome fixture (tests/genome_scale.py) and the oracle's zero-copy genome, on the CPU: the fixture crosses base
2^31, base 2^32 and byte 2^31 where it says it does, its planted windows tell a truncated offset from the true one, and the
oracle gives the same answers on views of one array as on copied contigs."""
import ctypes as C

import numpy as np
import pytest

import genome_scale as GS
from fade_amd import synth

READ_LENS = (36, 150, 512, 700, 4096, 5000)


@pytest.fixture(scope="module")
def G():
    return GS.ScaleGenome()


def test_packed_bases_follow_the_librarys_rounding():
    base, total = GS.packed_bases([1, 16, 17, 0, 33])
    assert list(base) == [0, 16, 32, 64, 64] and total == 112


def test_the_fixture_crosses_2p31_and_2p32_bases_and_2p31_bytes(G):
    n = len(G.names)
    assert n > 3000 and len(set(G.names)) == n
    assert G.total > (1 << 32) + GS.BIG_HI_LEN and G.total // 2 > (1 << 31)
    # the big contigs are views of the pool (no copy), of chr1's length, and one of them holds base 2^31, another 2^32
    for c in G.big:
        assert G.lengths[c] == GS.CHR1_LEN and np.shares_memory(G.seqs[c], G.pool)
    c31, _ = G.point_local(1 << 31)
    c32, p32 = G.point_local(1 << 32)
    assert c31 in G.big and c32 in G.big and c31 != c32
    assert G.base[c32] < (1 << 32) < G.base[c32] + G.lengths[c32]
    # a contig longer than 100 Mbp wholly above base 2^32, and every base of the short contigs after it too
    assert G.base[G.big_hi] > (1 << 32) and G.lengths[G.big_hi] > 100_000_000
    assert G.big_hi + 1 + GS.N_TAIL == n and G.base[G.big_hi + 1] > (1 << 32)
    assert all(500 <= G.lengths[c] <= 5000 for c in range(G.big_hi + 1, n))
    # a late contig with a long name; long names elsewhere too; the last contig ends the packed buffer on a half byte
    assert GS.LATE_LONG >= 3000 and len(G.names[GS.LATE_LONG]) >= 200
    assert sum(len(x) >= 200 for x in G.names) >= 30
    assert G.lengths[G.last] % 2 == 1 and G.base[G.last] + G.lengths[G.last] <= G.total < G.base[G.last] + G.lengths[G.last] + 16
    # the packed view agrees with the contigs on both sides of 2^32
    w = G.packed_window((1 << 32) - 5, 10)
    assert np.array_equal(w, G.seqs[c32][p32 - 5:p32 + 5])


def test_planted_windows_discriminate_true_from_truncated_offsets(G):
    """For every site and read length: the windows straddle / touch what the site claims, start at every residue mod 8 of
    the packed buffer, and hold bases that differ from those at the true offset - 2^32 and at the true offset mod 2^31."""
    S = GS.sites(G)
    residues = set()
    for L in READ_LENS:
        b, labels = GS.site_batch(G, L, 100, GS.n_per_site(L))
        labels = [lab for lab, t, co0, co1 in zip(labels, b["tid"], b["cigar_off"][:-1], b["cigar_off"][1:])
                  if t >= 0 and np.any((b["cigar_ops"][co0:co1] & 15) == 4)]
        wins = GS.windows(G, b, 100)
        assert len(wins) == len(labels) > 0
        seen = {}
        for lab, (c, s, e) in zip(labels, wins):
            assert c == S[lab][0]
            assert GS.discriminates(G, c, s, e), (lab, L, c, s, e)
            residues.add(int(G.base[c] + s) % 8)
            point = S[lab][3]
            hit = (point is not None and G.base[c] + s <= point < G.base[c] + e) or \
                  (point is None and (s < 512 or e > G.lengths[c] - 512)) or lab == "late_long_name"  # near a contig end
            seen[lab] = seen.get(lab, 0) + int(hit)
        assert seen["straddle_2p31"] >= 2 and seen["straddle_2p32"] >= 2, (L, seen)
        assert seen["big_high_start"] >= 1 and seen["big_high_end"] >= 1, (L, seen)
        if L <= 4096:
            assert seen.get("buffer_end", 0) >= 1 and seen.get("late_long_name", 0) >= 1, (L, seen)
        if L <= 512:
            assert seen.get("genome_start", 0) >= 1, (L, seen)
    assert residues == set(range(8))


def test_the_oracle_reads_views_of_one_array_like_copied_contigs(oracle):
    """GenomeHolder on numpy views (by pointer, kept alive) against GenomeHolder on bytes: the same rs and tags."""
    g = synth.Genome(3, 60_000, 5)
    pool = np.ascontiguousarray(np.concatenate(g.ascii_contigs()))
    views = [pool[g.offsets[k]:g.offsets[k + 1]] for k in range(3)]
    copied = oracle.GenomeHolder(g.names, [v.tobytes() for v in views])
    viewed = oracle.GenomeHolder(g.names, views)
    ptrs = C.cast(viewed._seqs, C.POINTER(C.c_void_p))
    assert [ptrs[k] for k in range(3)] == [v.ctypes.data for v in views]  # no copy
    b = synth.make_reads(g, 3000, 9, read_len=150, window=100, p_sc=0.4, p_planted=0.8)
    rs0, am0 = oracle.annotate_batch_soa(copied, b, 5, 100, threads=4)
    rs1, am1 = oracle.annotate_batch_soa(viewed, b, 5, 100, threads=4)
    assert np.array_equal(rs0, rs1) and am0 == am1
    tagged = np.nonzero((rs0 >> 1) & 3)[0]
    assert len(tagged) > 50
    reads, keep = oracle.make_reads(b)
    for i in tagged[:100]:
        assert oracle.annotate_one(copied, reads[int(i)], 5, 100) == oracle.annotate_one(viewed, reads[int(i)], 5, 100)
    # str contigs are still taken (copied) as before
    as_str = oracle.GenomeHolder(g.names, [v.tobytes().decode() for v in views])
    assert np.array_equal(oracle.annotate_batch_soa(as_str, b, 5, 100, threads=4)[0], rs0)


def test_genome_upload_passes_views_by_pointer():
    """Context.genome_upload hands the library the views' own addresses (no host copy of a multi-gigabase genome)."""
    import fade_amd

    seen = {}

    class FakeLib:
        def fadehip_genome_upload(self, h, n, lens, ptrs):
            seen["lens"] = list(C.cast(lens, C.POINTER(C.c_int64))[:n])
            seen["ptrs"] = list(C.cast(ptrs, C.POINTER(C.c_void_p))[:n])
            return 0

    ctx = fade_amd.Context.__new__(fade_amd.Context)
    ctx._L, ctx._h = FakeLib(), None
    pool = np.frombuffer(b"ACGT" * 1000, dtype=np.uint8)
    views = [pool[0:1000], pool[500:3999], pool[3999:4000]]
    ctx.genome_upload(["a", "b", "c"], views)
    assert seen["lens"] == [1000, 3499, 1] and seen["ptrs"] == [v.ctypes.data for v in views]
    assert ctx.contig_names == ["a", "b", "c"]
