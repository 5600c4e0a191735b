"""A human-sized-and-larger genome for the annotate tests, built on the CPU in a few seconds and a few hundred MB.

The packed genome the library keeps in HBM (fadehip_genome_upload) is addressed by 64-bit base offsets.  This fixture puts
windows past base 2^31 (a signed-int overflow), past base 2^32 (a 32-bit wrap; also byte 2^31 of the packed buffer), at the
very start and the very end of the packed buffer, on a contig with an index above 3,000 and a long name.  Reads are planted
at those sites so that their true windows hold bases that differ from where a truncated offset would read.

Layout (contig order = packed order):
  - N_HEAD short contigs of 1-4 kb (contig 0 is the genome's first base), names of varied length;
  - N_BIG contigs of chr1's length, each a view at its own offset into one seeded random ACGT pool;
  - one contig of BIG_HI_LEN bases, also a view of the pool, that lies wholly above base 2^32;
  - N_TAIL short contigs of 0.5-5 kb with their own random content, a few with names of 200+ characters.
Every contig is a uint8 numpy array (ASCII residues); the big ones share the pool's memory.
"""
import numpy as np

from fade_amd import synth

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE_OF_ASCII = np.zeros(256, dtype=np.uint8)
for _k, _c in enumerate(b"ACGT"):
    CODE_OF_ASCII[_c] = _k

CHR1_LEN = 248_956_422
N_HEAD, N_BIG, N_TAIL = 40, 18, 3000
BIG_HI_LEN = 120_000_001
POOL_LEN = 270_000_000
BIG_STRIDE = 1_000_003         # pool offset of big contig k: k * BIG_STRIDE
BIG_HI_AT = 123_456_789        # pool offset of the contig above 2^32
SEED = 20261016
LONG_NAME_EVERY = 97           # every 97th tail contig has a name of 200+ characters
LATE_LONG = N_HEAD + N_BIG + 1 + 2960   # a contig with an index >= 3,000 and a long name (forced)
LAST_LEN = 4999                # the last contig: odd, so the packed buffer ends on a half byte


def packed_bases(lengths):
    """The library's own rule (fadehip_genome_upload): each contig starts where the previous one's length, rounded up to 16
    bases, ends.  Returns (first packed base of every contig, total packed bases)."""
    padded = (np.asarray(lengths, dtype=np.int64) + 15) & ~np.int64(15)
    base = np.zeros(len(padded), dtype=np.int64)
    np.cumsum(padded[:-1], out=base[1:])
    return base, int(padded.sum())


def _random_acgt(rng, n, chunk=1 << 24):
    out = rng.integers(0, 4, size=n, dtype=np.uint8)
    for a in range(0, n, chunk):
        out[a:a + chunk] = ACGT[out[a:a + chunk]]
    return out


class ScaleGenome:
    def __init__(self, seed=SEED):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.pool = _random_acgt(rng, POOL_LEN)
        names, seqs = [], []
        head_lens = rng.integers(1000, 4001, size=N_HEAD)
        head_lens[0] = 4000
        head = _random_acgt(rng, int(head_lens.sum()))
        at = 0
        for k, L in enumerate(head_lens):
            names.append("h%d" % k + "_" * int(k % 7) + "x" * int(3 * (k % 11)))
            seqs.append(head[at:at + L])
            at += L
        self.big = list(range(N_HEAD, N_HEAD + N_BIG))
        for k in range(N_BIG):
            names.append("chr%d" % (k + 1))
            seqs.append(self.pool[k * BIG_STRIDE:k * BIG_STRIDE + CHR1_LEN])
        self.big_hi = len(names)
        names.append("chrHigh_above_2p32")
        seqs.append(self.pool[BIG_HI_AT:BIG_HI_AT + BIG_HI_LEN])
        tail_lens = rng.integers(500, 5001, size=N_TAIL)
        tail_lens[-1] = LAST_LEN
        tail_lens[LATE_LONG - self.big_hi - 1] = 5000
        tail = _random_acgt(rng, int(tail_lens.sum()))
        at = 0
        for k, L in enumerate(tail_lens):
            idx = len(names)
            name = "t%04d" % k
            if k % LONG_NAME_EVERY == 0 or idx == LATE_LONG:
                name += "_" + "".join(chr(c) for c in rng.choice(np.frombuffer(b"ACGTacgt0123456789.:_|-", np.uint8), 200 + k % 60))
            names.append(name)
            seqs.append(tail[at:at + L])
            at += L
        self.names = names
        self.seqs = seqs
        self.lengths = np.array([len(s) for s in seqs], dtype=np.int64)
        self.base, self.total = packed_bases(self.lengths)
        self.last = len(names) - 1

    # ---- what the packed buffer holds at a base offset (the pad bases of the rounding read as 0)
    def contig_at(self, g):
        c = int(np.searchsorted(self.base, g, side="right")) - 1
        return c, int(g - self.base[c])

    def packed_window(self, g, n):
        """n residues (uint8 ASCII, 0 for the pad bases of the rounding) at packed base offset g."""
        out = np.zeros(n, dtype=np.uint8)
        k = 0
        while k < n and g + k < self.total:
            c, p = self.contig_at(g + k)
            take = min(n - k, int(self.base[c] + ((self.lengths[c] + 15) & ~15)) - (g + k))
            seg = self.seqs[c][p:p + take]
            out[k:k + len(seg)] = seg
            k += take
        return out

    def point_local(self, g):
        """(contig, local position) of packed base g, which must lie inside a contig."""
        c, p = self.contig_at(g)
        assert p < self.lengths[c], (g, c, p)
        return c, p


class _Slice:
    """The object synth.make_reads draws reads from: one contig, the bases [lo, hi) of a real one."""

    def __init__(self, seq, lo, hi):
        self.names = ["s"]
        self.lengths = np.array([hi - lo], dtype=np.int64)
        self.offsets = np.array([0, hi - lo], dtype=np.int64)
        self.codes = CODE_OF_ASCII[seq[lo:hi]]


def sites(G):
    """name -> (contig, lo, hi, point): a region of one contig, and the packed base its reads' windows are built around
    (None where the region itself is the point: the ends of contigs and of the buffer)."""
    out = {}
    for name, g in (("straddle_2p31", 1 << 31), ("straddle_2p32", 1 << 32)):
        c, p = G.point_local(g)
        out[name] = (c, p, p, g)
    L = int(G.lengths[G.big_hi])
    out["big_high_start"] = (G.big_hi, 0, 0, None)
    out["big_high_end"] = (G.big_hi, L, L, None)
    out["genome_start"] = (0, 0, 0, None)
    out["buffer_end"] = (G.last, int(G.lengths[G.last]), int(G.lengths[G.last]), None)
    out["late_long_name"] = (LATE_LONG, 2500, 2500, None)
    return out


def site_region(G, site, read_len, window):
    """[lo, hi) of the contig to draw reads of read_len from: around the site's point, at most what the contig holds."""
    c, a, b, _ = site
    R = max(read_len, 350) + window + 100  # a fragment (insert ~350) and most of its reads' windows
    L = int(G.lengths[c])
    lo, hi = max(0, a - R // 2), min(L, b + R // 2)
    if hi - lo < R:  # at a contig end: extend into the contig
        lo, hi = max(0, min(lo, hi - R)), min(L, max(hi, lo + R))
    return lo, hi


def site_reads(G, site, n, seed, read_len, window):
    """n reads planted at the site (synth.make_reads on the region: most clipped reads carry planted artifacts), tid /
    pos moved back to the real contig.  None if the contig is too short for reads of read_len."""
    c = site[0]
    lo, hi = site_region(G, site, read_len, window)
    if hi - lo < read_len + 200:
        return None
    b = synth.make_reads(_Slice(G.seqs[c], lo, hi), n, seed, read_len=read_len, window=window, p_sc=0.6, clip_min=6,
                         clip_max=max(7, min(60, read_len // 3)), p_planted=0.9, p_unmapped=0.02)
    mapped = b["tid"] >= 0
    b["tid"] = np.where(mapped, c, -1).astype(np.int32)
    b["pos"] = np.where(mapped, b["pos"].astype(np.int64) + lo, -1).astype(np.int32)
    b.pop("_truth", None)
    return b


def windows(G, batch, window):
    """Per mapped record with an S op: (contig, window start, window end) as analysis.d:45-59 computes them."""
    out = []
    co = np.asarray(batch["cigar_off"], dtype=np.int64)
    ops = np.asarray(batch["cigar_ops"])
    for i in range(len(batch["pos"])):
        t = int(batch["tid"][i])
        o = ops[co[i]:co[i + 1]]
        if t < 0 or not np.any((o & 15) == 4):
            continue
        aligned = int(sum(int(x) >> 4 for x in o if (int(x) & 15) in (0, 2, 3, 7, 8)))
        p = int(batch["pos"][i])
        out.append((t, max(0, p - window), min(int(G.lengths[t]), p + aligned + window)))
    return out


def discriminates(G, c, start, end):
    """True iff the bases of the window [start, end) of contig c differ from those a truncated offset would read: at the
    true packed offset minus 2^32 (when it is >= 2^32) and at the true offset mod 2^31."""
    g = int(G.base[c]) + start
    n = end - start
    true = G.seqs[c][start:end]
    for alias in ([g - (1 << 32)] if g >= (1 << 32) else []) + ([g % (1 << 31)] if g >= (1 << 31) else []):
        if np.array_equal(G.packed_window(alias, n), true):
            return False
    return True


def n_per_site(read_len):
    return 48 if read_len <= 512 else 24 if read_len <= 2000 else 16


def site_batch(G, read_len, window, n_per_site, seed=1):
    """The reads of every site that can hold reads of read_len, as one batch, and the site of each record."""
    parts, labels = [], []
    for k, (name, site) in enumerate(sorted(sites(G).items())):
        b = site_reads(G, site, n_per_site, seed + 7919 * k + read_len, read_len, window)
        if b is None:
            continue
        parts.append(b)
        labels += [name] * len(b["pos"])
    return synth.concat(parts), labels
