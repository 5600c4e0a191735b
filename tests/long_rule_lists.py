"""The inputs of tests/test_gpu_rules_long.py, and what tests/test_long_rule_inputs.py holds them to on the CPU: lists of
pairs for the long-list kernels (sw_forward64_kernel, sw_long_kernel) and for windows of more than one staged chunk, built so
that the rule switches of Appendix A.3 / A.4 decide something in them.  Random long pairs do not: a tie has to be planted.

A list is one sw_batch_packed call (its longest read and widest window choose the runner).  Everything here is
deterministic, selected with the oracle alone, and cached for the session: the oracle's answer for a (list, scoring, rules)
is computed once and shared by every test that needs it."""
import numpy as np

from helpers import IUPAC, concat, embed_seed_pair, end_tie_pair, make_pairs, rand_seq
from test_gpu_rules import DEFAULT, END_MIN_REF, HDIR_F_E, PAD_S, SETTINGS, TIE_EXTENDS

FADE = (10, 2, 2, -3)  # open, ext, match, mismatch
ALL_SETTINGS = [("default", DEFAULT)] + SETTINGS
# other scoring under non-default rules (match <= 2: larger match scores refuse the switches at create); ext = open in the
# second, where opening and extending a gap tie everywhere
RULE_SCORINGS = [(6, 1, 1, -4), (4, 4, 2, -4)]
# other scoring under the default rules on the long list; 14 * 4,096 = 57,344 is the top of the wave64 key's 16 score bits
LONG_SCORINGS = [(6, 1, 1, -4), (5, 1, 8, -4), (1, 1, 14, -1)]
# the switches that change the DP's choices (the others change how a path is written): the lists plant ties for these
A3_A4 = {"end_cell_first_in_row_major_order": END_MIN_REF, "traceback_prefers_E_over_F": HDIR_F_E, "gap_ties_open": TIE_EXTENDS}
A4_NAMES = ("traceback_prefers_E_over_F", "gap_ties_open")

READ_LISTS = {"r12": (513, 768), "r16": (769, 1024), "r24": (1025, 1536), "r32": (1537, 2048), "r48": (2049, 3072),
              "r64": (3073, 4096), "thread": (4097,), "mixed": (513, 4097)}
WINDOW_LISTS = ("chunked", "wave_by_window", "thread_by_window")
LISTS = tuple(READ_LISTS) + WINDOW_LISTS
# what serves the list's long part under rules that sw_forward64_kernel carries, and its rows per lane
RUNNER = {"r12": 12, "r16": 16, "r24": 24, "r32": 32, "r48": 48, "r64": 64, "thread": None, "mixed": None,
          "chunked": None, "wave_by_window": 12, "thread_by_window": None}

_cache = {}


def params(oracle, scoring, rules):
    p = oracle.default_params(rules=rules)
    p.open, p.ext, p.match, p.mismatch = scoring
    return p


def run_oracle(oracle, qs, rs, scoring, rules):
    """[(score, end_query, end_ref, beg_query, beg_ref, n_ops, first min(n_ops, 16) ops)] of the pairs"""
    qc, qo = concat(qs)
    rc, ro = concat(rs)
    res, ops = oracle.sw_batch(qc, qo, rc, ro, threads=8, max_ops=16, params=params(oracle, scoring, rules))
    return [tuple(int(x) for x in res[k]) + (tuple(int(x) for x in ops[k][:min(int(res[k][5]), 16)]),) for k in range(len(qs))]


def gapped(result):
    """an I or a D among the first 16 ops"""
    return any((op & 15) in (1, 2) for op in result[6])


def seeds(oracle, scoring, bit):
    """Short low-complexity pairs whose alignment differs between the default rules and `bit` off, at most 8 ops either way."""
    key = ("seeds", scoring, bit)
    if key not in _cache:
        qs, rs = make_pairs(np.random.default_rng(6000), 6000, kinds=("lowcomplexity",))
        d, f = run_oracle(oracle, qs, rs, scoring, DEFAULT), run_oracle(oracle, qs, rs, scoring, DEFAULT & ~bit)
        _cache[key] = [(qs[k], rs[k]) for k in range(len(qs)) if d[k] != f[k] and d[k][5] <= 8 and f[k][5] <= 8]
    return _cache[key]


def _first_that_differs(oracle, cands, scoring, bit, what):
    qs, rs = [c[0] for c in cands], [c[1] for c in cands]
    d, f = run_oracle(oracle, qs, rs, scoring, DEFAULT), run_oracle(oracle, qs, rs, scoring, DEFAULT & ~bit)
    for k in range(len(cands)):
        if d[k] != f[k]:
            return cands[k]
    raise AssertionError("no input of %d exercises rule bit %d at %s" % (len(cands), bit, what))


def embedded(oracle, rng, scoring, bit, lq, lr=None, col_of=None, n_r=None):
    """One embedded seed of `bit` whose long pair still differs between the two settings (the first such seed, from a start
    that rng draws).  col_of(q_s, r_s) gives the window column of the seed, lr the window's width (default: lq + 60 .. 300)."""
    pool = [s for s in seeds(oracle, scoring, bit) if len(s[0]) + 8 <= lq]
    start = int(rng.integers(0, len(pool)))
    cands = []
    for k in range(min(len(pool), 8)):
        q_s, r_s = pool[(start + k) % len(pool)]
        w = lr
        if w is None:
            w = max(lq + int(rng.integers(60, 301)), lq - len(q_s) + len(r_s) + 60)
        cands.append(embed_seed_pair(rng, q_s, r_s, lq, col=None if col_of is None else col_of(q_s, r_s), lr=w, n_r=n_r))
    return _first_that_differs(oracle, cands, scoring, bit, "%d x %s" % (lq, lr))


def end_tie(oracle, rng, scoring, L, gap, lead=20, tail=20):
    """end_tie_pair whose best score is match * L exactly: the two end cells tie, and Appendix A.3's rule picks one."""
    cands = [end_tie_pair(rng, L, gap, lead, tail) for _ in range(6)]
    res = run_oracle(oracle, [c[0] for c in cands], [c[1] for c in cands], scoring, DEFAULT)
    for c, x in zip(cands, res):
        if x[0] == scoring[2] * L:
            return c
    raise AssertionError("no end-cell tie at L = %d" % L)


def exact_lq(rng, q, lq):
    """make_pairs' related queries come a few bases short or long of what was asked: the list's classes need the length exact"""
    return np.ascontiguousarray(np.concatenate([q, rand_seq(rng, max(0, lq - len(q)))])[:lq])


def n_related(rng, lq, lr):
    """A related pair whose N's and IUPAC letters face each other: the window has 4 % N and 3 % of any IUPAC letter, the query
    is a slice of it with substitutions and two short indels (what EQ_BY_CHAR and N_MATCHES_N decide, inside one long path)."""
    r = rand_seq(rng, lr)
    r[rng.random(lr) < 0.04] = ord("N")
    m = rng.random(lr) < 0.03
    r[m] = rand_seq(rng, int(m.sum()), IUPAC)
    a = int(rng.integers(0, lr - lq - 8))
    q = list(r[a:a + lq + 4])
    del q[lq // 3:lq // 3 + 2]
    q[2 * lq // 3:2 * lq // 3] = list(rand_seq(rng, 2))
    q = np.array(q[:lq], dtype=np.uint8)
    m = rng.random(lq) < 0.02
    q[m] = rand_seq(rng, int(m.sum()))
    return np.ascontiguousarray(q), np.ascontiguousarray(r)


def _family(rng, lq, lr_range):
    qs, rs = [], []
    for kind in ("related", "tandem", "nrich"):
        q, r = make_pairs(rng, 1, lq_range=(lq, lq), lr_range=lr_range, kinds=(kind,))
        qs.append(exact_lq(rng, q[0], lq))
        rs.append(r[0])
    q, r = n_related(rng, lq, int(rng.integers(lr_range[0], lr_range[1] + 1)))
    return qs + [q], rs + [r]


def _read_list(oracle, name, scoring):
    rng = np.random.default_rng(sum(READ_LISTS[name]))
    qs, rs = [], []
    for lq in READ_LISTS[name]:
        for rep in range(2 if len(READ_LISTS[name]) == 1 else 1):  # a list of one length holds everything twice
            even = lq - lq % 2
            pairs = [embedded(oracle, rng, scoring, HDIR_F_E, lq), embedded(oracle, rng, scoring, TIE_EXTENDS, lq),
                     end_tie(oracle, rng, scoring, even // 2, 40 + 10 * rep)]
            fq, fr = _family(rng, lq, (lq + 60, lq + 300))
            qs += [p[0] for p in pairs] + fq
            rs += [p[1] for p in pairs] + fr
    if name == "mixed":  # short pairs in the same call: the class kernels serve them, the long list keeps its runner
        q, r = make_pairs(rng, 20, lq_range=(30, 512), lr_range=(60, 900))
        qs += q
        rs += r
    return qs, rs


def _planted_at_the_end(rng, lq, lr):
    r = rand_seq(rng, lr)
    return r[lr - lq:].copy(), r


def _window_list(oracle, name, scoring):
    """Few seeds are short enough for a 50-base query, and none of them keeps its tie once embedded: the seeds go into the
    150- and 250-base (513-base) queries, the 50-base ones carry the end-cell ties, the planted matches and the families."""
    rng = np.random.default_rng(len(name))
    qs, rs = [], []

    def add(pair):
        qs.append(pair[0])
        rs.append(pair[1])

    def add_family(lq, lr):
        fq, fr = _family(rng, lq, (lr, lr))
        qs.extend(fq)
        rs.extend(fr)
    if name == "chunked":
        turn = 0
        for lr in (2044, 2045, 4100, 8001, 32000):
            # the seed's columns straddle the end of the first and of the second staged chunk, or lie in the last 100
            for c in [None] + [c for c in (2044, 4092) if lr >= c + 60]:
                for bit in (HDIR_F_E, TIE_EXTENDS):
                    lq = (150, 250)[turn % 2]
                    turn += 1
                    if c is None:
                        add(embedded(oracle, rng, scoring, bit, lq, lr, lambda q_s, r_s, lr=lr: lr - 12 - len(r_s), n_r=8))
                    else:
                        add(embedded(oracle, rng, scoring, bit, lq, lr, lambda q_s, r_s, c=c: c - len(r_s) // 2, n_r=8))
            # the two end cells of a tie in different chunks (in the same one at 2,044 / 2,045 columns)
            for L in (25, 75):
                add(end_tie(oracle, rng, scoring, L, lr - 2 * L - 100, lead=60, tail=40))
            add_family((50, 150, 250)[turn % 3], lr)
    else:
        widths, lqs = ((32001, 64990, 65000), (150, 513)) if name == "wave_by_window" else ((65001,), (50, 150))
        for lr in widths:
            for lq in lqs:
                seed_lq = max(lq, 150)
                add(embedded(oracle, rng, scoring, HDIR_F_E, seed_lq, lr, lambda q_s, r_s, lr=lr: lr // 2 + 7 * lq, n_r=8))
                add(_planted_at_the_end(rng, lq, lr))  # an exact match that ends in the last column
                if lq == 513:  # (the thread kernel walks a 513 x 65,000 pair for seconds: two of them per width are enough)
                    continue
                add(embedded(oracle, rng, scoring, TIE_EXTENDS, seed_lq, lr, lambda q_s, r_s, lr=lr: lr - 12 - len(r_s), n_r=8))
                even = lq - lq % 2
                add(end_tie(oracle, rng, scoring, even // 2, lr - even - 100, lead=60, tail=40))
            for lq in lqs[:1 if name == "wave_by_window" else 2]:
                add_family(lq, lr)
    return qs, rs


def pairs(oracle, name, scoring=FADE):
    """(queries, windows) of list `name`, its seeds and end-cell ties selected by the oracle under `scoring`"""
    key = ("pairs", name, scoring)
    if key not in _cache:
        _cache[key] = (_read_list if name in READ_LISTS else _window_list)(oracle, name, scoring)
    return _cache[key]


def short_pairs(oracle, scoring):
    """300 pairs of make_pairs' default families and 300 low-complexity ones, all for the 16-lane kernels, and the seeds of
    the three A.3 / A.4 switches under `scoring` (the 600 alone hold no pair that HDIR_DIAG_F_E decides at 6/1/1/-4)"""
    key = ("short", scoring)
    if key not in _cache:
        rng = np.random.default_rng(300)
        q1, r1 = make_pairs(rng, 300)
        q2, r2 = make_pairs(rng, 300, kinds=("lowcomplexity",))
        extra = [s for bit in (HDIR_F_E, TIE_EXTENDS) for s in seeds(oracle, scoring, bit)[:8]]
        _cache[key] = (q1 + q2 + [s[0] for s in extra], r1 + r2 + [s[1] for s in extra])
    return _cache[key]


def full_length_match(lq, seed=1):
    """the whole query matches the window: the score is match * lq, the top of what the list's kernel has to hold"""
    r = rand_seq(np.random.default_rng(seed + lq), lq + 120)
    return r[60:60 + lq].copy(), r


def expected(oracle, tag, qs, rs, scoring, rules):
    """the oracle's results for the pairs, computed once per (tag, scoring, rules); tag names the pairs"""
    key = ("expected", tag, scoring, rules)
    if key not in _cache:
        _cache[key] = run_oracle(oracle, qs, rs, scoring, rules)
    return _cache[key]



# Level 2: soft-clipped reads whose clips carry a planted window with an indel, so that gapped am tags come out.  The runner
# is the one the batch takes under rules that sw_forward64_kernel carries (its rows per lane, None for the thread kernel);
# `gapped` is the least number of am tags with an I or a D that the oracle has to give under every setting.
LEVEL2 = {
    "600_bases": dict(n_reads=160, read_len=600, window=120, runner=12, gapped=8),
    "4097_bases": dict(n_reads=24, read_len=4097, window=120, runner=None, gapped=2),
    # windows of ~34,150 columns, fewer where a contig ends: those stay with the 16-lane kernels
    "150_bases_w17000": dict(n_reads=120, read_len=150, window=17000, runner=12, gapped=8, also_short=True),
}
FLOOR_LEN = 5


def level2_batch(name):
    """(contig names, contigs as str, the batch) of LEVEL2[name]"""
    key = ("batch", name)
    if key not in _cache:
        from fade_amd import synth
        cfg = LEVEL2[name]
        g = synth.Genome(2, 60_000, 17)
        b = synth.make_reads(g, cfg["n_reads"], 41, read_len=cfg["read_len"], window=cfg["window"], p_sc=1.0, p_planted=1.0,
                             p_clip_indel=0.8, clip_min=20, clip_max=120, insert_mu=cfg["read_len"] + 200)
        b.pop("_truth", None)
        _cache[key] = (g.names, [a.tobytes().decode() for a in g.ascii_contigs()], b)
    return _cache[key]


def level2_expected(oracle, name, rules):
    """(rs, am) of the oracle for the batch under `rules`"""
    key = ("level2", name, rules)
    if key not in _cache:
        names, seqs, b = level2_batch(name)
        _cache[key] = oracle.annotate_batch_soa(oracle.GenomeHolder(names, seqs), b, FLOOR_LEN, LEVEL2[name]["window"], threads=8,
                                                params=oracle.default_params(rules=rules))
    return _cache[key]


def gapped_am(am):
    """am tags whose CIGARs hold an I or a D (an am tag is 'contig,pos,cigar' per clip, ';' between the two clips)"""
    return sum(1 for a in am if a is not None and any(ch in f.split(",")[-1] for f in a.split(";") if f for ch in "ID"))
