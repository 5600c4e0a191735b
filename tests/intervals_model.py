"""The interval set and its overlap query, stated in plain Python from the rule — no sort, no running maximum:
every query looks at every interval of its name.  The tests hold fadehip_intervals_* and the two columns of `fade stats
--repeats` to it.

  interval  (chrom name, start, end), 0-based half-open, 0 <= start < end <= 2^31 - 1; anything else is refused where it enters
  query     (name, qs, qe), qs and qe any integers: it hits iff qs < qe and the set holds an interval of that name — compared
            as exact bytes — with start < qe and qs < end: `bedtools subtract -A`'s "any overlap of at least one base", negated
  a name the set does not hold hits nothing"""

MAX_END = (1 << 31) - 1


class BadInterval(ValueError):
    """interval `index` of an add is outside the bounds; nothing of that add is taken"""

    def __init__(self, index, what):
        ValueError.__init__(self, "interval %d: %s" % (index, what))
        self.index = index


def _b(name):
    return name.encode("latin-1") if isinstance(name, str) else bytes(name)


class IntervalModel:
    def __init__(self, names=()):
        self.names = []
        self.by_name = {}
        for n in names:
            self.name(n)

    def name(self, n):
        n = _b(n)
        if not n or n in self.by_name:
            raise ValueError("a name is empty or comes twice")
        self.by_name[n] = []
        self.names.append(n)

    def add(self, intervals):
        """intervals: (name, start, end) each.  One bad interval: BadInterval with its index, and nothing is added."""
        for k, (n, s, e) in enumerate(intervals):
            if _b(n) not in self.by_name:
                raise BadInterval(k, "the set has no such name")
            if not 0 <= s < e <= MAX_END:
                raise BadInterval(k, "0 <= start < end <= 2^31 - 1 is required")
        for n, s, e in intervals:
            self.by_name[_b(n)].append((s, e))

    def count(self):
        return sum(len(v) for v in self.by_name.values())

    def hit(self, name, qs, qe):
        if not qs < qe:
            return False
        return any(s < qe and qs < e for s, e in self.by_name.get(_b(name), ()))


def rpm_columns(model, row):
    """The two columns a `fade stats` row (bytes, 21 tab-separated columns) gains: read_rpm is the query (rname, art_start,
    art_end) — columns 2, 5, 6 —, art_rpm the query (aln_rname, aln_start, aln_end) — columns 7, 8, 9 —, in the values the row
    prints.  Per row: rows that share (qname, rname, art_start) do not touch each other (the reference scripts' join does)."""
    c = row.split(b"\t")
    assert len(c) == 21, len(c)
    read = model.hit(c[1], int(c[4]), int(c[5]))
    art = model.hit(c[6], int(c[7]), int(c[8]))
    return b"\t%d\t%d" % (read, art)


def bed_text(intervals):
    """the intervals as BED lines"""
    return b"".join(b"%s\t%d\t%d\n" % (_b(n), s, e) for n, s, e in intervals)
