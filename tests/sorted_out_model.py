"""The rule of the coordinate-sorted main output (FADEHIP_BAM_STORE_OUTPUT, fadehip_recstore_measure / _set_window / _reset;
DESIGN.md 3.8n) in plain Python: the arbiter of tests/test_gpu_sorted_out.py.  Nothing here runs the code under test.

  records  exactly those the same stream writes without the flag, byte for byte per record
  order    stable by the key of the record AS IT LEAVES — recstore_model.key of the written record: a clipped record is
           keyed at its new pos, refID -1 sorts last — but for a RESET record, which is written zero-filled (refID 0, pos 0:
           DESIGN.md 3.8h) and keyed RS_KEY_UNMAPPED: it leaves at the end, as under --keep-sorted.  The written bytes do not
           say which record is a reset one; the caller does (`reset`, one flag per written record)
  buckets  SHIFT = 16; reference r has nb[r] = ((len[r] + 1) >> SHIFT) + 1 buckets from first[r] (their prefix sums); one more
           bucket, the last, holds refID -1 and every refID outside the header.
           bucket(key) = first[r] + min(uint32(key) >> SHIFT, nb[r] - 1): monotone in the key and total, a pos beyond the
           contig in the contig's last bucket.  A bucket's key range is inclusive; the last bucket's ends at all ones
  cost     cost(b bytes, n records) = b + 64 n
  windows  runs of consecutive buckets of cost <= budget, chosen greedily front to back; a bucket that holds nothing joins
           the window it lies in; a single bucket above the budget is an error that names it
"""
import recstore_model as rm

SHIFT = 16
ITEM_COST = 64
KEY_UNMAPPED = 0xffffffff00000000
ALL = (1 << 64) - 1

split = rm.split


def key(rec, reset=False):
    """The key a written record leaves with."""
    return KEY_UNMAPPED if reset else rm.key(rec)


def _flags(records, reset):
    reset = [False] * len(records) if reset is None else list(reset)
    assert len(reset) == len(records)
    return reset


def order(records, reset=None):
    """The written records in final order."""
    reset = _flags(records, reset)
    return [records[k] for k in sorted(range(len(records)), key=lambda k: key(records[k], reset[k]))]   # (sorted is stable)


def layout(ref_len):
    """(first, nb, n_buckets)"""
    nb = [((n + 1) >> SHIFT) + 1 for n in ref_len]
    first, at = [], 0
    for n in nb:
        first.append(at)
        at += n
    return first, nb, at + 1


def bucket(ref_len, k):
    first, nb, n = layout(ref_len)
    r = k >> 32
    if r >= len(ref_len):
        return n - 1
    return first[r] + min((k & 0xffffffff) >> SHIFT, nb[r] - 1)


def bucket_range(ref_len, b):
    """(lo, hi, ref) — both ends inclusive; ref -1 for the last bucket."""
    first, nb, n = layout(ref_len)
    assert 0 <= b < n
    if b == n - 1:
        return len(ref_len) << 32, ALL, -1
    r = max(r for r in range(len(ref_len)) if first[r] <= b)
    j = b - first[r]
    hi = 0xffffffff if j + 1 == nb[r] else ((j + 1) << SHIFT) - 1
    return (r << 32) | (j << SHIFT), (r << 32) | hi, r


def histogram(ref_len, records, reset=None):
    """(bytes per bucket, records per bucket) of written records."""
    n = layout(ref_len)[2]
    nbytes, nrec = [0] * n, [0] * n
    for rec, rst in zip(records, _flags(records, reset)):
        b = bucket(ref_len, key(rec, rst))
        nbytes[b] += len(rec)
        nrec[b] += 1
    return nbytes, nrec


def cost(nbytes, nrec):
    return nbytes + ITEM_COST * nrec


class BucketOverBudget(Exception):
    def __init__(self, b):
        Exception.__init__(self, "bucket %d alone is over the budget" % b)
        self.bucket = b


def windows(nbytes, nrec, budget):
    """[(b0, b1)]: buckets b0 .. b1 - 1 per window; together they cover every bucket."""
    out, b0, have = [], 0, 0
    for b in range(len(nbytes)):
        c = cost(nbytes[b], nrec[b])
        if c > budget:
            raise BucketOverBudget(b)
        if have + c > budget:
            out.append((b0, b))
            b0, have = b, 0
        have += c
    out.append((b0, len(nbytes)))
    return out


def window_keys(ref_len, w):
    """(lo, hi) inclusive of the window (b0, b1)."""
    return bucket_range(ref_len, w[0])[0], bucket_range(ref_len, w[1] - 1)[1]


def in_windows(ref_len, records, budget, reset=None):
    """The written records as the window loop yields them: per window its records in final order."""
    reset = _flags(records, reset)
    ws = windows(*histogram(ref_len, records, reset), budget)
    out = []
    for w in ws:
        lo, hi = window_keys(ref_len, w)
        keep = [k for k in range(len(records)) if lo <= key(records[k], reset[k]) <= hi]
        out.append(order([records[k] for k in keep], [reset[k] for k in keep]))
    return out
