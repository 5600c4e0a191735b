"""The record store's rule (fadehip_recstore_*, `fade extract --sorted`, `fade annotate --extract-sorted`) in plain Python:
the arbiter of tests/test_gpu_recstore.py and tests/test_gpu_cli_extract_sorted.py.  Nothing here runs the code under test.

  key      (refID as uint32) << 32 | (pos + 1 as uint32), from the record's own bytes: refID -1 sorts last, and on one
           reference pos -1 sorts first
  order    by key; records of one key keep the order in which they were added (a stable sort)
  drain    from record j0 of the final order: the longest run whose bytes total at most max_payload — one record when even
           the first is larger; a record is never split
  @HD      the header text of the sorted file: SO:coordinate on the @HD line (an SO: value replaced, a line without one gains
           the field, a text without the line gains "@HD VN:1.6 SO:coordinate" in front)
"""
import struct


def split(payload):
    """BAM records back to back (block_size first) -> the records' bytes."""
    out, at = [], 0
    while at < len(payload):
        n = 4 + struct.unpack_from("<I", payload, at)[0]
        out.append(bytes(payload[at:at + n]))
        at += n
    assert at == len(payload)
    return out


def key(rec):
    tid, pos = struct.unpack_from("<ii", rec, 4)
    return ((tid & 0xffffffff) << 32) | ((pos + 1) & 0xffffffff)


def order(records):
    """The records in final order."""
    return sorted(records, key=key)   # (sorted is stable)


def drain_cut(sizes, j0, max_payload):
    """Records j0 .. the returned index - 1 leave with the drain that begins at j0 < len(sizes)."""
    j, total = j0, 0
    while j < len(sizes) and total + sizes[j] <= max_payload:
        total += sizes[j]
        j += 1
    return max(j, j0 + 1)


def drains(records, max_payload):
    """The final order cut into drains: a list of lists of records."""
    recs = order(records)
    sizes = [len(r) for r in recs]
    out, j = [], 0
    while j < len(recs):
        e = drain_cut(sizes, j, max_payload)
        out.append(recs[j:e])
        j = e
    return out


def header_sorted(text):
    """The header text (str) with SO:coordinate on its @HD line."""
    so = "SO:coordinate"
    lines = text.split("\n")
    if not (lines[0] == "@HD" or lines[0].startswith("@HD\t")):
        return "@HD\tVN:1.6\t" + so + "\n" + text
    fields = [f for f in lines[0].split("\t")]
    if any(f.startswith("SO:") for f in fields):
        k = next(i for i, f in enumerate(fields) if f.startswith("SO:"))
        fields = fields[:k] + [so] + [f for f in fields[k + 1:] if not f.startswith("SO:")]
    else:
        fields.append(so)
    return "\n".join(["\t".join(fields)] + lines[1:])
