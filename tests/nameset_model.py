"""A plain-Python statement of the name set (fadehip_nameset_*, FADEHIP_BAM_COLLECT_NAMES / FADEHIP_BAM_EJECT_NAMED, `fade out
--fragments`): the set is the set of (l_read_name, name bytes) of the picked records, and a record is kept exactly when its
name is not in the set.  Written from that sentence, not from the kernels; tests hold the device to it."""
import struct

import tags_model as tm


def rec(name, aux=b""):
    """An unmapped BAM record (block_size first) of that name (bytes, without the NUL) and aux area."""
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, 0, 4, 0, -1, -1, 0) + name + b"\0" + aux
    return struct.pack("<I", len(body)) + body


def key(record):
    """What the set compares: l_read_name and the name bytes (the NUL among them)."""
    ln = record[12]
    return ln, bytes(record[36:36 + ln])


def name_set(records, pick=None):
    return {key(r) for k, r in enumerate(records) if pick is None or pick[k]}


def contains(names, records):
    return [1 if key(r) in names else 0 for r in records]


def keep(names, records):
    return [key(r) not in names for r in records]


def rs_of(record):
    """The rs a record carries as an integer field (its low byte), or None: what the stage kernel reads back."""
    t = tm.read_tags(record, [])
    return t["rs"] if t is not None and t["have"] & 1 else None


def artifact_names(records):
    """COLLECT_NAMES over a file's records: the names of the records with an integer rs and rs & 6."""
    return name_set(records, [1 if (rs_of(r) or 0) & 6 else 0 for r in records])
