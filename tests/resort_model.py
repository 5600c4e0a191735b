"""A plain-Python statement of FADEHIP_BAM_KEEP_SORTED (`--keep-sorted`): which records a call writes, in
which order, and which it holds back.  Written from the rule, not from the kernels; tests hold the device to it.

The key of a record is (refID as uint32, pos + 1 as uint32) compared as one 64-bit number, read from the record as it
leaves; a reset record (zero-filled by the clip: build_rec(name, 0, ...)) counts as unmapped and takes KEY_UNMAPPED.  A
call writes, in order of (key as it leaves, stream index), the held-over records and its own whose key as it leaves is not
above W, the key AS IT CAME IN of the call's last record (the last call: everything); the rest is held.  The keys as they
came in must not decrease over the stream."""
import struct

KEY_UNMAPPED = 0xffffffff00000000  # refID -1, pos -1
INF = (1 << 64) - 1


def key(tid, pos):
    return ((tid & 0xffffffff) << 32) | ((pos + 1) & 0xffffffff)


def key_in(rec):
    """The key of a BAM record (bytes, block_size first) as it stands."""
    tid, pos = struct.unpack_from("<ii", rec, 4)
    return key(tid, pos)


def is_reset(rec_in, rec_out):
    """The clip reset the record: it leaves zero-filled (refID, pos, flag, CIGAR and aux gone) and did not come in that way."""
    if rec_out == rec_in:
        return False
    tid, pos, lname, _mapq, _bin, ncig, flag, lseq = struct.unpack_from("<iiBBHHHi", rec_out, 4)
    return (tid, pos, ncig, flag) == (0, 0, 0, 0) and len(rec_out) == 36 + lname + (lseq + 1) // 2 + lseq


def key_out(rec_in, rec_out):
    """The key of a record as it leaves, given what it came in as."""
    return KEY_UNMAPPED if is_reset(rec_in, rec_out) else key_in(rec_out)


class OrderError(Exception):
    """The keys as they came in decrease in front of stream record `index`; `call` is the call that fails."""

    def __init__(self, index, call):
        Exception.__init__(self, "record %d: not in coordinate order" % index)
        self.index, self.call = index, call


def run(calls):
    """calls: per call a list of (key as it came in, key as it leaves, size) per record; the last list is the last call.
    Returns per call dict(emitted=[stream indices in the order written], held=[stream indices held behind the call, in
    the order they will leave], bytes=bytes written, held_bytes=bytes held)."""
    held, res, seq, front = [], [], 0, 0
    size = {}
    for c, recs in enumerate(calls):
        own = []
        for k_in, k_out, sz in recs:
            if k_in < front:
                raise OrderError(seq, c)
            front = k_in
            own.append((k_out, seq))
            size[seq] = sz
            seq += 1
        w = INF if c == len(calls) - 1 else front
        pool = sorted(held + own)
        emitted = [s for k, s in pool if k <= w]
        held = [(k, s) for k, s in pool if k > w]
        res.append(dict(emitted=emitted, held=[s for _, s in held], bytes=sum(size[s] for s in emitted), held_bytes=sum(size[s] for _, s in held)))
    return res


def stable_order(keys_out):
    """The whole stream's order: by (key as it leaves, stream index)."""
    return sorted(range(len(keys_out)), key=lambda i: (keys_out[i], i))
