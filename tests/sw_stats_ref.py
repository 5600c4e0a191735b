"""Restatement of parasail's stats-mode local alignment (tests/sw_stats_ref.c), built into a temporary directory.

stats(q, r, scoring, rules) -> dict for one pair; stats_batch(qs, rs, scoring, rules) -> structured array in the layout
of fade_amd.api.SW_STATS_DTYPE.  Compiled once per process with the system C compiler."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sw_stats_ref.c")
RULES_DEFAULT = 0x7f
SCORING_STATS = (3, 8, 10, -5)  # stats.d:87 Parasail("ACTGN", 3, 8, 10, -5)
DTYPE = np.dtype([("score", "<i4"), ("end_query", "<i4"), ("end_ref", "<i4"), ("matches", "<i4"), ("similar", "<i4"),
                  ("length", "<i4")])

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is not None:
        return _lib
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    if not cc:
        raise RuntimeError("no C compiler to build %s" % SRC)
    _dir = tempfile.mkdtemp(prefix="sw_stats_ref_")
    so = os.path.join(_dir, "libsw_stats_ref.so")
    subprocess.check_call([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.stats_ref_batch.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.stats_ref_batch.restype = C.c_int
    _lib = L
    return L


def _concat(strs):
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in strs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    buf = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8)
    return buf, off


def stats_batch(qs, rs, scoring=SCORING_STATS, rules=RULES_DEFAULT):
    assert len(qs) == len(rs)
    L = lib()
    qb, qo = _concat(qs)
    rb, ro = _concat(rs)
    sc = np.asarray(scoring, dtype=np.int32)
    out = np.zeros(len(qs), dtype=DTYPE)
    rc = L.stats_ref_batch(sc.ctypes.data, rules, len(qs), qb.ctypes.data, qo.ctypes.data, rb.ctypes.data, ro.ctypes.data,
                           out.ctypes.data)
    if rc:
        raise MemoryError("stats_ref_batch failed")
    return out


def stats(q, r, scoring=SCORING_STATS, rules=RULES_DEFAULT):
    o = stats_batch([q], [r], scoring, rules)[0]
    return {k: int(o[k]) for k in DTYPE.names}
