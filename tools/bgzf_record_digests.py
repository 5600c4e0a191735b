"""Records tests/golden/bgzf_device_digests.json for tests/test_gpu_bgzf_pinned.py: the SHA-256 and length of the device
compressor's stream for every case of that file's build_cases, in both block geometries, on a GPU.

    FADEHIP_LIB=<libfadehip.so of the commit to pin to> python tools/bgzf_record_digests.py <that commit's hash> <out.json>

The library is the one to pin TO (the parent of a refactor), never the code under test, so FADEHIP_LIB must be given.
Every case is compressed three times in a context of its own geometry; a case whose three streams differ is not written
and the run fails."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if len(sys.argv) != 3 or not os.environ.get("FADEHIP_LIB"):
    sys.exit(__doc__)
commit, out_path = sys.argv[1], sys.argv[2]

import fade_amd  # noqa: E402
from test_gpu_bgzf_pinned import build_cases, sha256  # noqa: E402

doc = {"recorded_from": commit, "cases": {}}
unstable = []
for geom in (64, 32):
    os.environ["FADEHIP_BGZF_GEOM"] = str(geom)  # (read when a context compresses for the first time)
    c = fade_amd.Context(device=0)
    rows = doc["cases"][str(geom)] = {}
    for name, data in build_cases(geom).items():
        outs = [bytes(c.bgzf_deflate(data)) for _ in range(3)]
        if outs[1] != outs[0] or outs[2] != outs[0]:
            unstable.append((geom, name))
            continue
        rows[name] = {"input_length": len(data), "input_sha256": sha256(data), "length": len(outs[0]), "sha256": sha256(outs[0])}
    c.close()
if unstable:
    sys.exit("not stable across three runs, nothing written: %r" % unstable)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("recorded %d + %d cases from %s" % (len(doc["cases"]["64"]), len(doc["cases"]["32"]), commit))
