"""Writes tests/golden/net_site_trace.json: the snapshots of tests/net_site_trace.py's walks, taken from the library as it is built in this
tree. Run ONCE on a GPU at the commit whose behaviour is to be pinned (it was: the parent of the commit that introduced net_resolve); the
file is then committed unchanged and tests/test_gpu_net_sites.py compares every later tree with it.

    python scripts/record_net_site_trace.py [output.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from anakin_amd import lib as L  # noqa: E402
from tests import net_site_trace as NT  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else NT.GOLDEN
    L.require_device()
    enc = {}
    for name in sorted(NT.WALKS):
        steps = NT.WALKS[name]()
        assert NT.decode(NT.encode(steps)) == steps, name
        enc[name] = NT.encode(steps)
        print("%s: %d steps" % (name, len(steps)))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(enc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
