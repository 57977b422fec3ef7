#!/usr/bin/env python3
"""Record tests/golden/halo_loop_bits.json: the SHA-256 of the output buffer (and of the quad-record buffer) of every case that
tests/test_gpu_halo_loop_bits.py holds against it.

Run it ONCE, on an MI355X, with the library of the commit whose bits are the yardstick — the parent of a change that must not move a bit —
never with the code under test:

    DCAMD_LIB=/path/to/parent/libdcamd.so python tools/record_halo_bits.py [OUT.json]

The cases, operands and launches are the test's own (imported from tests/), so recording and checking cannot drift apart."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_halo_loop_bits as B      # noqa: E402
from diffusion_classifier_amd import _lib as L      # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else B.FIXTURE
    digests = {}
    for c in B.HASHED:
        os.environ.pop("DCAMD_HALO_NO_STAG", None)
        os.environ.update(c["env"])
        digests[c["name"]] = B.case_digests(c)
        print(c["name"], digests[c["name"]], flush=True)
    os.environ.pop("DCAMD_HALO_NO_STAG", None)
    doc = {"what": "SHA-256 of the flat output / quad-record buffers of tests/conv_halo_cases.py cases, see tests/test_gpu_halo_loop_bits.py",
           "families": list(B.HASHED_FAMILIES), "library": os.path.basename(L.LIB_PATH), "digests": digests}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} cases -> {out}")


if __name__ == "__main__":
    main()
