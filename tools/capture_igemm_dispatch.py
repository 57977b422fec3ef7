"""Record dc_igemm's dispatch table (tests/golden/igemm_dispatch.npz) from the library built in this tree.

The cases, the sweep and the encoding live in tests/test_igemm_dispatch.py; this tool only runs them and writes the file.  Everything it
calls runs on the host (dc_igemm_variant, the dc_igemm_*_ok probes, dc_igemm on refused problems): no GPU is needed.  Run it on a build
of the commit whose behaviour is to be pinned — before a change to csrc/igemm.hip's dispatcher, not after — in an environment without
DCAMD_* switches:

    python tools/capture_igemm_dispatch.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_igemm_dispatch as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    tables = T.capture()
    np.savez_compressed(out, **T.encode(tables))
    d = tables["default"]
    print(f"{out}: {os.path.getsize(out)} bytes, {len(d['variant'])} + {len(T.ENVS) - 1} x {len(tables[T.ENVS[1][0]]['variant'])} cases, "
          f"{len({v for t in tables.values() for v in t['variant']})} variants")
