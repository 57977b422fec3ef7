"""GPU: the lock-step tap loop of conv3_halo.hip (mma_tap: software-pipelined fragment reads) must not move a single output bit.

One accumulator gets one MFMA per tap, taps in the same order, whatever the order and depth of the fragment reads — so three checks, none
of which needs a tolerance:

  parent hashes   every case of the families halo4, halo8_lockstep, up4 and thin of tests/conv_halo_cases.py, all three dtypes: the SHA-256
                  of the whole output buffer (sentinel pads and guard region included) and of the quad-record buffer where the case has
                  one equal tests/golden/halo_loop_bits.json, recorded by tools/record_halo_bits.py from the library of the commit
                  BEFORE the loop was rewritten (never from the code under test).
  cross-loop      every halo8 case: the lock-step loop (DCAMD_HALO_NO_STAG=1) and the staggered loop, which the rewrite does not
                  touch, give the same bytes on the same operands (the kernel header promises it).
  determinism     a second launch of every REPEAT_CASES entry gives the same bytes.

The cases are the small shapes at which the loop can go wrong (32x32 and 64x64 images over several tiles, 16x16 single-tile, 8x8 with
n = 11, the 4x4 mosaic with n = 40, two and more channel chunks, a side source of two and more chunks, two N tiles, ragged n_img); the
operands, the NaN-embedded allocations and the launch are those of tests/test_gpu_conv_halo.py."""
import hashlib
import json
import os

import pytest
import torch

import conv_halo_cases as G
import test_gpu_conv_halo as H

pytestmark = pytest.mark.gpu
DEV = H.DEV
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "halo_loop_bits.json")
HASHED_FAMILIES = ("halo4", "halo8_lockstep", "up4", "thin")
HASHED = [c for c in G.CASES if c["family"] in HASHED_FAMILIES]
HALO8 = [c for c in G.CASES if c["family"] == "halo8"]


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(c, ptrs):
    """One launch into fresh sentinel-filled buffers -> {"out": sha, "qstats": sha (cases with quad records)}."""
    out = G.new_output(c, DEV)
    qs = G.new_qstats(c, DEV) if "qstats" in c["use"] else None
    H.launch(c, ptrs, out, qs)
    torch.cuda.synchronize()
    d = {"out": sha(out)}
    if qs is not None:
        d["qstats"] = sha(qs)
    return d


def case_digests(c):
    """The digests of a case under its own environment (the caller has set it)."""
    ptrs, keep = H.device_operands(c, G.make_operands(c))
    return run_case(c, ptrs)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


def test_fixture_covers_every_hashed_case(recorded):
    assert sorted(recorded) == sorted(c["name"] for c in HASHED)
    for c in HASHED:
        assert sorted(recorded[c["name"]]) == (["out", "qstats"] if "qstats" in c["use"] else ["out"]), c["name"]


@pytest.mark.parametrize("c", HASHED, ids=lambda c: c["name"])
def test_output_bits_equal_the_parent_commit(c, recorded, monkeypatch):
    H.set_env(c, monkeypatch)
    got = case_digests(c)
    print(f"{c['name']} [{c['family']}] {c['instance']}: {got}")
    assert got == recorded[c["name"]], (c["name"], c["instance"])


@pytest.mark.parametrize("c", HALO8, ids=lambda c: c["name"])
def test_lockstep_loop_equals_staggered_loop(c, monkeypatch):
    ptrs, keep = H.device_operands(c, G.make_operands(c))
    monkeypatch.delenv("DCAMD_HALO_NO_STAG", raising=False)
    stag = run_case(c, ptrs)
    monkeypatch.setenv("DCAMD_HALO_NO_STAG", "1")
    lock = run_case(c, ptrs)
    print(f"{c['name']}: staggered {stag} lock-step {lock}")
    assert lock == stag, c["name"]


@pytest.mark.parametrize("name", G.REPEAT_CASES)
def test_second_launch_gives_the_same_bytes(name, monkeypatch):
    c = G.by_name(name)
    H.set_env(c, monkeypatch)
    ptrs, keep = H.device_operands(c, G.make_operands(c))
    first = run_case(c, ptrs)
    torch.randn(1 << 20, device=DEV).sum()
    assert run_case(c, ptrs) == first, name
