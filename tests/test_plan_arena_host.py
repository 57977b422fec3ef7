"""CPU: the arena offset assignment of the launch plans (plan.assign_arena) — the piece that decides which activations share memory.
Generated liveness patterns are held to the properties an arena must have (a hard condition: no two live tensors overlap); hand cases
pin the policy (best fit, split, coalesce, free after the op) to offsets worked out by hand."""
import random

import numpy as np
import pytest

from diffusion_classifier_amd.plan import assign_arena

SEEDS = range(2000)
_CACHE = {}


class Base:
    def __init__(self, first, last, nbytes):
        self.first, self.last, self.nbytes, self.off = first, last, nbytes, None


def generate(seed):
    """1-60 ops, 1-80 tensors; first uniform over the ops; last == first or uniform in [first, nops] (nops: kept to the end); sizes
    multiples of 256 up to 40 x 256."""
    rng = random.Random(seed)
    nops = rng.randint(1, 60)
    bases = []
    for _ in range(rng.randint(1, 80)):
        first = rng.randrange(nops)
        last = first if rng.random() < 0.5 else rng.randint(first, nops)
        bases.append(Base(first, last, 256 * rng.randint(1, 40)))
    return bases, nops


def solved():
    """seed -> (first, last, nbytes, off as int64 arrays, nops, arena size), computed once for the tests below."""
    if not _CACHE:
        for seed in SEEDS:
            bases, nops = generate(seed)
            top = assign_arena(bases, nops)
            assert all(b.off is not None for b in bases), seed
            _CACHE[seed] = tuple(np.array([getattr(b, k) for b in bases], dtype=np.int64) for k in ("first", "last", "nbytes", "off")) + (nops, top)
    return _CACHE


def test_every_offset_is_set_aligned_and_inside_the_arena():
    for seed, (first, last, nbytes, off, nops, top) in solved().items():
        assert (off >= 0).all() and (off % 256 == 0).all() and (off + nbytes <= top).all(), seed


def test_tensors_live_at_the_same_time_never_share_a_byte():
    for seed, (first, last, nbytes, off, nops, top) in solved().items():
        live = (first[:, None] <= last[None, :]) & (first[None, :] <= last[:, None])
        share = (off[:, None] < (off + nbytes)[None, :]) & (off[None, :] < (off + nbytes)[:, None])
        np.fill_diagonal(live, False)
        bad = np.argwhere(live & share)
        assert bad.size == 0, (seed, bad[:4].tolist())


def test_the_arena_holds_the_peak_of_live_bytes():
    for seed, (first, last, nbytes, off, nops, top) in solved().items():
        idx = np.arange(nops + 1)[:, None]
        peak = (((first[None, :] <= idx) & (idx <= last[None, :])) * nbytes[None, :]).sum(1).max()
        assert top >= peak, (seed, top, peak)


def test_the_same_input_gives_the_same_offsets():
    for seed, (first, last, nbytes, off, nops, top) in solved().items():
        bases, nops2 = generate(seed)                       # a fresh copy of the same input
        assert nops2 == nops and assign_arena(bases, nops) == top and [b.off for b in bases] == off.tolist(), seed
        assert assign_arena(bases, nops) == top and [b.off for b in bases] == off.tolist(), seed      # offsets already set: no matter


# (first, last, nbytes) per tensor in the order given, the op count, the expected offsets and arena size
HAND = {
    # C is as large as the hole A left after op 0 and takes it
    "an exactly fitting hole is reused": ([(0, 0, 512), (0, 2, 256), (1, 2, 512)], 3, [0, 512, 0], 768),
    # holes of 1024 at 0 and of 512 at 1280 after op 0: E (512) takes the smaller one that fits, not the first
    "best fit among two holes": ([(0, 0, 1024), (0, 3, 256), (0, 0, 512), (0, 3, 256), (1, 3, 512)], 4, [0, 1024, 1280, 1792, 1280], 2048),
    # the hole of 1024 takes C (256) at its start, its remainder takes D (512) right behind
    "a larger hole is split": ([(0, 0, 1024), (0, 2, 256), (1, 2, 256), (1, 2, 512)], 3, [0, 1024, 0, 256], 1280),
    # A freed after op 0 and B after op 1 are neighbours: together they hold D (512), which neither does alone
    "neighbouring holes coalesce": ([(0, 0, 256), (0, 1, 256), (0, 3, 256), (2, 3, 512)], 4, [0, 256, 512, 0], 768),
    # A is written and dead within op 0: B, first used by the same op, must not take its place; C, at op 1, may
    "first == last is freed only after its op": ([(0, 0, 512), (0, 1, 256), (1, 1, 512)], 2, [0, 512, 0], 768),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(name):
    spec, nops, offs, top = HAND[name]
    bases = [Base(*t) for t in spec]
    assert assign_arena(bases, nops) == top
    assert [b.off for b in bases] == offs
