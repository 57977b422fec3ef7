"""CPU: the host arithmetic of the scoring path (scoring.py) — the control-block layout, the launch-size rule, the index part of a
stage's control blocks against the per-unit loop the GPU tests hold the kernels to (helpers.expected_unit_maps), and the eps runs."""
import pytest
import torch

from diffusion_classifier_amd import dist as D
from diffusion_classifier_amd import scoring as SC
from helpers import expected_unit_maps

WORLDS = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]


# ------------------------------------------------------------------------------------------------ ControlBlock
@pytest.mark.parametrize("n_bj,k", [(1, 1), (7, 2), (7, 3), (200, 5)])
def test_control_block_fields_tile_the_block(n_bj, k):
    lay = SC.ControlBlock(n_bj, k)
    assert lay.U == n_bj * k and lay.host_words == 6 * n_bj and lay.words == 6 * n_bj + 2 * n_bj * k
    assert list(lay.fields) == ["pair_id", "lam", "alpha", "sigma", "img_of_bj", "ctx_of_unit", "out_index"]
    at = 0
    for name, (sl, dt) in lay.fields.items():                  # in the order of the block: no gap, no overlap
        assert sl.start == at and sl.stop > sl.start and sl.step is None, name
        at = sl.stop
    assert at == lay.words
    assert lay.fields["pair_id"][0].start == 0                 # its int64 view is 8-byte aligned
    assert lay.fields["img_of_bj"][0].stop == lay.host_words == lay.fields["ctx_of_unit"][0].start
    sizes = {name: sl.stop - sl.start for name, (sl, _) in lay.fields.items()}
    assert sizes == dict(pair_id=2 * n_bj, lam=n_bj, alpha=n_bj, sigma=n_bj, img_of_bj=n_bj, ctx_of_unit=lay.U, out_index=lay.U)
    dts = {name: dt for name, (_, dt) in lay.fields.items()}
    assert dts == dict(pair_id=torch.int64, lam=torch.float32, alpha=torch.float32, sigma=torch.float32, img_of_bj=torch.int32,
                       ctx_of_unit=torch.int32, out_index=torch.int32)
    block = torch.arange(lay.words, dtype=torch.int32)
    assert lay.view(block, "pair_id").shape == (n_bj,) and lay.view(block, "pair_id").dtype == torch.int64
    assert lay.view(block, "lam").dtype == torch.float32 and lay.view(block, "out_index").tolist() == list(range(lay.words - lay.U, lay.words))
    assert lay.view(block, "img_of_bj").data_ptr() == block.data_ptr() + 4 * 5 * n_bj            # views, not copies


# ------------------------------------------------------------------------------------------------ launch_size
@pytest.mark.parametrize("n_pairs,cap,subset,want", [(800, 256, False, 200), (21, 256, True, 32), (3, 256, True, 8), (3, 4, True, 4),
                                                     (300, 256, True, 256), (1, 1, True, 1), (5, 256, False, 5)])
def test_launch_size_pinned_values(n_pairs, cap, subset, want):
    assert SC.launch_size(n_pairs, cap, subset) == want


@pytest.mark.parametrize("cap", [1, 4, 5, 64, 256])
def test_launch_size_properties(cap):
    rungs = set()
    for n in range(1, 601):
        a, b = SC.launch_size(n, cap, False), SC.launch_size(n, cap, True)
        assert 1 <= a <= cap and 1 <= b <= cap
        n_mb = -(-n // a)
        assert n_mb * a - n < n_mb, (n, cap, a)                # no micro-batch padded by a whole slot more than evenness needs
        rungs.add(b)
    assert len(rungs) <= 6, rungs                              # a plan size per rung: the default score_plan_cache holds them


# ------------------------------------------------------------------------------------------------ index_blocks
def _check_blocks(pairs, keep, n_bj, ncls, T, dump, padded):
    k = keep.shape[1]
    lay = SC.ControlBlock(n_bj, k)
    n_mb = -(-len(pairs) // n_bj)
    assert (n_mb * n_bj > len(pairs)) == padded
    tmpl, jsb = SC.index_blocks(lay, pairs, keep, ncls, T, dump)
    assert tmpl.shape == (n_mb, lay.words) and tmpl.dtype == torch.int32 and len(jsb) == n_mb
    cl, oi = expected_unit_maps(pairs, keep.tolist(), n_bj, ncls, T, dump)
    bare, jsb0 = SC.index_blocks(lay, pairs, None, ncls, T, dump)       # classes on the device: the maps are not the host's
    for m in range(n_mb):
        chunk = pairs[m * n_bj:(m + 1) * n_bj]
        slots = chunk + [chunk[0]] * (n_bj - len(chunk))                # a slot past the last pair repeats the chunk's first pair
        js, bs = jsb[m]
        assert js.tolist() == [p[0] for p in slots] and bs.tolist() == [p[1] for p in slots]
        assert lay.view(tmpl[m], "pair_id").tolist() == [b * T + j for j, b in slots]
        assert lay.view(tmpl[m], "img_of_bj").tolist() == [b for _, b in slots]
        for f in ("lam", "alpha", "sigma"):                             # filled per call from the t draws
            assert not tmpl[m][lay.fields[f][0]].any()
        assert torch.equal(lay.view(tmpl[m], "ctx_of_unit").long(), cl[m]) and torch.equal(lay.view(tmpl[m], "out_index").long(), oi[m])
        assert torch.equal(bare[m, :lay.host_words], tmpl[m, :lay.host_words]) and not bare[m, lay.host_words:].any()
        assert torch.equal(jsb0[m][0], js) and torch.equal(jsb0[m][1], bs)
    if padded:
        assert (oi[-1, (len(pairs) - (n_mb - 1) * n_bj) * k:] == dump).all() and int(oi.max()) == dump
    else:
        assert int(oi.max()) < dump


@pytest.mark.parametrize("world,rank", WORLDS)
def test_index_blocks_over_all_images(world, rank):
    BS, Cn, T, k, t0, t1, n_bj = 5, 9, 12, 3, 4, 12, 7
    torch.manual_seed(43)
    keep = torch.stack([torch.randperm(Cn)[:k] for _ in range(BS)]).to(torch.int32)
    pairs = D.local_pairs(t0, t1, BS, rank, world)
    # every case has a padded tail but rank 0 of 3, whose 14 pairs are two full micro-batches
    _check_blocks(pairs, keep, n_bj, Cn, T, BS * Cn * T, padded=(world, rank) != (3, 0))


@pytest.mark.parametrize("world,rank", WORLDS)
def test_index_blocks_over_an_image_subset(world, rank):
    BS, Cn, T, k, t0, t1, n_bj = 5, 9, 12, 2, 4, 12, 7
    torch.manual_seed(43)
    keep = torch.stack([torch.randperm(Cn)[:k] for _ in range(BS)]).to(torch.int32)
    pairs = D.local_pairs_rows(t0, t1, [1, 3, 4], rank, world)
    _check_blocks(pairs, keep, n_bj, Cn, T, BS * Cn * T, padded=True)


def test_index_blocks_single_slot_and_exact_fit():
    BS, Cn, T = 5, 9, 12
    keep1 = torch.tensor([[4], [0], [8], [2], [7]], dtype=torch.int32)
    _check_blocks(D.local_pairs(4, 6, BS, 0, 1), keep1, 1, Cn, T, BS * Cn * T, padded=False)        # k = 1, n_bj = 1: a block per pair
    torch.manual_seed(44)
    keep = torch.stack([torch.randperm(Cn)[:3] for _ in range(BS)]).to(torch.int32)
    pairs = D.local_pairs(0, 2, BS, 0, 1)
    _check_blocks(pairs, keep, len(pairs), Cn, T, BS * Cn * T, padded=False)                       # len(pairs) == n_bj: one block, no padding


# ------------------------------------------------------------------------------------------------ eps_runs
@pytest.mark.parametrize("world", [1, 2, 3])
def test_eps_runs_cover_the_chunk_with_consecutive_images_of_one_trial(world):
    seen = set()
    for rank in range(world):
        pairs = D.local_pairs(0, 3, 5, rank, world)
        for n_bj in (4, len(pairs)):
            for m in range(-(-len(pairs) // n_bj)):
                chunk = pairs[m * n_bj:(m + 1) * n_bj]
                runs = SC.eps_runs(chunk)
                back = []
                for r, j, b0, n in runs:
                    assert r == len(back) and n >= 1
                    back += [(j, b0 + i) for i in range(n)]             # one trial, consecutive images
                assert back == chunk
                seen.add(max(n for _, _, _, n in runs))
    assert (max(seen) == 5) == (world == 1)                             # a whole trial's images in one copy only when one rank owns them all
    assert SC.eps_runs([]) == []
