"""Host: the index maps of the tail fold (csrc/epi_pn.h pn_tail_finish, csrc/conv3_halo.h pn_tail_ring_slot, csrc/elementwise.hip
pn_tail_combine_kernel) and the Wt packing (engine.pack_tail) replayed in numpy on the three geometries the GPU tests use, against
F.conv2d: z = Wt . y per tile, shift-and-add over the nine taps, own pixels + bias into pred, the surround into the tile's ring slots,
then the border pixels collect their neighbours' slots in ascending tile order.  Ring and pred start as NaN, so a slot that is read
without having been written, or a pixel nobody writes, shows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import engine as E


def ring_slot(oy, ox, tw, th):
    if oy < 0:
        return ox + 1
    if oy >= th:
        return tw + 2 + ox + 1
    return 2 * (tw + 2) + (0 if ox < 0 else th) + oy


def geometry(H, W):
    tw = min(W, 32)
    th = min(256 // tw, H)
    return tw, th, W // tw, H // th


def fold(y, Wt, bias, Co):
    """y [n, H, W, 128] -> (pred, ring) as the conv kernel leaves them."""
    n, H, W, _ = y.shape
    tw, th, tiles_x, tiles_y = geometry(H, W)
    R = 2 * (tw + 2) + 2 * th
    pred = np.full((n, H, W, Co), np.nan, np.float32)
    ring = np.full((n, tiles_x * tiles_y, R, Co), np.nan, np.float32)
    for s in range(n):
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                tile = y[s, ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].reshape(th * tw, -1)      # pixel p = py * tw + px
                z = Wt.astype(np.float64) @ tile.T.astype(np.float64)                               # [32, 256]
                for oy in range(-1, th + 1):
                    for ox in range(-1, tw + 1):
                        gy, gx = ty * th + oy, tx * tw + ox
                        if not (0 <= gy < H and 0 <= gx < W):
                            continue
                        acc = np.zeros(Co)
                        for tap in range(9):
                            py, px = oy + tap // 3 - 1, ox + tap % 3 - 1
                            if 0 <= py < th and 0 <= px < tw:
                                acc += z[tap * Co:(tap + 1) * Co, py * tw + px]
                        if 0 <= oy < th and 0 <= ox < tw:
                            pred[s, gy, gx] = acc + bias
                        else:
                            ring[s, ty * tiles_x + tx, ring_slot(oy, ox, tw, th)] = acc
    return pred, ring


def combine(pred, ring):
    n, H, W, Co = pred.shape
    tw, th, tiles_x, tiles_y = geometry(H, W)
    if tiles_x * tiles_y == 1:
        return 0
    nb = 2 * tw + 2 * (th - 2)
    most = 0
    for idx in range(n * tiles_x * tiles_y * nb):
        b, rest = idx % nb, idx // nb
        tile, s = rest % (tiles_x * tiles_y), rest // (tiles_x * tiles_y)
        ty, tx = divmod(tile, tiles_x)
        if b < 2 * tw:
            py, px = (0 if b < tw else th - 1), b & (tw - 1)
        else:
            c = b - 2 * tw
            py, px = 1 + (c >> 1), (tw - 1 if c & 1 else 0)
        gy, gx = ty * th + py, tx * tw + px
        terms = 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ny, nx = ty + dy, tx + dx
                if (dy == 0 and dx == 0) or not (0 <= ny < tiles_y and 0 <= nx < tiles_x):
                    continue
                oy, ox = gy - ny * th, gx - nx * tw
                if oy < -1 or oy > th or ox < -1 or ox > tw:
                    continue
                pred[s, gy, gx] += ring[s, ny * tiles_x + nx, ring_slot(oy, ox, tw, th)]
                terms += 1
        most = max(most, terms)
    return most


@pytest.mark.parametrize("n,H,W,most", [(3, 32, 32, 1), (2, 16, 16, 0), (1, 64, 64, 3)])
def test_tail_fold_index_maps_reproduce_conv2d(n, H, W, most):
    torch.manual_seed(5)
    Co = 3
    y = torch.randn(n, 128, H, W)
    wo = torch.randn(Co, 128, 3, 3) / 34.0
    bo = torch.randn(Co)
    Wt = E.pack_tail(wo, L.DC_F32, "cpu")
    assert tuple(Wt.shape) == (32, 128) and torch.count_nonzero(Wt[9 * Co:]) == 0
    for tap in range(9):
        assert torch.equal(Wt[tap * Co:(tap + 1) * Co], wo[:, :, tap // 3, tap % 3])
    pred, ring = fold(y.permute(0, 2, 3, 1).numpy(), Wt.numpy(), bo.numpy(), Co)
    assert np.isfinite(pred).all()                     # every pixel is some tile's own
    assert combine(pred, ring) == most                 # neighbours per border pixel: none / the tile above or below / three at a crossing
    ref = F.conv2d(y.double(), wo.double(), bo.double(), padding=1).permute(0, 2, 3, 1).numpy()
    assert np.isfinite(pred).all()
    np.testing.assert_allclose(pred, ref, rtol=0, atol=2e-5 * np.abs(ref).max())


def test_ring_slots_are_a_bijection_onto_the_surround():
    for tw, th in [(32, 8), (16, 16)]:
        pos = [(oy, ox) for oy in range(-1, th + 1) for ox in range(-1, tw + 1) if not (0 <= oy < th and 0 <= ox < tw)]
        slots = sorted(ring_slot(oy, ox, tw, th) for oy, ox in pos)
        assert slots == list(range(2 * (tw + 2) + 2 * th))


def test_tail_fold_symbols_and_struct_layout():
    import ctypes as C
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(L.PnTailParams) == 7 * ptr + 6 * 4 and C.sizeof(L.Conv3PnTailOp) == 2 * ptr
    assert {"dc_conv3_pn_tail", "dc_conv3_pn_tail_ok", "dc_conv3_pn_tail_variant", "dc_conv3_pn_tail_ring_floats"} <= set(L.EXPORTS)
    assert L.OP_CONV3_PN_TAIL == 22
    lib = L.lib()
    # probes touch no memory: a 3x3 bf16 conv with Cout = 128 on 32x32 images is served, f32 and Co = 4 are not
    d = C.addressof((C.c_char * 64)()) + 15 & ~15
    conv = lambda dt, Cout=128: L.IgemmParams(dtype=dt, taps=9, stride=1, upsample=0, n_img=4, Hin=32, Win=32, Hout=32, Wout=32, src0=d, C0=128, W=d,
                                              Cout=Cout, tile_n=128, out_dtype=dt, out_ld=Cout, qstats=d)
    tail = lambda Co: L.PnTailParams(Co=Co, pred_ld=Co, groups=32, silu=1, eps=1e-5)
    assert lib.dc_conv3_pn_tail_ok(conv(L.DC_BF16), tail(3)) == 1
    assert lib.dc_conv3_pn_tail_variant(conv(L.DC_F16), tail(3)) == b"conv3_halo<f16,4w,pn,tail>"
    assert lib.dc_conv3_pn_tail_ring_floats(conv(L.DC_BF16), tail(3)) == 4 * 4 * 84 * 3
    assert lib.dc_conv3_pn_tail_ok(conv(L.DC_F32), tail(3)) == 0
    assert lib.dc_conv3_pn_tail_ok(conv(L.DC_BF16), tail(4)) == 0
    assert lib.dc_conv3_pn_tail_ok(conv(L.DC_BF16, 256), tail(3)) == 0
