"""``wdmpnn_slots_join`` and ``wdmpnn_slots_split`` on the GPU against numpy, bit for bit.

The inputs are random 32-bit patterns viewed as float32 (NaN payloads, infinities, -0.0 and denormals among them):
both kernels are pure copies.  Every feature row index a kernel sees is inside its table (the kernels clamp
nothing); buffers the kernels must not touch are prefilled with a sentinel pattern and compared whole."""
import ctypes

import numpy as np
import pytest
import torch

from chemprop_amd import _native
from chemprop_amd.slots import join_slots, split_slots

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = np.uint32(0xC29A8000)  # -77.25
TABLE_ROWS = 7


def _pattern(rng, *shape):
    a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = a.reshape(-1)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x7f800000, 0xff800000, 1, 0x807fffff],
                       np.uint32)
    flat[:min(len(special), flat.size)] = special[:flat.size]
    return a


def _dev(a):
    return torch.from_numpy(a.view(np.int32).copy()).to(DEV).view(torch.float32)


def _host(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _struct(B, N, H, slot_ptrs, ld_slot, x, feat=None, Ff=0, idx=None):
    s = _native.WdSlots()
    s.B, s.n_slots, s.H, s.ld_slot = B, N, H, ld_slot
    for k, p in enumerate(slot_ptrs):
        s.slot[k] = p
    if feat is not None:
        s.feat, s.ld_feat, s.Ff = feat.data_ptr(), feat.shape[1], Ff
        s.feat_idx = None if idx is None else idx.data_ptr()
    s.x, s.ld_x = x.data_ptr(), x.shape[1]
    return s


def _index(B, how):
    if how == 'none':
        return None
    # repeated and out-of-order rows, every one inside the table
    idx = [(5 * i + 3) % TABLE_ROWS for i in range(B)]
    if B >= 3:
        idx[1] = idx[0]
    assert all(0 <= i < TABLE_ROWS for i in idx)
    return idx


@pytest.mark.parametrize('H', [4, 30, 300])
@pytest.mark.parametrize('B', [1, 3, 67])
def test_join_and_split_against_numpy(B, H):
    """Every N in {1, 2, 3, 8}, Ff in {0, 5} with and without an index, ld_x exact and + 3 (unaligned: the word path,
    sentinel columns unchanged), ld_slot exact and padded, separate slot buffers.  H = 30 gives rows of 120 bytes:
    the word path whatever the rest.  split(join(.)) gives every slot back, and leaves the slots' padding alone."""
    rng = np.random.default_rng(1000 * B + H)
    L = _native.lib()
    sid = _native.current_stream(DEV)
    for N in (1, 2, 3, 8):
        for Ff, how in ((0, 'none'), (5, 'none'), (5, 'index')):
            for pad_x in (0, 3):
                for pad_s in (0, 4):
                    ld_slot, ld_x = H + pad_s, N * H + Ff + pad_x
                    slots_h = [_pattern(rng, B, ld_slot) for _ in range(N)]
                    slots = [_dev(a) for a in slots_h]
                    rows = TABLE_ROWS if how == 'index' else max(B, 1)
                    feat_h = _pattern(rng, rows, 8) if Ff else None
                    feat = None if feat_h is None else _dev(feat_h)
                    idx_l = _index(B, how)
                    idx = None if idx_l is None else torch.tensor(idx_l, dtype=torch.int64, device=DEV)
                    x = _dev(np.full((B, ld_x), SENTINEL, np.uint32))
                    s = _struct(B, N, H, [t.data_ptr() for t in slots], ld_slot, x, feat, Ff, idx)
                    _native.check(L.wdmpnn_slots_join(ctypes.byref(s), sid), 'slots join')
                    want = np.full((B, ld_x), SENTINEL, np.uint32)
                    for k in range(N):
                        want[:, k * H:(k + 1) * H] = slots_h[k][:, :H]
                    if Ff:
                        src = feat_h[idx_l] if idx_l is not None else feat_h[:B]
                        want[:, N * H:N * H + Ff] = src[:, :Ff]
                    case = (N, Ff, how, pad_x, pad_s)
                    assert np.array_equal(_host(x), want), case
                    # the inverse, into sentinel-filled slots: the H columns come back, the padding stays
                    back = [_dev(np.full((B, ld_slot), SENTINEL, np.uint32)) for _ in range(N)]
                    s2 = _struct(B, N, H, [t.data_ptr() for t in back], ld_slot, x, feat, Ff, idx)
                    _native.check(L.wdmpnn_slots_split(ctypes.byref(s2), sid), 'slots split')
                    for k in range(N):
                        w = np.full((B, ld_slot), SENTINEL, np.uint32)
                        w[:, :H] = slots_h[k][:, :H]
                        assert np.array_equal(_host(back[k]), w), case + (k,)
                    assert np.array_equal(_host(x), want), case  # (split reads x only)


@pytest.mark.parametrize('B,H,N', [(67, 300, 2), (3, 30, 3), (1, 4, 8), (67, 4, 8)])
def test_one_buffer_slot_major_form(B, H, N):
    """slot[k] = base + k B H with ld_slot = H: the [N B][H] matrix of a merged batch, through the wrappers the
    training step and the prediction loop use (``join_slots`` with a list of one, ``split_slots``)."""
    rng = np.random.default_rng(7 * B + H + N)
    merged_h = _pattern(rng, N * B, H)
    merged = _dev(merged_h)
    feat_h = _pattern(rng, B, 5)
    x = join_slots([merged], B, _dev(feat_h))
    assert tuple(x.shape) == (B, N * H + 5)
    want = np.concatenate([merged_h[k * B:(k + 1) * B] for k in range(N)] + [feat_h], axis=1)
    assert np.array_equal(_host(x), want)
    x0 = join_slots([merged], B)
    assert np.array_equal(_host(x0), want[:, :N * H])
    d = split_slots(x, N, H)
    assert tuple(d.shape) == (N, B, H) and d.is_contiguous()
    assert np.array_equal(_host(d).reshape(N * B, H), merged_h)
    # separate tensors give the same x
    parts = [_dev(merged_h[k * B:(k + 1) * B]) for k in range(N)]
    assert torch.equal(join_slots(parts, B, _dev(feat_h)).view(torch.int32), x.view(torch.int32))
