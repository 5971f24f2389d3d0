"""The split-operand formats on the device, bit for bit against oracle/split_ref.py: the plane-tile producers
(wdmpnn_split_planes, wdmpnn_split_planes_rows), the plane tiles a device graph carries (host-built and
compact), and the fp16 pair tiles and scale words of the packed W_h and W_o.  Every comparison is exact equality
of bytes; there is no tolerance.  Values stay finite and inside [2^-96, 2^100] (outside it the l plane may
underflow: not part of the contract)."""
import ctypes

import numpy as np
import pytest
import torch

import split_cases as sc
from chemprop_amd import TrainArgs, _native, synthetic
from chemprop_amd.featurization import BatchMolGraph, get_atom_fdim, get_bond_fdim
from chemprop_amd.mpn import MPNEncoder
from oracle import split_ref as sr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GUARD = 4096  # bytes past the destination that must stay untouched


def _bits(v):
    return np.asarray(v, np.uint32).view(np.float32)


def _special_values():
    """Values that sit on the edges of the split: exact ties of the first rounding with h's last bit even and
    odd, exact ties of the second (m's last bit even and odd), values with l = 0, with m = l = 0, and both zeros."""
    tie1 = _bits([0x3f808000, 0x3f818000, 0xbf808000, 0xc1818000, 0x5a7a8000, 0x1a7b8000])
    k = np.arange(8)
    tie2 = (1.0 + 2.0 ** -10 + k * 2.0 ** -17 + 2.0 ** -18).astype(np.float32)  # x - h = 2^-10 (1 + k/128 + 1/256)
    rng = np.random.default_rng(8)
    h, m, _ = sr.split3(sc.full_mantissa(rng, (64,), -60, 60))
    no_l = (h.astype(np.float64) + m).astype(np.float32)
    vals = np.concatenate([tie1, tie2, -tie2, no_l, h, np.array([0.0, -0.0], np.float32)])
    H, M, L = sr.split3(vals)
    n1, n2 = len(tie1), 2 * len(tie2)
    # what each group is there for, checked on the reference's own split
    r1 = (vals.astype(np.float64) - H).astype(np.float32)
    assert ((tie1.view(np.uint32) & 0xffff) == 0x8000).all() and not (sr.bf16_bits(H[:n1]) & 1).any()
    assert set((tie1.view(np.uint32) >> 16) & 1) == {0, 1}  # h's last bit before rounding: even and odd
    assert ((r1[n1:n1 + n2].view(np.uint32) & 0xffff) == 0x8000).all() and not (sr.bf16_bits(M[n1:n1 + n2]) & 1).any()
    assert set((r1[n1:n1 + n2].view(np.uint32) >> 16) & 1) == {0, 1} and (L[n1:n1 + n2] != 0).all()
    assert (L[n1 + n2:n1 + n2 + 64] == 0).all() and (M[n1 + n2:n1 + n2 + 64] != 0).any()
    assert (M[n1 + n2 + 64:] == 0).all() and (L[n1 + n2 + 64:] == 0).all()
    return vals


def _matrix(rows, ld, seed):
    """fp32 [rows][ld]: random sign, exponent and mantissa over [2^-96, 2^100), the special values scattered in."""
    rng = np.random.default_rng(seed)
    x = sc.full_mantissa(rng, (rows, ld), -96, 100)
    sp = _special_values()
    reps = max(1, min(64, x.size // (4 * len(sp))))
    pos = rng.choice(x.size, reps * len(sp), replace=False)
    x.reshape(-1)[pos] = np.tile(sp, reps)
    return x


def _stream():
    return _native.current_stream(DEV)


@pytest.mark.parametrize('rows,kp,ld', [(64, 32, 32), (128, 64, 68), (192, 160, 160), (4160, 2048, 2048)],
                         ids=['64x32', '128x64-ld68', '192x160', 'grid-stride'])
def test_split_planes_bytes(rows, kp, ld):
    """(4160, 2048): 1 064 960 threads' worth of work for a grid capped at 4096 x 256 = 1 048 576."""
    x = _matrix(rows, ld, rows + kp)
    n = rows * kp * 6
    nbytes = ctypes.c_size_t()
    L = _native.lib()
    _native.check(L.wdmpnn_plane_bytes(rows, kp, ctypes.byref(nbytes)), 'plane bytes')
    assert nbytes.value == n
    src = torch.from_numpy(x).to(DEV)
    dst = torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    _native.check(L.wdmpnn_split_planes(src.data_ptr(), ld, rows, kp, dst.data_ptr(), n, _stream()), 'split planes')
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[n:] == 0xFF).all()  # nothing past rows * kp * 6
    want = sr.encode_planes(x[:, :kp])
    assert np.array_equal(got[:n], want)  # (which also says: every 0xFF byte was overwritten)
    h, m, l = sr.decode_planes(got[:n], rows, kp)
    assert np.array_equal(h.astype(np.float64) + m + l, x[:, :kp].astype(np.float64))


def test_split_planes_rows_bytes():
    rng = np.random.default_rng(21)
    rows, out_rows, kp, ld = 200, 320, 64, 68
    x = _matrix(rows, ld, 22)
    row_map = np.full(rows, -1, np.int32)
    keep = rng.permutation(rows)[:150]
    row_map[keep] = rng.permutation(out_rows)[:150].astype(np.int32)
    n = out_rows * kp * 6
    L = _native.lib()
    src, rm = torch.from_numpy(x).to(DEV), torch.from_numpy(row_map).to(DEV)
    dst = torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    _native.check(L.wdmpnn_split_planes_rows(src.data_ptr(), ld, rows, kp, rm.data_ptr(), out_rows, dst.data_ptr(), n,
                                             _stream()), 'split planes rows')
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[n:] == 0xFF).all()
    assert np.array_equal(got[:n], sr.encode_planes(x[:, :kp], 64, row_map, out_rows))
    h, m, l = sr.decode_planes(got[:n], out_rows, kp)
    unmapped = np.setdiff1d(np.arange(out_rows), row_map[keep])
    assert len(unmapped) == out_rows - 150
    for p in (h, m, l):
        assert not p[unmapped].view(np.uint32).any()  # zero rows, +0 in every plane
    assert np.array_equal((h.astype(np.float64) + m + l)[row_map[keep]], x[keep, :kp].astype(np.float64))
    # no source rows: the destination is zero-filled, nothing else is written
    dst.fill_(0xFF)
    _native.check(L.wdmpnn_split_planes_rows(src.data_ptr(), ld, 0, kp, rm.data_ptr(), out_rows, dst.data_ptr(), n,
                                             _stream()), 'split planes rows, no rows')
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert not got[:n].any() and (got[n:] == 0xFF).all()


# ---------------------------------------------------------------------------------------------------
# the graph's planes
# ---------------------------------------------------------------------------------------------------
def _check_graph_planes(dg):
    """f_atoms_x6, f_bonds_x6 and f_atoms_blk_x6 against the fp32 rows the same device graph holds."""
    s = dg.struct
    torch.cuda.synchronize()
    Vap, Rbp = -(-s.n_atoms // 128) * 128, -(-s.n_bonds // 128) * 128
    fa = sc.dev_read(dg, s.f_atoms, Vap * s.ld_atoms * 4).view(np.float32).reshape(Vap, s.ld_atoms)
    fb = sc.dev_read(dg, s.f_bonds, Rbp * s.ld_bonds * 4).view(np.float32).reshape(Rbp, s.ld_bonds)
    assert not fa[s.n_atoms:].any() and not fb[s.n_bonds:].any() and not fa[0].any() and not fb[0].any()
    assert s.f_atoms_x6 and s.f_bonds_x6 and s.f_atoms_blk_x6 and s.n_blocks > 0
    assert np.array_equal(sc.dev_read(dg, s.f_atoms_x6, fa.size * 6), sr.encode_planes(fa))
    assert np.array_equal(sc.dev_read(dg, s.f_bonds_x6, fb.size * 6), sr.encode_planes(fb))
    blocks = sc.dev_read(dg, s.blocks, s.n_blocks * 32).view(np.int32).reshape(-1, 8)
    row_map = np.full(Vap, -1, np.int64)
    for k, b in enumerate(blocks):
        row_map[b[2]:b[2] + b[3]] = 64 * k + np.arange(b[3])
    assert (row_map[1:s.n_atoms] >= 0).all()  # every atom sits in a block
    got = sc.dev_read(dg, s.f_atoms_blk_x6, s.n_blocks * 64 * s.ld_atoms * 6)
    assert np.array_equal(got, sr.encode_planes(fa, 64, row_map, 64 * s.n_blocks))
    return fa, fb


def test_host_built_graph_planes_with_full_mantissa_features():
    g = BatchMolGraph(sc.full_mantissa_mols(synthetic.make_batch('polymer', 8, 31), 31), compact=False)
    dg = g.device_graph(DEV, False, get_bond_fdim())
    assert not dg.built_on_device
    fa, fb = _check_graph_planes(dg)
    n = g.n_atoms
    assert np.array_equal(fa[:n, :get_atom_fdim()], g.f_atoms.numpy())
    h, m, l = sr.split3(fa[1:n, :get_atom_fdim()])
    assert (m != 0).mean() > 0.9 and (l != 0).mean() > 0.9  # every column exercises m and l


def test_compact_graph_planes():
    g = BatchMolGraph(synthetic.make_batch('polymer', 8, 32))
    dg = g.device_graph(DEV, False, get_bond_fdim())
    assert dg.built_on_device
    fa, fb = _check_graph_planes(dg)
    assert np.array_equal(fa[:g.n_atoms, :get_atom_fdim()], g.f_atoms.numpy())
    assert np.array_equal(fb[:g.n_bonds, :get_bond_fdim()], g.f_bonds.numpy())


def test_atom_message_graph_feature_sum_planes():
    """atom_feat_sum_x6: per atom the sum of its in-bonds' feature rows, added in fp32 in the order the packer's
    list emits them, as bf16x3 planes."""
    g = BatchMolGraph(sc.full_mantissa_mols(synthetic.make_batch('polymer', 8, 33), 33), compact=False)
    Fb = get_bond_fdim(atom_messages=True)
    dg = g.device_graph(DEV, True, Fb)
    s = dg.struct
    torch.cuda.synchronize()
    assert s.atom_feat_sum_x6 and s.atom_messages == 1
    Vap, Rbp = -(-s.n_atoms // 128) * 128, -(-s.n_bonds // 128) * 128
    fb = sc.dev_read(dg, s.f_bonds, Rbp * s.ld_bonds * 4).view(np.float32).reshape(Rbp, s.ld_bonds)
    assert np.array_equal(fb[:g.n_bonds, :Fb], g.f_bonds.numpy()[:, -Fb:])
    feat = g.atom_message_gather()[1]
    want = np.zeros((Vap, s.ld_bonds), np.float32)
    for a in range(s.n_atoms):
        for e in range(feat.ptr[a], feat.ptr[a + 1]):  # fp32 adds, list order
            want[a] = want[a] + fb[feat.idx[e]]
    assert np.diff(feat.ptr).max() >= 3 and np.abs(want).max() > 0
    assert np.array_equal(sc.dev_read(dg, s.atom_feat_sum_x6, want.size * 6), sr.encode_planes(want))
    fa = sc.dev_read(dg, s.f_atoms, Vap * s.ld_atoms * 4).view(np.float32).reshape(Vap, s.ld_atoms)
    assert np.array_equal(sc.dev_read(dg, s.f_atoms_x6, fa.size * 6), sr.encode_planes(fa))


# ---------------------------------------------------------------------------------------------------
# packed weights: the pair tiles of W_h and W_o[:, Fa:] and their scale words
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hidden', [300, 257])
def test_packed_pair_tiles_and_scale_words(hidden):
    Fa, Fb = get_atom_fdim(), get_bond_fdim()
    Hk = -(-hidden // 64) * 64
    assert Hk == 320  # 80-row blocks: the layout the pair layers and W_o read
    rng = np.random.default_rng(hidden)
    args = TrainArgs(hidden_size=hidden, depth=3)
    enc = MPNEncoder(args, Fa, Fb)
    w = {'W_i.weight': sc.full_mantissa(rng, (hidden, Fb), -12, 2),
         'W_h.weight': sc.full_mantissa(rng, (hidden, hidden), -42, 3),      # 2^45 between smallest and largest:
         'W_o.weight': sc.full_mantissa(rng, (hidden, Fa + hidden), -40, 6),  # lo, then hi, run out of fp16 range
         'W_o.bias': sc.full_mantissa(rng, (hidden,), -4, 1), 'cached_zero_vector': np.zeros(hidden, np.float32)}
    sc.load_parameters(enc, {n: torch.from_numpy(a) for n, a in w.items()})
    enc = enc.to(DEV).eval()
    g = BatchMolGraph(synthetic.make_batch('polymer', 4, 34))
    dg = g.device_graph(DEV, False, Fb)
    gs = enc._graph_struct(dg)
    cfg = enc._config(False)
    params = tuple(t.detach() if t is not None else None for t in enc._param_tuple())
    pstruct, buf = enc._packed_params(gs, cfg, params, DEV, cache=False)
    L = _native.lib()
    L.wdmpnn_debug_fwd_offsets.argtypes = [ctypes.c_void_p] * 4
    L.wdmpnn_debug_fwd_offsets.restype = ctypes.c_int
    offs = (ctypes.c_size_t * 15)()
    _native.check(L.wdmpnn_debug_fwd_offsets(ctypes.addressof(gs), ctypes.addressof(pstruct), ctypes.addressof(cfg),
                                             ctypes.addressof(offs)), 'offsets')
    torch.cuda.synchronize()
    pk = buf.cpu().numpy()
    wo_tiles, wo_words, wh_tiles, wh_words = offs[10], offs[11], offs[12], offs[13]
    assert wo_tiles and wo_words and wh_tiles and wh_words  # this pack holds both pair-tile sets
    for name, W, tiles, words in (('W_h', w['W_h.weight'], wh_tiles, wh_words),
                                  ('W_o', w['W_o.weight'][:, Fa:], wo_tiles, wo_words)):
        word = int(pk[words + 4 * 64:words + 4 * 65].view(np.uint32)[0])
        assert word == int(sr.abs_bits(np.abs(W).max())), name  # the folded word: the bits of max |W|
        s = float(sr.h2_scale(word))
        assert 2.0 ** 14 <= float(np.abs(W).max()) * s < 2.0 ** 15, name
        padded = np.zeros((Hk, Hk), np.float32)
        padded[:hidden, :hidden] = W
        hi, lo = sr.decode_pairs(pk[tiles:tiles + Hk * Hk * 4], Hk, Hk, 80)
        HI, LO = sr.split_h2(padded, s)
        assert np.array_equal(hi.view(np.uint16), HI.view(np.uint16)), name
        assert np.array_equal(lo.view(np.uint16), LO.view(np.uint16)), name
        for p in (hi, lo):  # padding rows and columns: +0
            assert not p[hidden:].view(np.uint16).any() and not p[:, hidden:].view(np.uint16).any(), name
        # the range is exercised: subnormal and zero halves among the real entries
        lo_real = np.abs(lo[:hidden, :hidden].astype(np.float64))
        assert ((lo_real > 0) & (lo_real < 2.0 ** -14)).any() and (hi[:hidden, :hidden] == 0).any(), name
