"""The split-operand GEMMs term by term: with signed permutation weights every dot product of a message layer
and of W_o is ONE product of full-mantissa operands, and each element is held to the elementwise bound of
split_cases.py -- 2^-21 (|Z_0| + |w_i| sum_j |c_j| |M_j|), plus the fp16-pair floor where pairs may multiply --
against a float64 reference built from the kernel's own Z_0 and previous layer.  test_split_ref.py shows on
these same inputs that the complete schemes stay under the bound and that a scheme that lost one product puts
a quarter or more of the elements over it.

Intermediates are read where the code exposes them: the training forward's saved pre-activations
(gemm_variant 0 and 9), and the no-grad forward's debug stops and W_o dump on register-staged (12) and pair (13)
layers at hidden 257 (Hk 320: the smallest size that lays out pair tiles).  Paths that expose only their output
are probed through W_o alone (split_cases.OUTPUT_CASES).

The scale in the pair floor is that of the largest message of the whole batch (no tile has a smaller scale, so
the term covers any tiling), except where a test decodes pair tiles and knows each tile's scale word."""
import ctypes

import numpy as np
import pytest
import torch

import split_cases as sc
from chemprop_amd import TrainArgs, _native, mpn
from chemprop_amd.featurization import get_atom_fdim, get_bond_fdim
from chemprop_amd.mpn import MPNEncoder
from oracle import split_ref as sr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FA, FB = get_atom_fdim(), get_bond_fdim()


def _encoder(args, params, atom=False):
    enc = MPNEncoder(args, FA, get_bond_fdim(atom_messages=atom))
    sc.load_parameters(enc, params)
    return enc.to(DEV).eval()


def _ws_bytes(enc, g, save=False, variant=None, n_blocks=None):
    """wdmpnn_workspace_bytes of ``enc``'s forward on ``g`` (``save``: the training forward), optionally under
    another gemm_variant or with the molecule blocks withheld."""
    dg = g.device_graph(DEV, enc.atom_messages, enc.bond_fdim, not enc.bias and not save)
    gs = _native.WdGraph.from_buffer_copy(enc._graph_struct(dg))
    if n_blocks is not None:
        gs.n_blocks = n_blocks
    cfg = enc._config(save)
    if variant is not None:
        cfg.gemm_variant = variant
    params = tuple(t.detach() if t is not None else None for t in enc._param_tuple())
    pstruct, _ = enc._packed_params(gs, cfg, params, DEV, cache=False)
    n = ctypes.c_size_t()
    _native.check(_native.lib().wdmpnn_workspace_bytes(ctypes.byref(gs), ctypes.byref(pstruct), ctypes.byref(cfg),
                                                       ctypes.byref(n)), 'workspace')
    return n.value


def _runs_blocked(enc, g, save=False):
    return _ws_bytes(enc, g, save) != _ws_bytes(enc, g, save, n_blocks=0)


def _lays_out_pairs(enc, g):
    return _ws_bytes(enc, g, variant=_native.VARIANT_PAIRS) != _ws_bytes(enc, g, variant=_native.VARIANT_STAGED)


def _global_scales(M, W):
    """(per-source-row message scale, weight scale) of the pair floor, from the batch's largest message."""
    s_m = float(sr.h2_scale(sr.abs_bits(np.abs(M).max(initial=0.0))))
    return np.full(M.shape[0], s_m), float(sr.h2_scale(sr.abs_bits(np.abs(W).max())))


def _assert_under(tag, Z, ref, bound, rows):
    top, over = sc.worst(Z, ref, bound, rows)
    print(f'\n{tag}: worst |error| / bound {top:.3f}')
    assert over == 0.0, (tag, top, over)
    return top


# ---------------------------------------------------------------------------------------------------
# the training forward's saved pre-activations
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,variant', [('h300', 0), ('h70', 0), ('h300', 9), ('h70', 9)])
def test_training_forward_layers_and_w_o(name, variant):
    kind, b, hidden, depth = sc.LAYER_CASES[name]
    g = sc.make_graph(kind, b)
    params, info = sc.probe_parameters(hidden, FA, FB, sc.case_seed(name))
    enc = _encoder(TrainArgs(hidden_size=hidden, depth=depth), params)
    enc._gemm_variant = variant
    assert _runs_blocked(enc, g, save=True) == (variant == 0)  # 9: f32 MFMA on the unblocked path
    out = enc(g)
    saved = mpn.saved_preactivations(out)
    Z = [z.cpu().numpy() for z in saved['Z']]
    Zo = saved['Zo'].cpu().numpy()
    assert len(Z) == depth and all(np.isfinite(z).all() for z in Z) and np.isfinite(Zo).all()
    Wh, Wo = params['W_h.weight'].numpy(), params['W_o.weight'].numpy()[:, FA:]
    # (the gather entries of a row are those of the form its path evaluates: split_cases.fused_message_gather)
    msg = sc.fused_message_gather(g) if variant == 0 else g.bond_message_gather()
    agg = g.atom_aggregate_gather()
    f64 = g.f_bonds.numpy().astype(np.float64) @ params['W_i.weight'].numpy().astype(np.float64).T
    assert np.abs(Z[0] - f64).max() <= 1e-5 * np.abs(f64).max()  # (Z_0 is the input layer's, as the test assumes)
    for t in range(1, depth):
        M = sc.relu(Z[t - 1])
        ref, bound = sc.layer_reference(Z[0], M, msg, info['pi_h'], info['w_h'],
                                        _global_scales(M, Wh) if variant == 0 else None)
        _assert_under(f'training v{variant} {name} layer {t}', Z[t], ref, bound, slice(1, g.n_bonds))
    M = sc.relu(Z[-1])
    ref, bound = sc.layer_reference(np.zeros_like(Zo), M, agg, info['pi_o'], info['w_o'],
                                    _global_scales(M, Wo) if variant == 0 else None)
    _assert_under(f'training v{variant} {name} W_o', Zo, ref, bound, slice(1, g.n_atoms))


# ---------------------------------------------------------------------------------------------------
# the no-grad forward's debug stops: register-staged and pair layers at hidden 257
# ---------------------------------------------------------------------------------------------------
class _Stops:
    """The fused forward of one encoder on one batch, stopped after a stage, with its workspace decoded."""

    def __init__(self, enc, g, hidden):
        self.enc, self.g, self.H = enc, g, hidden
        self.Hk = -(-hidden // 64) * 64
        self.dg = g.device_graph(DEV, False, FB)
        gs = enc._graph_struct(self.dg)
        torch.cuda.synchronize()
        self.blocks = sc.dev_read(self.dg, gs.blocks, gs.n_blocks * 32).view(np.int32).reshape(-1, 8).astype(np.int64)
        self.L = _native.lib()
        self.L.wdmpnn_debug_fwd_offsets.argtypes = [ctypes.c_void_p] * 4
        self.L.wdmpnn_debug_fwd_offsets.restype = ctypes.c_int

    def run(self, layers, stage):
        """(workspace bytes, offsets) after the forward stopped at ``stage`` (wdmpnn.h WD_VARIANT_DEBUG_STOP)."""
        enc = self.enc
        enc._gemm_variant = _native.variant_debug(layers, stage)
        with torch.no_grad():
            enc(self.g)
        torch.cuda.synchronize()
        gs = enc._graph_struct(self.dg)
        cfg = enc._config(False)
        params = tuple(t.detach() if t is not None else None for t in enc._param_tuple())
        pstruct, _ = enc._packed_params(gs, cfg, params, DEV, cache=False)
        offs = (ctypes.c_size_t * 15)()
        _native.check(self.L.wdmpnn_debug_fwd_offsets(ctypes.addressof(gs), ctypes.addressof(pstruct),
                                                      ctypes.addressof(cfg), ctypes.addressof(offs)), 'offsets')
        ws = enc._ws_by_stream[_native.current_stream(DEV)].cpu().numpy()
        enc._gemm_variant = 0
        assert offs[9] == 1  # the workspace holds pair tiles
        return ws, list(offs)

    def rows_f32(self, ws, off, rows):
        """fp32 [rows][Hk] in natural row order at ``off``, the first H columns (the rest must be 0)."""
        z = ws[off:off + rows * self.Hk * 4].view(np.float32).reshape(rows, self.Hk)
        assert not z[:, self.H:].any()
        return z[:, :self.H]

    def _natural(self, tiles, br, col, rows):
        """block-row layout [n_blocks * br][Hk] -> natural rows (``col``: the blocks' start column)."""
        out = np.zeros((rows,) + tiles.shape[1:], tiles.dtype)
        for k, b in enumerate(self.blocks):
            out[b[col]:b[col] + b[col + 1]] = tiles[br * k:br * k + b[col + 1]]
        return out

    def pairs(self, ws, off, br, words_off, group, col, rows):
        """(values, scales) float64 [rows][H] in natural rows of pair tiles with ``br``-row blocks whose scale
        words sit at ``words_off``, one per block and ``group`` columns."""
        nblk = len(self.blocks)
        hi, lo = sr.decode_pairs(ws[off:off + nblk * br * self.Hk * 4], nblk * br, self.Hk, br)
        words = ws[words_off:words_off + 4 * nblk * (self.Hk // group)].view(np.uint32).reshape(nblk, self.Hk // group)
        s = sr.h2_scale(words)[:, np.arange(self.Hk) // group]  # [nblk][Hk]
        with np.errstate(invalid='ignore'):  # (tile rows past a block's count hold whatever the buffer held)
            v = (hi.astype(np.float64) + lo.astype(np.float64)) / np.repeat(s, br, axis=0)
        v, s = self._natural(v, br, col, rows), self._natural(np.repeat(s, br, axis=0), br, col, rows)
        assert not v[:, self.H:].any()
        return v[:, :self.H], np.where(s[:, :self.H] > 0, s[:, :self.H], np.inf)

    def planes(self, ws, off, br, col, rows):
        nblk = len(self.blocks)
        h, m, l = sr.decode_planes(ws[off:off + nblk * br * self.Hk * 6], nblk * br, self.Hk, br)
        with np.errstate(invalid='ignore'):  # (as in pairs: rows past a block's count are never copied)
            v = self._natural(h.astype(np.float64) + m + l, br, col, rows)
        assert not v[:, self.H:].any()
        return v[:, :self.H]


@pytest.fixture(scope='module')
def stops():
    kind, b, hidden, depth = sc.LAYER_CASES['h257']
    g = sc.make_graph(kind, b)
    params, info = sc.probe_parameters(hidden, FA, FB, sc.case_seed('h257'))
    enc = _encoder(TrainArgs(hidden_size=hidden, depth=depth), params)
    assert depth == 3 and _runs_blocked(enc, g) and _lays_out_pairs(enc, g)
    return _Stops(enc, g, hidden), params, info


def _pair_repr(ref_abs, bound, s):
    """What decoding a value from its pair tile adds: 2^-22 of the value (itself within ``bound`` of the
    reference) or, where lo is subnormal, 2^-25 of the tile's scaled unit."""
    return 2.0 ** -22 * (ref_abs + bound) + 2.0 ** -25 / s


@pytest.mark.parametrize('layers', ['staged', 'pairs'])
def test_no_grad_layers_through_debug_stops(stops, layers):
    S, params, info = stops
    g, H = S.g, S.H
    code = _native.DEBUG_STAGED if layers == 'staged' else _native.DEBUG_PAIRS
    Wh, Wo = params['W_h.weight'].numpy(), params['W_o.weight'].numpy()[:, FA:]
    msg, agg = sc.fused_message_gather(g), g.atom_aggregate_gather()
    bonds, atoms = slice(1, g.n_bonds), slice(1, g.n_atoms)

    # layer 1 from the embed's Z_0
    ws, off = S.run(code, 2)
    Z0 = S.rows_f32(ws, off[0], g.n_bonds).copy()
    M0 = sc.relu(Z0)
    ref1, b1 = sc.layer_reference(Z0, M0, msg, info['pi_h'], info['w_h'], _global_scales(M0, Wh))
    if layers == 'staged':
        Z1 = S.rows_f32(ws, off[7], g.n_bonds).copy()
        _assert_under('staged layer 1', Z1, ref1, b1, bonds)
        M1 = sc.relu(Z1).astype(np.float64)
    else:  # the layer hands relu(Z_1) on as pair tiles: relu moves no error, the tile adds its representation
        M1, s1 = S.pairs(ws, off[2], 128, off[5], 80, 0, g.n_bonds)
        _assert_under('pairs layer 1 (M_1 tiles)', M1, sc.relu(ref1), b1 + _pair_repr(sc.relu(ref1), b1, s1), bonds)

    # layer 2 and the atom aggregate A it hands to W_o, from the kernel's own M_1: Z_2 within the layer bound,
    # relu and the aggregate's weights carry that bound through, the aggregate's own fp32 sums add (entries + 1)
    # 2^-24 of sum |c| |M_2|, and on the pair path A's tile its representation
    ref2, b2 = sc.layer_reference(Z0, M1, msg, info['pi_h'], info['w_h'], _global_scales(M1, Wh))
    M2 = sc.relu(ref2)
    A_ref, A_abs = sc.gather_sums(agg, M2)
    bA = sc.gather_sums(agg, b2)[1] + (np.diff(agg.ptr)[:, None] + 1) * 2.0 ** -24 * A_abs
    ws, off = S.run(code, 3)
    if layers == 'staged':
        A = S.planes(ws, off[3], 64, 2, g.n_atoms)
    else:
        A, sA = S.pairs(ws, off[3], 64, off[4], 80, 2, g.n_atoms)
        bA = bA + _pair_repr(np.abs(A_ref), bA, sA)
    _assert_under(f'{layers} layer 2 + aggregate (A)', A, A_ref, bA, atoms)

    # W_o from the kernel's own A
    ws, off = S.run(code, _native.DEBUG_WO_DUMP)
    if layers == 'staged':
        A = S.planes(ws, off[3], 64, 2, g.n_atoms)
        Zo = S.rows_f32(ws, off[7], g.n_atoms)
        floor = 0.0
    else:
        A, sA = S.pairs(ws, off[3], 64, off[4], 80, 2, g.n_atoms)
        Zo = S.rows_f32(ws, off[2], g.n_atoms)
        s_w = float(sr.h2_scale(sr.abs_bits(np.abs(Wo).max())))
        w = np.abs(info['w_o'].astype(np.float64))[None, :]
        floor = w * (2.0 ** -25 / sA)[:, info['pi_o']] + 2.0 ** -25 / s_w * np.abs(A)[:, info['pi_o']]
    ref = info['w_o'].astype(np.float64)[None, :] * A[:, info['pi_o']]
    _assert_under(f'{layers} W_o', Zo, ref, sc.REL * np.abs(ref) + floor, atoms)


# ---------------------------------------------------------------------------------------------------
# paths that expose only their output
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(sc.OUTPUT_CASES))
def test_output_only_paths_through_w_o(name):
    case = sc.OUTPUT_CASES[name]
    g = sc.output_graph(case)
    params, info = sc.output_parameters(case)
    atom = bool(case.get('atom'))
    enc = _encoder(sc.output_args(case), params, atom)
    # the intended path
    assert _runs_blocked(enc, g) == (case['path'] != 'unblocked')
    if not atom:
        assert _lays_out_pairs(enc, g) == bool(case.get('pairs') or case['path'] == 'small')
    if case['path'] == 'small':
        st = g.device_graph(DEV, False, FB).struct
        assert 0 < st.blk_max_bonds <= 32 and st.blk_max_atoms <= 32 and st.atom_codes
    if case['kind'] == 'hub':
        assert g.molecule_blocks() is None
    elif case['path'] != 'small':
        assert len(g.molecule_blocks()) >= 2 and g.molecule_blocks()[:, 1].max() > 64  # several 16-row groups
    with torch.no_grad():
        out = enc(g).cpu().numpy()
    assert np.isfinite(out).all()
    ref, bound = sc.output_reference(g, params, info, case)
    real = ref != 0
    assert real.mean() > 0.5 and not out[~real].any()
    ratio = np.abs(out.astype(np.float64) - ref)[real] / bound[real]
    print(f'\noutput {name}: worst |error| / bound {ratio.max():.3f}')
    assert (ratio <= 1.0).all(), (name, float(ratio.max()), float((ratio > 1.0).mean()))
