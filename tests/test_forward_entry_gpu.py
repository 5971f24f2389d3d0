"""GPU: the entries of the fused forward kernels (embed, pair layers, pair W_o + readout).

The entries copy a head of their arguments by value, decode the grid tile into (molecule block, column tile)
with a multiplication by a host-made reciprocal instead of a division (common.hpp tile_split), skip the job
search in one-batch launches (multi_pick), add the embed's column sums without branches (code_sum) and issue
the loaders' first weight copies ahead of the block row (gemm_x6.hpp h2_mainloop_pairs).  None of that may
change a bit of any output; each test below aims at one of these steps with the smallest shapes at which it
can go wrong.

Tolerances: 1e-5 normwise against the fp32 oracle and 2e-6 against the register-staged layers (gemm_variant
12) are the project's standing bounds for the pair layers (tests/test_early_copies_gpu.py); everything else
is bitwise or exact.
"""
import ctypes

import numpy as np
import pytest
import torch

from chemprop_amd import TrainArgs, _native, synthetic
from chemprop_amd.featurization import BatchMolGraph, get_atom_fdim, get_bond_fdim
from chemprop_amd.mpn import MPNEncoder
from oracle import mpn_ref

import golden_io

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FA, FB = get_atom_fdim(), get_bond_fdim()


def _chain(rng, n_atoms, extra_edges=()):
    """A chain of ``n_atoms`` atoms (+ ring closures): 2 (n_atoms - 1 + len(extra_edges)) bond rows."""
    pairs = {(i, i + 1) for i in range(n_atoms - 1)} | set(extra_edges)
    return synthetic._build(rng, n_atoms, pairs, [], [1.0] * n_atoms, 1.0)


def _full(rng):
    """128 bond rows, 64 atoms: a molecule block's capacity, so every such molecule is a block of its own"""
    return _chain(rng, 64, [(3, 40)])


def _encoder(hidden, depth, seed=21, **extra):
    args = TrainArgs(hidden_size=hidden, depth=depth, **extra)
    enc = MPNEncoder(args, FA, FB)
    synthetic.fill_parameters(enc, seed)
    p = {n: t.detach().clone() for n, t in enc.named_parameters()}
    return args, enc.to(DEV).eval(), p


def _forward(enc, g, variant, fill):
    """wdmpnn_forward on a workspace of the caller's, every byte ``fill`` before the call: (out, ws, offsets)"""
    L = _native.lib()
    enc._gemm_variant = variant
    dg = g.device_graph(DEV, False, FB)
    dg.use_on(torch.cuda.current_stream(DEV))
    gs = enc._graph_struct(dg)
    cfg = enc._config(False)
    params = tuple(t.detach().float() if t is not None else None for t in enc._param_tuple())
    pstruct, keep = enc._packed_params(gs, cfg, params, DEV)
    n = ctypes.c_size_t()
    _native.check(L.wdmpnn_workspace_bytes(ctypes.byref(gs), ctypes.byref(pstruct), ctypes.byref(cfg), ctypes.byref(n)),
                  'workspace')
    ws = torch.full((max(n.value, 256),), fill, dtype=torch.uint8, device=DEV)
    out = torch.full((gs.n_mols, enc.hidden_size), float('nan'), dtype=torch.float32, device=DEV)
    _native.check(L.wdmpnn_forward(ctypes.byref(gs), ctypes.byref(pstruct), ctypes.byref(cfg), ws.data_ptr(), n.value,
                                   out.data_ptr(), _native.current_stream(DEV)), 'forward')
    torch.cuda.synchronize()
    offs = (ctypes.c_size_t * 15)()
    L.wdmpnn_debug_fwd_offsets.argtypes = [ctypes.c_void_p] * 4
    L.wdmpnn_debug_fwd_offsets.restype = ctypes.c_int
    _native.check(L.wdmpnn_debug_fwd_offsets(ctypes.addressof(gs), ctypes.addressof(pstruct), ctypes.addressof(cfg),
                                             ctypes.addressof(offs)), 'offsets')
    enc._gemm_variant = 0
    del keep, dg
    return out, ws, list(offs)


# ---------------------------------------------------------------------------------------------------
# tile -> (block, column tile) without a division
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def block_graphs():
    """n -> a graph of n full molecule blocks (1, 3, 9: no multiple of the chip's 8 XCDs)"""
    rng = np.random.default_rng(5)
    out = {}
    for n in (1, 3, 9):
        g = BatchMolGraph([_full(rng) for _ in range(n)], device_bond_features=True)
        assert np.asarray(g.molecule_blocks()).shape[0] == n
        out[n] = g
    return out


@pytest.mark.parametrize('depth', [2, 3])
@pytest.mark.parametrize('nblk', [1, 3, 9])
@pytest.mark.parametrize('hidden', [300, 600])
def test_tile_decode_without_division(block_graphs, hidden, nblk, depth):
    """Hidden 300 / 600: 4 / 8 column tiles of 80 (and 10 / 20 embed tiles of 32), grids of 4 .. 72 workgroups
    whose XCD ranges are uneven.  A wrong (block, tile) pair reads another block's rows or writes other
    columns: the oracle's at 1e-5 normwise, the register-staged layers' at 2e-6."""
    g = block_graphs[nblk]
    args, enc, p = _encoder(hidden, depth)
    ref = mpn_ref.encoder_forward(p, g, args).numpy()
    pairs, _, offs = _forward(enc, g, _native.VARIANT_PAIRS, 0x00)
    assert offs[9] == 1  # (pair tiles: the kernels under test ran)
    staged, _, _ = _forward(enc, g, _native.VARIANT_STAGED, 0x00)
    e_ref = golden_io.normwise(pairs.cpu().numpy(), ref)
    e_stg = golden_io.normwise(pairs.cpu().numpy(), staged.cpu().numpy())
    print(f'hidden {hidden} blocks {nblk} depth {depth}: vs oracle {e_ref:.3e}, vs staged {e_stg:.3e}')
    assert torch.isfinite(pairs).all()
    assert e_ref <= 1e-5
    assert e_stg <= 2e-6


# ---------------------------------------------------------------------------------------------------
# the job search of launches with several batches, against the one-batch launches that skip it
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counts', [(1, 3), (9, 1), (1, 3, 9), (3, 9, 1)])
def test_job_search_equals_single_forwards(counts):
    rng = np.random.default_rng(9)
    graphs = [BatchMolGraph([_full(rng) for _ in range(n)], device_bond_features=True, block_target=1) for n in counts]
    assert tuple(np.asarray(g.molecule_blocks()).shape[0] for g in graphs) == counts
    _, enc, _ = _encoder(300, 3)
    with torch.no_grad():
        one = [enc(g) for g in graphs]
        many = enc.forward_many(graphs)
    torch.cuda.synchronize()
    assert len(many) == len(graphs)
    for a, b in zip(one, many):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------
# the embed's column sums
# ---------------------------------------------------------------------------------------------------
def _set_feature(mol, atom, aromatic=None, mass=None):
    """Rewrite an atom's aromatic flag (the only optional 1.0 of an atom row: 6 or 7 set columns) / its mass
    column, in its row and in the rows of the bonds leaving it."""
    rows = [mol.f_atoms[atom]] + [mol.f_bonds[b] for b in range(mol.n_bonds) if mol.b2a[b] == atom]
    for r in rows:
        if aromatic is not None:
            r[FA - 2] = float(aromatic)
        if mass is not None:
            r[FA - 1] = float(mass)


@pytest.fixture(scope='module')
def code_block():
    """One block: a lone atom, and a chain whose atoms carry the fewest (6) and the most (7) set columns the
    featuriser produces, each with the mass column zero and non-zero."""
    rng = np.random.default_rng(31)
    chain = _chain(rng, 8)
    for atom, (aro, mass) in enumerate([(0, 0.0), (0, None), (1, 0.0), (1, None)]):
        _set_feature(chain, atom, aromatic=aro, mass=mass)
    mols = [synthetic.single_atom_graph(rng), chain, _chain(rng, 5)]
    host = BatchMolGraph(mols)
    dev = BatchMolGraph(mols, device_bond_features=True, block_target=1)
    assert np.asarray(dev.molecule_blocks()).shape[0] == 1
    fa = host.f_atoms.numpy()
    nset = (fa[1:, :FA - 1] != 0).sum(1)
    assert nset.min() == 6 and nset.max() == 7
    for n in (6, 7):
        assert (fa[1:, FA - 1][nset == n] == 0).any() and (fa[1:, FA - 1][nset == n] != 0).any()
    return host, dev


def test_code_sums_on_hostile_workspaces(code_block):
    """Depth 2 (embed, one layer, W_o): bitwise the same on a zero-byte and a 0xFF-byte workspace, finite, the
    oracle's at 1e-5."""
    host, dev = code_block
    args, enc, p = _encoder(300, 2, bias=True)
    zero, _, _ = _forward(enc, dev, _native.VARIANT_PAIRS, 0x00)
    ones, _, _ = _forward(enc, dev, _native.VARIANT_PAIRS, 0xFF)
    assert torch.isfinite(zero).all() and torch.isfinite(ones).all()
    assert torch.equal(zero, ones)
    ref = mpn_ref.encoder_forward(p, host, args)
    assert golden_io.normwise(zero.cpu().numpy(), ref.numpy()) <= 1e-5


def _step_sum(start, terms):
    """start + terms[0] + terms[1] + ... in fp64, cast to fp32 after every step"""
    s = start.astype(np.float32)
    for t in terms:
        s = (s.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    return s


def test_inp_and_eo_are_the_ordered_column_sums(code_block):
    """inp and Eo, read from the workspace, against the column sums in the kernel's order -- ascending set
    columns, then mass * the last atom column; for a bond its source atom's sum, then its set bond columns
    ascending, then the bias -- in fp64 cast to fp32 step by step: exact."""
    host, dev = code_block
    H = 300
    args, enc, p = _encoder(H, 2, bias=True)
    _, ws, offs = _forward(enc, dev, _native.VARIANT_PAIRS, 0xFF)
    Hk = -(-H // 64) * 64
    ws = ws.cpu().numpy()
    fa, fb = host.f_atoms.numpy(), host.f_bonds.numpy()
    n_atoms, n_bonds = fa.shape[0], fb.shape[0]
    inp = ws[offs[0]:offs[0] + n_bonds * Hk * 4].view(np.float32).reshape(n_bonds, Hk)
    eo = ws[offs[14]:offs[14] + n_atoms * Hk * 4].view(np.float32).reshape(n_atoms, Hk)
    assert not inp[:, H:].any() and not eo[1:, H:].any()
    Wi, bi = p['W_i.weight'].numpy(), p['W_i.bias'].numpy()  # [H][Fb], [H]
    Wo = p['W_o.weight'].numpy()                             # [H][Fa + H]

    def atom_sum(W, a):
        cols = np.nonzero(fa[a, :FA - 1])[0]
        assert (fa[a, cols] == 1.0).all()
        s = _step_sum(np.zeros(H, np.float32), [W[:, c] for c in cols])
        # (the mass term is one fma: the fp64 product of two fp32 numbers is exact)
        return (np.float64(fa[a, FA - 1]) * W[:, FA - 1].astype(np.float64) + s.astype(np.float64)).astype(np.float32)

    b2a = host.b2a.numpy()
    for a in range(1, n_atoms):
        assert np.array_equal(eo[a, :H], atom_sum(Wo, a)), f'Eo of atom {a}'
    for b in range(1, n_bonds):
        cols = FA + np.nonzero(fb[b, FA:])[0]
        assert (fb[b, cols] == 1.0).all()
        want = _step_sum(atom_sum(Wi, int(b2a[b])), [Wi[:, c] for c in cols] + [bi])
        assert np.array_equal(inp[b, :H], want), f'inp of bond {b}'
    assert not inp[0].any()  # (the pad row)


# ---------------------------------------------------------------------------------------------------
# the loaders' changed issue order: weight copies, the block row, then the live 16-row groups
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def row_graphs():
    rng = np.random.default_rng(77)
    spec = {16: ([_chain(rng, 9), _chain(rng, 9)], [(16, 9)] * 2),
            18: ([_chain(rng, 10), _chain(rng, 10), _chain(rng, 10)], [(18, 10)] * 3),
            128: ([_full(rng), _full(rng)], [(128, 64)] * 2)}
    out = {}
    for rows, (mols, want) in spec.items():
        g = BatchMolGraph(mols, device_bond_features=True)
        blocks = np.asarray(g.molecule_blocks())
        assert [(int(r[1]), int(r[3])) for r in blocks] == want, blocks
        out[rows] = g
    return out


@pytest.mark.parametrize('rows', [16, 18, 128])
def test_copy_order_on_hostile_workspaces(row_graphs, rows):
    """Blocks of 16, 18 and 128 bond rows (one live 16-row group, two, all eight), depth 3 (both layer
    instantiations): the waits of the new issue order let no chunk be multiplied before it landed and no
    group past the block's rows be read -- zero-byte and 0xFF-byte workspaces give the same bits, finite, the
    oracle's at 1e-5."""
    g = row_graphs[rows]
    args, enc, p = _encoder(300, 3)
    zero, _, _ = _forward(enc, g, _native.VARIANT_PAIRS, 0x00)
    ones, _, _ = _forward(enc, g, _native.VARIANT_PAIRS, 0xFF)
    assert torch.isfinite(zero).all() and torch.isfinite(ones).all()
    assert torch.equal(zero, ones)
    ref = mpn_ref.encoder_forward(p, g, args)
    assert golden_io.normwise(zero.cpu().numpy(), ref.numpy()) <= 1e-5
