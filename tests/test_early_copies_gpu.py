"""GPU: the pair-operand layers on caller-owned workspaces whose never-written bytes are hostile.

The pair layers' loader waves (gemm_x6.hpp h2_mainloop_pairs) copy M_{t-1} from pair tiles that the producers
write only up to a block's last live 16-row group (a measured variant, DESIGN.md "Measured dead ends", copied
every group of the first NS - 1 chunks, past it too).  Whatever the rows past it hold is what the caller's
workspace held, and the consumers must never multiply it.  The tests run wdmpnn_forward through the C-ABI on a workspace pre-filled with zero bytes and with
0xFF bytes (every never-written fp16 then reads as NaN) and ask for bitwise equal, finite outputs, on blocks
at the edges of the 16-row groups, and against the oracle and the register-staged layers.

Two of the cases asked for cannot be built and are replaced by their nearest neighbours:
  * a block of 17 bond rows: bond rows come in directed pairs, so a block's row count is even; the block here
    has 18 (two live rows in the second 16-row group);
  * a hidden size whose chunk count is <= NS - 1 = 2: pair layers need 80 | Hk and Hk = 64 ceil(H / 64), so
    the smallest Hk is 320 (hidden 257 .. 320, ten chunks); hidden 257 is what runs here.
"""
import ctypes
import json
import os

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
TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'layout_contract.json')


def _mol(rng, n_atoms, extra_edges=()):
    """A chain of ``n_atoms`` atoms (+ ring closures): 2 (n_atoms - 1 + len(extra_edges)) bond rows."""
    pairs = {(i, i + 1) for i in range(n_atoms - 1)} | set(extra_edges)
    return synthetic._build(rng, n_atoms, pairs, [], [1.0] * n_atoms, 1.0)


def _graphs():
    """name -> (molecules, the (bond rows, atom rows) of the blocks they must pack into)"""
    rng = np.random.default_rng(77)
    full = lambda: _mol(rng, 64, [(3, 40)])  # noqa: E731  (128 bond rows, 64 atoms: the capacity)
    return {
        'rows18': ([_mol(rng, 10), _mol(rng, 10), _mol(rng, 10)], [(18, 10)] * 3),
        'rows16': ([_mol(rng, 9), _mol(rng, 9)], [(16, 9)] * 2),
        'rows128': ([full(), full()], [(128, 64)] * 2),
        'lone_atom': ([full(), synthetic.single_atom_graph(rng), full()], [(128, 64), (0, 1), (128, 64)]),
    }


GRAPHS = _graphs()


def _batch(name):
    mols, want = GRAPHS[name]
    g = BatchMolGraph(mols, device_bond_features=True)
    blocks = np.asarray(g.molecule_blocks())
    assert [(int(r[1]), int(r[3])) for r in blocks] == want, blocks
    return g


def _encoder(hidden, depth, seed=14, **extra):
    args = TrainArgs(hidden_size=hidden, depth=depth, **extra)
    enc = MPNEncoder(args, get_atom_fdim(), get_bond_fdim())
    synthetic.fill_parameters(enc, seed)
    p = {n: t.detach().clone() for n, t in enc.named_parameters()}
    return args, enc.to(DEV).eval(), p


def _structs(enc, g, variant):
    enc._gemm_variant = variant
    dg = g.device_graph(DEV, False, get_bond_fdim())
    dg.use_on(torch.cuda.current_stream(DEV))
    gs = enc._graph_struct(dg)
    cfg = enc._config(False)
    params = tuple(t.detach().float() if t is not None else None for t in enc._param_tuple())
    pstruct, keep = enc._packed_params(gs, cfg, params, DEV)
    return gs, cfg, pstruct, keep, dg


def _forward(enc, g, variant, fill):
    """wdmpnn_forward on a workspace of the caller's, every byte ``fill`` before the call: (out, ws, structs)"""
    L = _native.lib()
    gs, cfg, pstruct, keep, dg = _structs(enc, g, variant)
    n = ctypes.c_size_t()
    _native.check(L.wdmpnn_workspace_bytes(ctypes.byref(gs), ctypes.byref(pstruct), ctypes.byref(cfg), ctypes.byref(n)),
                  'workspace')
    ws = torch.full((max(n.value, 256),), fill, dtype=torch.uint8, device=DEV)
    out = torch.full((gs.n_mols, enc.hidden_size), float('nan'), dtype=torch.float32, device=DEV)
    _native.check(L.wdmpnn_forward(ctypes.byref(gs), ctypes.byref(pstruct), ctypes.byref(cfg), ws.data_ptr(), n.value,
                                   out.data_ptr(), _native.current_stream(DEV)), 'forward')
    torch.cuda.synchronize()
    return out, ws, (gs, cfg, pstruct, keep, dg)


@pytest.mark.parametrize('depth', [2, 3])
@pytest.mark.parametrize('name', ['rows18', 'rows16', 'rows128', 'lone_atom'])
def test_stale_pair_rows_cannot_leak(name, depth):
    """Pair layers (variant 13: forced also for small blocks) on a workspace of zero bytes and of 0xFF bytes
    (stale pair rows read as fp16 NaN): bitwise equal, finite, and the oracle's at 1e-5.  Depth 2 is one layer
    (the last-layer instantiation, fed by the embed's pairs), depth 3 both instantiations."""
    g = _batch(name)
    args, enc, p = _encoder(300, depth)
    zero, _, _ = _forward(enc, g, _native.VARIANT_PAIRS, 0x00)
    ones, _, _ = _forward(enc, g, _native.VARIANT_PAIRS, 0xFF)
    assert torch.isfinite(zero).all() and torch.isfinite(ones).all()
    assert torch.equal(zero, ones)
    ref = mpn_ref.encoder_forward(p, g, args)
    assert golden_io.normwise(zero.cpu().numpy(), ref.numpy()) <= TOL


def _selects_pairs(hidden):
    """host-only: the forward workspace of the pair variant differs from the register-staged one's"""
    g = _batch('rows16')
    _, enc, _ = _encoder(hidden, 3)
    sizes = []
    for v in (_native.VARIANT_PAIRS, _native.VARIANT_STAGED):
        gs, cfg, pstruct, _, _ = _structs(enc, g, v)
        n = ctypes.c_size_t()
        _native.check(_native.lib().wdmpnn_workspace_bytes(ctypes.byref(gs), ctypes.byref(pstruct), ctypes.byref(cfg),
                                                           ctypes.byref(n)), 'workspace')
        sizes.append(n.value)
    return sizes[0] != sizes[1]


def test_smallest_pair_hidden_size():
    """The recorded layouts: hidden 64 runs no pair layers (its pair-variant workspace is the staged one's),
    300 does; by get_dims' rule (80 | Hk, Hk = 64 ceil(H / 64)) the smallest hidden size with pair layers is
    257, Hk 320 -- ten chunks, so no layout reaches nchunks <= NS - 1."""
    gold = json.load(open(GOLDEN))
    ws = lambda h, v: gold[f'polymer4|bond|codes|h{h}|d3|s0|b0|v{v}']['ws']  # noqa: E731
    assert ws(64, 13) == ws(64, 12) and ws(300, 13) != ws(300, 12)
    assert not _selects_pairs(256) and _selects_pairs(257)


@pytest.mark.parametrize('hidden', [257, 300])
def test_short_k_pairs_vs_oracle_and_staged(hidden):
    """The smallest hidden size with pair layers and hidden 300, on the 0xFF workspace: the oracle's at 1e-5
    normwise, the register-staged layers' (variant 12, untouched here) at 2e-6, and bitwise the zero-byte
    workspace's."""
    g = _batch('rows18')
    args, enc, p = _encoder(hidden, 3, activation='LeakyReLU', bias=True)
    ref = mpn_ref.encoder_forward(p, g, args).numpy()
    pairs, _, _ = _forward(enc, g, _native.VARIANT_PAIRS, 0xFF)
    pairs0, _, _ = _forward(enc, g, _native.VARIANT_PAIRS, 0x00)
    staged, _, _ = _forward(enc, g, _native.VARIANT_STAGED, 0xFF)
    e_ref = golden_io.normwise(pairs.cpu().numpy(), ref)
    e_stg = golden_io.normwise(pairs.cpu().numpy(), staged.cpu().numpy())
    print(f'hidden {hidden}: pairs vs oracle {e_ref:.3e}, pairs vs staged {e_stg:.3e}')
    assert torch.equal(pairs, pairs0)
    assert e_ref <= TOL
    assert e_stg <= 2e-6
