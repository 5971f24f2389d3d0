"""Atom-message graphs built on the device (wdmpnn.h ``wdmpnn_build_graph_atom``), host side: the two entry
points are declared, bound and exported under the unchanged ABI number, the size query and the refusals work
without a GPU, the static-offset layout the kernel writes -- restated here in NumPy from the batch's in-lists
-- gives back the host packer's gather lists once zero coefficients are dropped, and the command line takes
``--atom_messages``.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from chemprop_amd import _native, synthetic
from chemprop_amd.featurization import BatchMolGraph, Csr, _packer, _stage_bound, get_bond_fdim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1000, -1001, -1002


def batches():
    """(name, molecules): polymer 8, qm9 4, the edge cases of test_gpu_parity.test_blocked_atom_messages_edge_cases
    (empty and single-atom molecules, a hub) and the weight cases (hubs of degree 9 .. 16, zero bond weights)."""
    return [('polymer', synthetic.make_batch('polymer', 8, 3)), ('qm9', synthetic.make_batch('qm9', 4, 4)),
            ('edge', synthetic.edge_case_batch(9, star_leaves=20)), ('weights', synthetic.weight_case_batch(12))]


# ------------------------------------------------------------------------------------------------ the layout
def static_layout(g: BatchMolGraph):
    """The five gather lists of an atom-message graph as ``wdmpnn_build_graph_atom`` lays them out: every row a
    holds one entry per in-bond of a (zero coefficients kept), msg_gather one more -- the pad slots' entry
    (0, max_num_bonds - deg(a)), last, written even when 0 -- so row a starts at in_ptr[a] (msg_gather: + a), and
    the transposes are ``Csr.transpose`` of those.  From the batch's in-lists alone (``_in_ptr``, ``_in_idx``)."""
    V1 = g.n_atoms
    deg, ptr, j = g._deg[:V1], g._in_ptr[:V1 + 1], g._in_idx
    b2a, w = g._np['b2a'], g._np['w_bonds']
    src = b2a[j]
    ones = np.ones(len(j), np.float32)
    feat = Csr(ptr, j, ones)
    agg = Csr(ptr, src, w[src])
    rows = np.arange(V1, dtype=np.int64)
    m_ptr = ptr + np.arange(V1 + 1)
    m_idx = np.zeros(len(j) + V1, np.int64)
    m_coef = np.zeros(len(j) + V1, np.float32)
    at = np.arange(len(j)) + np.repeat(rows, deg)  # entry e of in(a) sits a entries further on
    m_idx[at], m_coef[at] = src, 1.0
    m_coef[m_ptr[1:] - 1] = g.max_num_bonds - deg  # (their index stays 0)
    msg = Csr(m_ptr, m_idx, m_coef)
    return {'feat': feat, 'msg': msg, 'agg': agg, 'msg_t': msg.transpose(V1), 'agg_t': agg.transpose(V1)}


def rows_without_zeros(c: Csr):
    """[(idx, coef) sequence per row] with the zero-coefficient entries removed."""
    out = []
    for r in range(c.rows):
        s = slice(int(c.ptr[r]), int(c.ptr[r + 1]))
        keep = c.coef[s] != 0
        out.append((c.idx[s][keep].tolist(), c.coef[s][keep].tolist()))
    return out


def host_lists(g: BatchMolGraph):
    """The host packer's lists for the same batch (featurization.BatchMolGraph.device_graph, atom messages)."""
    msg, feat = g.atom_message_gather()
    agg = g.atom_aggregate_gather(True)
    return {'feat': feat, 'msg': msg, 'agg': agg, 'msg_t': msg.transpose(g.n_atoms), 'agg_t': agg.transpose(g.n_atoms)}


@pytest.mark.parametrize('case', range(4))
def test_static_layout_restates_the_host_lists(case):
    name, mols = batches()[case]
    g = BatchMolGraph(mols, compact=False)
    assert g.n_atoms <= g.n_bonds  # (no atom id overruns w_bonds: the device build's domain)
    spec, host = static_layout(g), host_lists(g)
    for k in spec:
        assert rows_without_zeros(spec[k]) == rows_without_zeros(host[k]), k
        assert spec[k].rows == g.n_atoms
    V1, E = g.n_atoms, g.n_bonds - 1
    deg = g._deg[:V1]
    # entry counts: functions of the atom and bond counts alone
    assert [len(spec[k].idx) for k in ('feat', 'msg', 'agg', 'msg_t', 'agg_t')] == [E, E + V1, E, E + V1, E]
    assert np.array_equal(np.diff(spec['msg'].ptr), deg + 1) and np.array_equal(np.diff(spec['agg'].ptr), deg)
    assert np.array_equal(np.diff(spec['agg_t'].ptr), deg)  # (every pair: one in- and one out-bond per end)
    assert np.array_equal(np.diff(spec['msg_t'].ptr), np.concatenate([[V1], deg[1:]]))
    # row 0: the pad slots alone; msg_gather_t row 0: every atom's pad entry, in atom order
    assert (spec['msg'].idx[0], spec['msg'].coef[0]) == (0, g.max_num_bonds)
    assert np.array_equal(spec['msg_t'].idx[:V1], np.arange(V1))
    assert np.array_equal(spec['msg_t'].coef[:V1], (g.max_num_bonds - deg).astype(np.float32))
    # every offset follows from the block table: the bonds before a block are the in-bonds of the atoms before it
    blocks = g.molecule_blocks()
    for bs, bn, as_, an in blocks[:, :4].tolist():
        assert spec['feat'].ptr[as_] == bs - 1 and spec['agg_t'].ptr[as_] == bs - 1
        assert spec['msg'].ptr[as_] == bs - 1 + as_ and spec['msg_t'].ptr[as_] == V1 + bs - 1
        assert spec['feat'].ptr[as_ + an] == bs - 1 + bn
    if name == 'weights':  # the cases the kept zeros and the ELL width are about
        assert deg.max() > 8 and (spec['agg'].coef == 0).any() and (g.max_num_bonds - deg == 0).any()
        assert len(host['agg'].idx) < len(spec['agg'].idx)


def test_a_batch_with_more_atoms_than_bonds_keeps_the_host_error():
    """The readout's w_bonds[atom id] (mpn.py:128) overruns w_bonds there: the host path's IndexError stays."""
    rng = np.random.default_rng(0)
    g = BatchMolGraph([synthetic.single_atom_graph(rng) for _ in range(3)] + [synthetic.star_graph(rng, 1)])
    assert g.n_atoms > g.n_bonds and g._compact is not None
    with pytest.raises(IndexError, match='atom ids'):
        g.device_graph('cpu', True, get_bond_fdim(atom_messages=True))


# ------------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_declared_bound_and_exported():
    text = open(HEADER).read()
    assert '#define WDMPNN_ABI_VERSION 12' in text
    assert re.search(r'\bint wdmpnn_graph_bytes_atom\(const WdCompact \*c, size_t \*bytes\);', text)
    assert re.search(r'\bint wdmpnn_build_graph_atom\(const WdCompact \*c, void \*buffer, size_t bytes, WdGraph \*g,\s*'
                     r'int32_t max_num_bonds,\s*void \*stream\);', text)
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    L = _native.lib()
    assert _native.ABI_VERSION == 12 and L.wdmpnn_abi_version() == 12
    for fn in ('wdmpnn_graph_bytes_atom', 'wdmpnn_build_graph_atom'):
        assert fn in _native.EXPORTED_SYMBOLS and re.search(rf'\bT {fn}\b', out), fn
        assert getattr(L, fn).argtypes[0]._type_ is _native.WdCompact and getattr(L, fn).restype is ctypes.c_int
    assert L.wdmpnn_build_graph_atom.argtypes[3]._type_ is _native.WdGraph
    assert L.wdmpnn_build_graph_atom.argtypes[4] is ctypes.c_int32


def _compact_struct(g: BatchMolGraph, with_pointers: bool = False):
    """The WdCompact of a batch, host only: pointers are offsets into the staged image, never dereferenced."""
    extra = g._compact_extra or ()
    host = np.zeros(_stage_bound(g._compact + tuple(extra[:2])), np.uint8)
    info = _packer().compact_stage(*g._compact, *g._compact_dims, 64, host.ctypes.data, host.nbytes, *extra)
    _, (n_mols, n_atoms, n_bonds, n_blocks, nnz_msg, nnz_agg), off, total = info[:4]
    c = _native.WdCompact()
    c.n_mols, c.n_atoms, c.n_bonds, c.n_blocks = n_mols, n_atoms, n_bonds, n_blocks
    c.atom_fdim, c.bond_fdim = g._compact_dims
    c.nnz_msg, c.nnz_agg = nnz_msg, nnz_agg
    if with_pointers:
        c.mols, c.xn, c.atoms, c.pairs, c.blocks, c.block_nnz = (4096 + o for o in off)
    if extra:
        c.atom_extra_dim, c.bond_extra_dim = extra[2:]
        if with_pointers:
            c.atom_extra, c.bond_extra = (4096 + o for o in info[4])
    return c


def _sections(c) -> int:
    """Bytes of the arrays the atom-message graph holds (no alignment gaps): a lower bound of the buffer."""
    up = lambda x, m: -(-x // m) * m  # noqa: E731
    V1, E1, B, nblk = c.n_atoms, c.n_bonds, c.n_mols, c.n_blocks
    Vap, Rbp, lda, ldb = up(V1, 128), up(E1, 128), up(c.atom_fdim, 32), up(c.bond_fdim - c.atom_fdim, 32)
    rows = 4 * (Vap * lda + Rbp * ldb)
    planes = 6 * (Vap * lda + Rbp * ldb + 64 * nblk * lda + Vap * ldb)  # f_atoms, f_bonds, blocked f_atoms, the sums
    small = 4 * V1 + 3 * 4 * B + 4 * E1 + 32 * nblk + 4 * Rbp + 4 * Vap  # w_atoms, scope, b2revb, blocks, block rows
    ell = 2 * Vap * 8 * (1 + 4)
    E = E1 - 1
    csr = 5 * 4 * (V1 + 1) + 2 * 4 * (3 * (E + 8) + 2 * (E + V1 + 8))
    return rows + planes + small + ell + csr


def test_size_query_on_a_host_only_struct():
    L = _native.lib()
    sizes = []
    for b in (2, 8, 32):
        c = _compact_struct(BatchMolGraph(synthetic.make_batch('polymer', b, 3)))
        n = ctypes.c_size_t()
        assert L.wdmpnn_graph_bytes_atom(ctypes.byref(c), ctypes.byref(n)) == 0
        assert _sections(c) <= n.value <= _sections(c) + 40 * 256  # (+ the 256-byte alignment of its arrays)
        sizes.append(n.value)
        # the entry counts of the bond-mode lists are not read
        c.nnz_msg = c.nnz_agg = 0
        m = ctypes.c_size_t()
        assert L.wdmpnn_graph_bytes_atom(ctypes.byref(c), ctypes.byref(m)) == 0 and m.value == n.value
    assert sizes[0] < sizes[1] < sizes[2]
    wide = _compact_struct(BatchMolGraph(synthetic.with_extra_features(synthetic.make_batch('polymer', 8, 3), 4, 3, 1)))
    n = ctypes.c_size_t()
    assert L.wdmpnn_graph_bytes_atom(ctypes.byref(wide), ctypes.byref(n)) == 0
    assert wide.bond_fdim - wide.atom_fdim == 17 and _sections(wide) <= n.value
    assert L.wdmpnn_graph_bytes_atom(ctypes.byref(c), None) == ERR_ARG
    assert L.wdmpnn_graph_bytes_atom(None, ctypes.byref(n)) == ERR_ARG
    c.n_bonds += 1  # (bonds come in pairs)
    assert L.wdmpnn_graph_bytes_atom(ctypes.byref(c), ctypes.byref(n)) == ERR_SHAPE


def test_build_refuses_before_any_launch():
    """Short, misaligned or missing buffers and max_num_bonds < 1: refused on the host (no GPU here)."""
    L = _native.lib()
    c = _compact_struct(BatchMolGraph(synthetic.make_batch('polymer', 4, 3)), with_pointers=True)
    n = ctypes.c_size_t()
    assert L.wdmpnn_graph_bytes_atom(ctypes.byref(c), ctypes.byref(n)) == 0
    g = _native.WdGraph()
    buf = 1 << 20  # (an address-like number: 256-byte aligned, never dereferenced)
    assert L.wdmpnn_build_graph_atom(ctypes.byref(c), buf, n.value - 1, ctypes.byref(g), 4, None) == ERR_WORKSPACE
    assert L.wdmpnn_build_graph_atom(ctypes.byref(c), buf + 64, n.value, ctypes.byref(g), 4, None) == ERR_ARG
    assert L.wdmpnn_build_graph_atom(ctypes.byref(c), None, n.value, ctypes.byref(g), 4, None) == ERR_ARG
    assert L.wdmpnn_build_graph_atom(ctypes.byref(c), buf, n.value, None, 4, None) == ERR_ARG
    for bad in (0, -3):
        assert L.wdmpnn_build_graph_atom(ctypes.byref(c), buf, n.value, ctypes.byref(g), bad, None) == ERR_ARG
    c.blocks = None
    assert L.wdmpnn_build_graph_atom(ctypes.byref(c), buf, n.value, ctypes.byref(g), 4, None) == ERR_ARG
    assert g.n_atoms == 0 and not g.f_atoms  # (nothing was handed out)


# ------------------------------------------------------------------------------------------------ command line
BASE = ['--data_path', 'd.csv', '--graphs_path', 'g.npz', '--save_dir', 'out']
PRED = ['--test_path', 't.csv', '--graphs_path', 'g.npz', '--preds_path', 'p.csv', '--checkpoint_path', 'm.pt']


def test_cli_arguments(capsys):
    from chemprop_amd import cli
    assert cli.parse_args(BASE).atom_messages is False
    a = cli.parse_args(BASE + ['--atom_messages', '--resident_graphs', '--bias'])
    assert a.atom_messages is True and a.resident_graphs and a.bias
    with pytest.raises(SystemExit) as e:  # an argument error (usage + one line), not a traceback
        cli.parse_args(BASE + ['--atom_messages', '--undirected'])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert '--atom_messages cannot be combined with --undirected' in err and 'Traceback' not in err
    # prediction reads the mode from the checkpoint: no such flag there
    for parse in (cli.parse_predict_args, cli.parse_fingerprint_args):
        with pytest.raises(SystemExit):
            parse(PRED + ['--atom_messages'])
        assert 'unrecognized arguments: --atom_messages' in capsys.readouterr().err
    assert not hasattr(cli.parse_predict_args(PRED), 'atom_messages')


def test_checkpoint_args_carry_the_flag(tmp_path):
    """The flag is a TrainArgs field: save_checkpoint stores it, load_checkpoint rebuilds an atom-message model."""
    import torch
    from chemprop_amd import TrainArgs, cli
    from chemprop_amd.model import MoleculeModel
    args = TrainArgs(hidden_size=32, depth=2, atom_messages=True, dataset_type='regression', num_tasks=1)
    cli.set_feature_sizes(args)
    model = MoleculeModel(args)
    path = str(tmp_path / 'm.pt')
    cli.save_checkpoint(path, model, args=args)
    assert torch.load(path, weights_only=True)['args']['atom_messages'] is True
    enc = cli.load_checkpoint(path).encoder.encoder[0]
    assert enc.atom_messages and enc.bond_fdim == get_bond_fdim(atom_messages=True)
    assert tuple(enc.W_h.weight.shape) == (32, 32 + enc.bond_fdim)
