"""Resident graph tables (chemprop_amd.graph_table, wdmpnn.h "Resident graph tables"), host side: the plan made
from a table's per-molecule sizes equals ``compact_stage``'s for the assembled batch, the index and the table
refuse what they must, the new entry point is declared, exported and laid out as its ctypes struct, and the CLI
takes the flag.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import graph_table_cases as cases
from chemprop_amd import _native, synthetic
from chemprop_amd.cli import parse_args
from chemprop_amd.featurization import BatchMolGraph, _packer
from chemprop_amd.graph_table import GraphTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')


@pytest.fixture(scope='module')
def table():
    return GraphTable(cases.pool(), 'cpu')


def _draws():
    """(ids, block_target) of 320 seeded batches of 1, 2, 50 and 200 molecules.  Every fourth batch draws from
    the tiny molecules only (no atoms / one atom): 200 of those are cut by the 64-molecule limit and the 64-atom
    limit, the others by the bond limit and, at 50 molecules and below, by the ``block_target`` share."""
    rng = np.random.default_rng(2024)
    n = len(cases.pool())
    out = []
    for k in range(320):
        size = (1, 2, 50, 200)[k % 4]
        if k % 16 >= 12:
            ids = rng.choice([cases.ONE_ATOM, cases.EMPTY], size=size, p=[0.3, 0.7])
        else:
            ids = rng.integers(0, n, size=size)
        out.append((ids, (64, 1, 7)[k % 3]))
    return out


def test_planner_equals_compact_plan(table):
    pool = cases.pool()
    img, small = np.zeros(1 << 20, np.uint8), np.zeros(1 << 16, np.uint8)
    seen_mol_cut = seen_share_cut = False
    for ids, target in _draws():
        g = BatchMolGraph([pool[i] for i in ids])
        assert g._compact is not None, g._compact_why
        want = _packer().compact_stage(*g._compact, *g._compact_dims, target, img.ctypes.data, img.nbytes)
        got = _packer().compact_plan(np.ascontiguousarray(table.sizes[ids]), target, small.ctypes.data, small.nbytes)
        copied, counts, off, total = want
        assert copied and got[0]
        assert got[1] == counts and got[2] == off and got[3] == total
        h_mols, h_blocks, h_nnz = got[4]
        B, nblk = counts[0], counts[3]
        assert bytes(small[h_mols:h_mols + 16 * B]) == bytes(img[off[0]:off[0] + 16 * B])
        assert bytes(small[h_blocks:h_blocks + 32 * nblk]) == bytes(img[off[4]:off[4] + 32 * nblk])
        assert bytes(small[h_nnz:h_nnz + 8 * nblk]) == bytes(img[off[5]:off[5] + 8 * nblk])
        assert h_nnz - h_blocks == off[5] - off[4]  # the pair uploads as one copy
        blocks = img[off[4]:off[4] + 32 * nblk].view(np.int32).reshape(-1, 8)
        assert got[5] == (int(blocks[:, 1].max()), int(blocks[:, 3].max()))
        seen_mol_cut |= bool(((blocks[:, 5] - blocks[:, 4] == 64) & (blocks[:, 3] < 64) & (blocks[:, 1] < 128)).any())
        seen_share_cut |= target == 64 and nblk > 1 and int(blocks[:, 1].max()) < 112 and int(blocks[:, 3].max()) < 40
    assert seen_mol_cut and seen_share_cut  # the draws reached both rules


def test_table_keeps_each_molecules_own_entries(table):
    """nnz_msg / nnz_agg of a molecule in the table = those of the molecule planned alone."""
    for i, m in enumerate(cases.pool()):
        g = BatchMolGraph([m])
        info = _packer().compact_stage(*g._compact, *g._compact_dims, 64, 0, 0)
        assert tuple(table.sizes[i]) == (m.n_atoms, m.n_bonds, info[1][4], info[1][5]), i


def test_table_batch_decodes_the_list_paths_tables(table):
    """A host attribute read on a table batch decodes the same tables as the list path's batch."""
    ids = [cases.BONDS_128, cases.ONE_ATOM, 7, 7, cases.WEIGHTS, cases.ATOMS_64]
    a = table.rows(ids).batch()
    b = BatchMolGraph([cases.pool()[i] for i in ids])
    assert '_np' not in a.__dict__ and '_compact' not in a.__dict__  # nothing decoded yet
    assert (a.n_atoms, a.n_bonds, a.a_scope, a.b_scope) == (b.n_atoms, b.n_bonds, b.a_scope, b.b_scope)
    assert np.array_equal(np.float32(a.degree_of_polym), np.float32(b.degree_of_polym))
    assert all(bytes(x) == bytes(y) for x, y in zip(a._compact, b._compact))
    for attr in ('f_atoms', 'f_bonds', 'w_atoms', 'w_bonds', 'b2a', 'b2revb', 'a2b'):
        assert np.array_equal(getattr(a, attr).numpy(), getattr(b, attr).numpy()), attr
    assert a.max_num_bonds == b.max_num_bonds


@pytest.mark.parametrize('bad,names', [([0, -1, 2], 'graph row -1 at position 1'),
                                       ([3, 1, None], None),  # (None stands for N, filled in below)
                                       ([0.0, 1.0], 'flat sequence of ints'),
                                       ([[0, 1], [2, 3]], 'flat sequence of ints')])
def test_index_validates_positions(table, bad, names):
    n = len(table)
    if names is None:
        bad, names = [3, 1, n], f'graph row {n} at position 2 is outside the table of {n} rows'
    with pytest.raises(ValueError, match=re.escape(names)):
        table.index(bad)
    ok = table.index([n - 1, 0, 0])
    assert len(ok) == 3 and len(ok[1:]) == 2
    with pytest.raises(TypeError):
        ok[::2]


def test_table_refuses_what_cannot_be_compact():
    mols = synthetic.make_batch('polymer', 5, 1)
    mols[3].f_atoms[2][5] = 0.5  # not one-hot
    with pytest.raises(ValueError, match='molecule 3 does not encode compactly: atom row not one-hot coded'):
        GraphTable(mols, 'cpu')
    rng = np.random.default_rng(0)
    mols = synthetic.make_batch('qm9', 3, 1)
    mols.insert(2, synthetic._build(rng, 65, {(i, i + 1) for i in range(64)}, [], [1.0] * 65, 1.0))
    with pytest.raises(ValueError, match='molecule 2 exceeds a molecule block: 65 atoms, 128 directed bonds'):
        GraphTable(mols, 'cpu')
    rows = [(a, b) for a, b in zip(synthetic.make_batch('polymer', 3, 2), synthetic.make_batch('qm9', 3, 3))]
    rows[1][1].f_bonds[1][140] = 2.0  # bond column not binary
    with pytest.raises(ValueError, match='molecule 1 of row 1 does not encode compactly: bond columns'):
        GraphTable(rows, 'cpu')
    with pytest.raises(ValueError, match='no molecules'):
        GraphTable([], 'cpu')


def test_table_of_rows_numbers_every_slot():
    a, b = synthetic.make_batch('polymer', 4, 2), synthetic.make_batch('qm9', 4, 3)
    t = GraphTable(list(zip(a, b)), 'cpu')
    assert (len(t), t.n_slots, len(t.sizes)) == (4, 2, 8)
    rows = t.rows([2, 0])
    sb = rows.slot_batch(shared=True)
    assert [n for _, n in sb[0].a_scope] == [a[2].n_atoms, a[0].n_atoms]
    assert [n for _, n in sb[1].a_scope] == [b[2].n_atoms, b[0].n_atoms]
    assert [n for _, n in sb.merged.a_scope] == [a[2].n_atoms, a[0].n_atoms, b[2].n_atoms, b[0].n_atoms]
    assert sb.n_rows == 2 and rows.slot_batch().merged is None
    want = BatchMolGraph([a[2], a[0], b[2], b[0]])
    assert all(bytes(x) == bytes(y) for x, y in zip(sb.merged._compact, want._compact))


# ------------------------------------------------------------------------------------------------ ABI
def test_entry_point_is_declared_bound_and_exported():
    assert re.search(r'\bint wdmpnn_gather_compact\(const WdGatherCompact \*g, void \*stream\);', open(HEADER).read())
    assert 'wdmpnn_gather_compact' in _native.EXPORTED_SYMBOLS
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r'\bT wdmpnn_gather_compact\b', out)
    assert _native.ABI_VERSION == 12 and _native.lib().wdmpnn_abi_version() == 12


def test_struct_layout_matches_the_header(tmp_path):
    S = _native.WdGatherCompact
    names = [n for n, _ in S._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wdmpnn.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(WdGatherCompact), sizeof(WdAtomCode), sizeof(WdBondPair));\n' +
                   ''.join(f'  printf(" %zu", offsetof(WdGatherCompact, {n}));\n' for n in names) +
                   '  printf("\\n"); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC', 'gcc'), '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert c == [ctypes.sizeof(S), 16, 16] + [getattr(S, n).offset for n in names]


def _fake(**kw):
    """A WdGatherCompact of made-up addresses (never dereferenced: every call below is refused, or a no-op)."""
    g = _native.WdGatherCompact()
    g.n_mols, g.n_rows, g.n_slots, g.slot0 = 4, 4, 1, 0
    for n in ('t_atoms', 't_pairs', 't_xn', 't_first', 'ids', 'mols', 'xn', 'atoms', 'pairs'):
        setattr(g, n, 4096)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


ERR_ARG, ERR_SHAPE = -1000, -1001
POINTERS = ['t_atoms', 't_pairs', 't_xn', 't_first', 'ids', 'mols', 'xn', 'atoms', 'pairs']


@pytest.mark.parametrize('kw,rc', [({p: None}, ERR_ARG) for p in POINTERS] + [
    (dict(n_mols=-1), ERR_SHAPE), (dict(n_rows=-1), ERR_SHAPE), (dict(n_rows=0), ERR_SHAPE),
    (dict(n_slots=0), ERR_SHAPE), (dict(slot0=-1), ERR_SHAPE), (dict(slot0=1), ERR_SHAPE),
    (dict(n_rows=3), ERR_SHAPE), (dict(n_mols=8), ERR_SHAPE), (dict(atoms=4104), ERR_ARG)])
def test_gather_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    got = L.wdmpnn_gather_compact(ctypes.byref(_fake(**kw)), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert 'gather_compact' in L.wdmpnn_last_error().decode()


def test_gather_null_struct_and_empty_batch():
    L = _native.lib()
    assert L.wdmpnn_gather_compact(None, None) == ERR_ARG
    assert L.wdmpnn_gather_compact(ctypes.byref(_fake(n_mols=0)), None) == 0
    empty = _native.WdGatherCompact()  # every pointer NULL: still a no-op
    assert L.wdmpnn_gather_compact(ctypes.byref(empty), None) == 0


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_accepts_resident_graphs(tmp_path):
    base = ['--data_path', 'd.csv', '--graphs_path', 'g.pkl', '--save_dir', str(tmp_path)]
    assert parse_args(base).resident_graphs is False
    assert parse_args(base + ['--resident_graphs']).resident_graphs is True
