"""Atom descriptors natively, the host side (no GPU): the four entry points are declared, bound and exported with
the ABI still 12 and their structs laid out as a C compiler lays out the header's; every refusal happens before a
launch; the table, its index and the binding to a ``BatchMolGraph`` are validated on the host; the ``.npz`` loader
and the scaler are the reference's; the CLI refusals; the checkpoint keeps the atom descriptor scaler."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from chemprop_amd import TrainArgs, _native, cli, synthetic
from chemprop_amd.atom_descriptors import (AtomDescriptorIndex, AtomDescriptorRows, AtomDescriptorTable,
                                           is_device_descriptors)
from chemprop_amd.featurization import BatchMolGraph
from chemprop_amd.model import MoleculeModel
from chemprop_amd.mpn import MPNEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'atom_descriptors', 'atom_descriptors_ref.npz')
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1000, -1001, -1003
FUNCS = {'wdmpnn_desc_join': 'WdDescJoin', 'wdmpnn_desc_layer': 'WdDescLayer',
         'wdmpnn_desc_layer_backward': 'WdDescLayerBackward', 'wdmpnn_desc_rows': 'WdDescRows'}


def test_header_binding_and_library_agree(tmp_path):
    text = open(HEADER).read()
    assert '#define WDMPNN_ABI_VERSION 12' in text and '#define WD_DESC_MAX_WIDTH 4096' in text
    assert _native.ABI_VERSION == 12 and _native.DESC_MAX_WIDTH == 4096
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    L = _native.lib()
    assert L.wdmpnn_abi_version() == 12
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wdmpnn.h"', 'int main(void) {']
    want = []
    for fn, st in FUNCS.items():
        assert re.search(r'\bint\s+%s\s*\(\s*const\s+%s\s*\*' % (fn, st), text), fn
        assert fn in _native.EXPORTED_SYMBOLS and re.search(r'\bT %s\b' % fn, out), fn
        S = getattr(_native, st)
        assert getattr(L, fn).argtypes[0]._type_ is S and getattr(L, fn).restype is ctypes.c_int
        lines.append(f'  printf("%zu ", sizeof({st}));')
        want.append(ctypes.sizeof(S))
        for n, _ in S._fields_:
            lines.append(f'  printf("%zu ", offsetof({st}, {n}));')
            want.append(getattr(S, n).offset)
    lines += ['  return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC', 'gcc'), '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


# made-up addresses, never dereferenced: every call below is refused, or a no-op, on the host
P = 4096


def _graph(B=4, n_atoms=20, **kw):
    g = _native.WdGraph()
    g.n_mols, g.n_atoms = B, n_atoms
    g.mol_start, g.mol_size, g.w_atoms, g.degree_of_polym = (kw.get(k, P) for k in
                                                           ('mol_start', 'mol_size', 'w_atoms', 'degree_of_polym'))
    return g


def _join(g='default', **kw):
    j = _native.WdDescJoin()
    keep = _graph(**{k: kw.pop(k) for k in list(kw) if k in ('B', 'n_atoms', 'mol_start', 'mol_size', 'w_atoms',
                                                               'degree_of_polym')})
    j.g = ctypes.pointer(keep) if g == 'default' else None
    v = dict(H=48, d=5, emb=P, ld_emb=48, table=P, ld_table=5, table_rows=100, row0=P, aggregation=0,
             aggregation_norm=100.0, x=P, ld_x=54)
    v.update(kw)
    for k, val in v.items():
        setattr(j, k, val)
    return j, keep


@pytest.mark.parametrize('kw,rc', [
    (dict(g=None), ERR_ARG), (dict(B=-1), ERR_SHAPE), (dict(H=0), ERR_SHAPE), (dict(d=0), ERR_SHAPE),
    (dict(d=-3), ERR_SHAPE), (dict(table_rows=-1), ERR_SHAPE), (dict(ld_emb=47), ERR_SHAPE),
    (dict(ld_table=4), ERR_SHAPE), (dict(ld_x=53), ERR_SHAPE), (dict(aggregation=3), ERR_SHAPE),
    (dict(aggregation=-1), ERR_SHAPE), (dict(H=4092, ld_emb=4092, ld_x=5000), ERR_UNSUPPORTED),
    (dict(emb=None), ERR_ARG), (dict(table=None), ERR_ARG), (dict(row0=None), ERR_ARG), (dict(x=None), ERR_ARG),
    (dict(mol_start=None), ERR_ARG), (dict(mol_size=None), ERR_ARG), (dict(w_atoms=None), ERR_ARG),
    (dict(degree_of_polym=None), ERR_ARG)])
def test_desc_join_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    j, keep = _join(**kw)
    got = L.wdmpnn_desc_join(ctypes.byref(j), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()


def _layer(**kw):
    l = _native.WdDescLayer()
    v = dict(B=4, Hd=53, x=P, ld_x=54, W_d=P, b_d=P, y=P, ld_y=53)
    v.update(kw)
    for k, val in v.items():
        setattr(l, k, val)
    return l


@pytest.mark.parametrize('kw,rc', [
    (dict(B=-1), ERR_SHAPE), (dict(Hd=0), ERR_SHAPE), (dict(ld_x=53), ERR_SHAPE), (dict(ld_y=52), ERR_SHAPE),
    (dict(Hd=4097, ld_x=4098, ld_y=4097), ERR_UNSUPPORTED), (dict(x=None), ERR_ARG), (dict(W_d=None), ERR_ARG),
    (dict(y=None), ERR_ARG)])
def test_desc_layer_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    got = L.wdmpnn_desc_layer(ctypes.byref(_layer(**kw)), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    with pytest.raises((ValueError, NotImplementedError)):
        _native.check(got, 'desc layer')


def _layer_bwd(**kw):
    l = _native.WdDescLayerBackward()
    v = dict(B=4, H=48, Hd=53, dy=P, ld_dy=53, x=P, ld_x=54, W_d=P, dW_d=P, db_d=P, demb=P, ld_demb=48)
    v.update(kw)
    for k, val in v.items():
        setattr(l, k, val)
    return l


@pytest.mark.parametrize('kw,rc', [
    (dict(B=-1), ERR_SHAPE), (dict(H=0), ERR_SHAPE), (dict(Hd=47), ERR_SHAPE), (dict(ld_dy=52), ERR_SHAPE),
    (dict(ld_x=53), ERR_SHAPE), (dict(ld_demb=47), ERR_SHAPE),
    (dict(Hd=4097, ld_dy=4097, ld_x=4098), ERR_UNSUPPORTED), (dict(dy=None), ERR_ARG), (dict(x=None), ERR_ARG),
    (dict(W_d=None), ERR_ARG)])
def test_desc_layer_backward_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    got = L.wdmpnn_desc_layer_backward(ctypes.byref(_layer_bwd(**kw)), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()


def _rows(g='default', **kw):
    r = _native.WdDescRows()
    keep = _graph(**{k: kw.pop(k) for k in list(kw) if k in ('B', 'n_atoms', 'mol_start', 'mol_size')})
    r.g = ctypes.pointer(keep) if g == 'default' else None
    v = dict(d=5, table=P, ld_table=5, table_rows=100, row0=P, atom_desc=P, rows=128, ld=32)
    v.update(kw)
    for k, val in v.items():
        setattr(r, k, val)
    return r, keep


@pytest.mark.parametrize('kw,rc', [
    (dict(g=None), ERR_ARG), (dict(B=-1), ERR_SHAPE), (dict(d=0), ERR_SHAPE), (dict(table_rows=-1), ERR_SHAPE),
    (dict(ld_table=4), ERR_SHAPE), (dict(rows=127), ERR_SHAPE), (dict(n_atoms=129), ERR_SHAPE),
    (dict(ld=31), ERR_SHAPE), (dict(d=33), ERR_SHAPE), (dict(n_atoms=0), ERR_SHAPE), (dict(table=None), ERR_ARG),
    (dict(row0=None), ERR_ARG), (dict(atom_desc=None), ERR_ARG), (dict(mol_start=None), ERR_ARG),
    (dict(mol_size=None), ERR_ARG)])
def test_desc_rows_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    r, keep = _rows(**kw)
    got = L.wdmpnn_desc_rows(ctypes.byref(r), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()


def test_no_rows_is_a_no_op_and_null_structs_are_refused():
    L = _native.lib()
    j, k1 = _join(B=0, emb=None, table=None, row0=None, x=None)
    assert L.wdmpnn_desc_join(ctypes.byref(j), None) == 0
    assert L.wdmpnn_desc_layer(ctypes.byref(_layer(B=0, x=None, W_d=None, y=None)), None) == 0
    assert L.wdmpnn_desc_layer_backward(ctypes.byref(_layer_bwd(B=0, dy=None, x=None, W_d=None)), None) == 0
    r, k2 = _rows(B=0, table=None, row0=None, atom_desc=None)
    assert L.wdmpnn_desc_rows(ctypes.byref(r), None) == 0
    for fn in FUNCS:
        assert getattr(L, fn)(None, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------
MOLS = synthetic.make_batch('polymer', 4, 3)


def test_table_and_index_are_validated_on_the_host():
    desc = synthetic.random_descriptors(MOLS, 3, 1)
    table = AtomDescriptorTable(desc, 'cpu')
    assert len(table) == 4 and table.width == 3 and table.data.dtype == torch.float32
    assert table.n_rows == sum(g.n_atoms for g in MOLS)
    assert table.offsets.tolist() == np.concatenate([[0], np.cumsum([g.n_atoms for g in MOLS])]).tolist()
    for bad in ([-1], [4], [0, 2, 4], [1 << 40]):
        with pytest.raises(ValueError):
            table.index(bad)
        with pytest.raises(ValueError):
            table.rows(bad)
    with pytest.raises(ValueError):
        table.index([0.5, 1.0])
    idx = table.index([3, 0, 0, 2])
    assert isinstance(idx, AtomDescriptorIndex) and len(idx) == 4
    rows = idx[1:3]
    assert isinstance(rows, AtomDescriptorRows) and len(rows) == 2 and rows.width == 3
    assert rows._row0.dtype == torch.int64 and rows._row0.tolist() == [0, 0]
    assert idx[:]._row0.tolist() == [int(table.offsets[3]), 0, 0, int(table.offsets[2])]
    assert len(table.rows([])) == 0
    with pytest.raises(TypeError):
        AtomDescriptorIndex(table, torch.tensor([9]), np.array([1]))
    with pytest.raises(TypeError):
        AtomDescriptorRows(table, torch.tensor([9]), np.array([1]))
    with pytest.raises(TypeError):
        idx[::2]
    with pytest.raises(TypeError):
        idx[torch.tensor([0])]
    assert is_device_descriptors(rows) and not is_device_descriptors(desc)
    # the arrays of the batch come back as the list path takes them
    back = table.rows([2, 1]).to_list()
    assert np.array_equal(back[0], desc[2]) and np.array_equal(back[1], desc[1])
    # unequal widths, and what is no [n_atoms][d] array
    with pytest.raises(ValueError, match='molecule 1'):
        AtomDescriptorTable([np.zeros((3, 2)), np.zeros((2, 3))], 'cpu')
    for bad in ([np.zeros(3)], [np.zeros((3, 0))], [np.array([['a']])], []):
        with pytest.raises(ValueError):
            AtomDescriptorTable(bad, 'cpu')


def test_table_scales_and_casts_as_the_list_path_does():
    rng = np.random.default_rng(0)
    raw = [rng.standard_normal((n, 4)) * 1e3 for n in (3, 1, 5)]
    sc = cli.StandardScaler(replace_nan_token=0).fit(np.vstack(raw))
    table = AtomDescriptorTable(raw, 'cpu', sc)
    # data.py:432-478 scales per molecule in float64; mpn.py:77-79 then casts the stacked rows to float32
    want = torch.from_numpy(np.concatenate([sc.transform(a) for a in raw], axis=0)).float()
    assert torch.equal(table.data, want)
    assert torch.equal(AtomDescriptorTable(raw, 'cpu').data, torch.from_numpy(np.concatenate(raw)).float())


def test_binding_rows_to_a_graph():
    desc = synthetic.random_descriptors(MOLS, 3, 1)
    graph = BatchMolGraph(MOLS)
    table = AtomDescriptorTable(desc, 'cpu')
    table.rows([0, 1, 2, 3]).bind(graph)
    if len({g.n_atoms for g in MOLS}) > 1:
        order = sorted(range(4), key=lambda k: MOLS[k].n_atoms)
        swapped = [order[-1]] + [k for k in range(1, 4)]
        if MOLS[swapped[0]].n_atoms != MOLS[0].n_atoms:
            with pytest.raises(ValueError, match='number of atoms is different'):
                table.rows(swapped).bind(graph)
    with pytest.raises(ValueError, match='number of atoms is different'):
        table.rows([0, 1, 2]).bind(graph)
    short = [desc[0][:-1]] + desc[1:]
    with pytest.raises(ValueError, match='number of atoms is different'):
        AtomDescriptorTable(short, 'cpu').rows(range(4)).bind(graph)

    class Empty:  # a graph whose second molecule has no atoms
        a_scope = [(1, 2), (3, 0)]
    with pytest.raises(RuntimeError, match='empty molecule'):
        AtomDescriptorTable([np.zeros((2, 3)), np.zeros((0, 3))], 'cpu').rows([0, 1]).bind(Empty())
    # an encoder refuses rows it cannot take before anything is launched
    enc = MPNEncoder(TrainArgs(hidden_size=48, device=torch.device('cpu')), 133, 147)
    with pytest.raises(ValueError, match='no atom_descriptors_layer'):
        enc(graph, table.rows(range(4)))
    enc = MPNEncoder(TrainArgs(hidden_size=48, atom_descriptors='descriptor', atom_descriptors_size=5,
                               device=torch.device('cpu')), 133, 147)
    with pytest.raises(ValueError, match='descriptors per atom'):
        enc(graph, table.rows(range(4)))
    with pytest.raises(TypeError):
        enc(graph, np.zeros((3, 3)))


# ---------------------------------------------------------------------------------------------------
# the loader, the scaler, the CLI, the checkpoint
# ---------------------------------------------------------------------------------------------------
def test_npz_loader_order_and_errors(tmp_path):
    desc = synthetic.random_descriptors(MOLS, 3, 2)
    desc[1][0, 2] = np.nan
    path = str(tmp_path / 'd.npz')
    # file order, not key order: 'm9' is written first and sorts last
    np.savez(path, **{'m9': desc[0], 'm1': desc[1], 'm5': desc[2], 'm0': desc[3]})
    got = cli.load_atom_descriptors(path, MOLS)
    assert len(got) == 4 and all(a.dtype == np.float64 for a in got)
    assert np.array_equal(got[0], desc[0].astype(np.float64)) and np.array_equal(got[3], desc[3].astype(np.float64))
    assert got[1][0, 2] == 0.0 and not np.isnan(got[1]).any()  # NaN -> 0 at load (data.py:133-135)
    with pytest.raises(ValueError, match='3 descriptor arrays for 4'):
        np.savez(path, a=desc[0], b=desc[1], c=desc[2])
        cli.load_atom_descriptors(path, MOLS)
    with pytest.raises(ValueError, match='array 2'):
        np.savez(path, a=desc[0], b=desc[1], c=desc[2][:, :2], d=desc[3])
        cli.load_atom_descriptors(path, MOLS)
    with pytest.raises(ValueError, match='array 1 has'):
        np.savez(path, a=desc[0], b=desc[1][:-1], c=desc[2], d=desc[3])
        cli.load_atom_descriptors(path, MOLS)
    with pytest.raises(ValueError, match='array 3'):
        np.savez(path, a=desc[0], b=desc[1], c=desc[2], d=desc[3].reshape(-1))
        cli.load_atom_descriptors(path, MOLS)
    for ext, why in (('.pkl', 'pandas'), ('.sdf', 'RDKit'), ('.csv', '.npz')):
        with pytest.raises(ValueError, match=why):
            cli.load_atom_descriptors(str(tmp_path / ('d' + ext)), MOLS)


def test_scaler_equals_the_reference_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    raw, sizes = z['scaler_raw'], z['scaler_sizes']
    assert np.isnan(raw).any()
    mols, o = [], 0
    for n in sizes:
        mols.append(raw[o:o + n])
        o += n
    train_idx = z['scaler_train_idx'].tolist()
    loaded = [np.where(np.isnan(a), 0.0, a) for a in mols]  # (the loader's NaN -> 0)
    scaled, sc = cli.scale_atom_descriptors(loaded, train_idx)
    assert np.allclose(sc.means, z['scaler_means'], rtol=1e-12, atol=1e-12)
    assert np.allclose(sc.stds, z['scaler_stds'], rtol=1e-12, atol=0)
    assert (np.asarray(sc.stds) == 1.0).any()  # the zero-variance column keeps std 1
    assert np.allclose(np.concatenate(scaled), z['scaler_transformed'], rtol=1e-12, atol=1e-12)
    same, none = cli.scale_atom_descriptors(loaded, train_idx, no_atom_descriptor_scaling=True)
    assert none is None and all(np.array_equal(a, b) for a, b in zip(same, loaded))


BASE = ['--data_path', 'd.csv', '--graphs_path', 'g.npz', '--save_dir', 'out']


def test_cli_arguments_and_refusals():
    a = cli.parse_args(BASE)
    assert a.atom_descriptors is None and a.atom_descriptors_path is None and a.no_atom_descriptor_scaling is False
    a = cli.parse_args(BASE + ['--atom_descriptors', 'descriptor', '--atom_descriptors_path', 'd.npz',
                               '--no_atom_descriptor_scaling'])
    assert (a.atom_descriptors, a.atom_descriptors_path, a.no_atom_descriptor_scaling) == ('descriptor', 'd.npz', True)
    with pytest.raises(ValueError, match='featuris'):
        cli.parse_args(BASE + ['--atom_descriptors', 'feature', '--atom_descriptors_path', 'd.npz'])
    with pytest.raises(ValueError, match='pandas'):
        cli.parse_args(BASE + ['--atom_descriptors', 'descriptor', '--atom_descriptors_path', 'd.pkl'])
    with pytest.raises(ValueError, match='RDKit'):
        cli.parse_args(BASE + ['--atom_descriptors', 'descriptor', '--atom_descriptors_path', 'd.sdf'])
    with pytest.raises(ValueError, match='without --atom_descriptors'):
        cli.parse_args(BASE + ['--atom_descriptors_path', 'd.npz'])
    with pytest.raises(ValueError, match='needs --atom_descriptors_path'):
        cli.parse_args(BASE + ['--atom_descriptors', 'descriptor'])
    pred = ['--test_path', 't.csv', '--graphs_path', 'g.npz', '--preds_path', 'p.csv', '--checkpoint_path', 'm.pt']
    assert cli.parse_predict_args(pred).atom_descriptors_path is None
    assert cli.parse_predict_args(pred + ['--atom_descriptors_path', 'd.npz']).atom_descriptors_path == 'd.npz'
    assert cli.parse_fingerprint_args(pred + ['--atom_descriptors_path', 'd.npz']).atom_descriptors_path == 'd.npz'
    with pytest.raises(ValueError, match='pandas'):
        cli.parse_predict_args(pred + ['--atom_descriptors_path', 'd.pkl'])
    t = TrainArgs()
    assert t.atom_descriptors_path is None and t.no_atom_descriptor_scaling is False


def test_checkpoint_round_trips_the_atom_descriptor_scaler(tmp_path):
    args = TrainArgs(hidden_size=48, atom_descriptors='descriptor', atom_descriptors_size=3,
                     atom_descriptors_path='d.npz', no_atom_descriptor_scaling=False, device=torch.device('cpu'))
    model = MoleculeModel(args)
    sc = cli.StandardScaler(np.array([1.5, -2.0, 0.25]), np.array([2.0, 1.0, 0.5]), replace_nan_token=0)
    path = str(tmp_path / 'm.pt')
    cli.save_checkpoint(path, model, None, None, args, atom_descriptor_scaler=sc)
    state = torch.load(path, weights_only=True)
    assert state['atom_descriptor_scaler'] == {'means': [1.5, -2.0, 0.25], 'stds': [2.0, 1.0, 0.5]}
    assert state['args']['atom_descriptors'] == 'descriptor' and state['args']['atom_descriptors_size'] == 3
    assert state['args']['atom_descriptors_path'] == 'd.npz' and state['args']['no_atom_descriptor_scaling'] is False
    back = cli.load_scalers(path)[2]
    assert np.array_equal(back.means, sc.means) and np.array_equal(back.stds, sc.stds) and back.replace_nan_token == 0
    again = cli.load_checkpoint(path, 'cpu')
    assert again.encoder.atom_descriptors == 'descriptor'
    assert again.encoder.encoder[0].atom_descriptors_layer.in_features == 51
    # the default stays None
    cli.save_checkpoint(path, model, None, None, args)
    assert torch.load(path, weights_only=True)['atom_descriptor_scaler'] is None
