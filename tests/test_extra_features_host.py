"""Extra atom / bond features (wdmpnn.h "Compact graphs": WdCompact.atom_extra / bond_extra), host side: the
compact encoder splits widened rows into codes plus two dense sections and round-trips them bit for bit through
the staged image, refuses what it must with a reason, the grown structs agree between the header, ctypes and
the library under the unchanged ABI number, and the resident table and multi-molecule batches refuse extras.
Nothing here needs a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from chemprop_amd import _native, synthetic
from chemprop_amd.featurization import BatchMolGraph, _packer, _stage_bound
from chemprop_amd.graph_table import GraphTable
from chemprop_amd.slots import SlotBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')
DIMS = [(1, 0), (0, 1), (3, 2), (13, 0), (7, 7), (64, 64)]


def _mols(da, db, seed=5):
    base = synthetic.make_batch('polymer', 3, seed) + synthetic.edge_case_batch(seed + 1, star_leaves=12)
    return synthetic.with_extra_features(base, da, db, seed)


def test_with_extra_features_layout_and_special_values():
    base = synthetic.make_batch('polymer', 3, 5)
    wide = synthetic.with_extra_features(base, 3, 2, 5)
    again = synthetic.with_extra_features(base, 3, 2, 5)
    vals = []
    for g, w, w2 in zip(base, wide, again):
        fa, fb = np.float32(w.f_atoms), np.float32(w.f_bonds)
        assert fa.shape == (g.n_atoms, 136) and fb.shape == (g.n_bonds, 152)
        assert np.array_equal(fa[:, :133], np.float32(g.f_atoms))
        assert np.array_equal(fb[:, :136], fa[np.array(g.b2a)]) and np.array_equal(fb[:, 136:150], np.float32(g.f_bonds)[:, 133:])
        assert np.array_equal(fb[0::2, 150:], fb[1::2, 150:])  # one row per pair
        assert np.array_equal(fa.view(np.uint32), np.float32(w2.f_atoms).view(np.uint32))
        assert len(base[0].f_atoms[0]) == 133  # (copies: the inputs are untouched)
        vals += [fa[:, 133:].ravel(), fb[0::2, 150:].ravel()]
    v = np.concatenate(vals)
    tiny = np.finfo(np.float32).tiny
    assert (v < 0).any() and (v == 0).any() and (np.abs(v) == 1e3).any() and ((np.abs(v) > 0) & (np.abs(v) < tiny)).any()


@pytest.mark.parametrize('da,db', DIMS)
def test_encode_stage_decode_roundtrip_is_bitwise(da, db):
    mols = _mols(da, db)
    g = BatchMolGraph(mols)
    ref = BatchMolGraph(mols, compact=False)
    assert g._compact is not None, g._compact_why
    ax, bx, da_, db_ = g._compact_extra
    assert (da_, db_) == (da, db) and g._compact_dims == (133 + da, 147 + da + db)
    assert len(ax) == g.n_atoms * da * 4 and len(bx) == (g.n_bonds - 1) // 2 * db * 4
    assert len(g._compact[2]) == 16 * g.n_atoms and len(g._compact[3]) == 16 * ((g.n_bonds - 1) // 2)
    # the staged image: the six sections of a batch without extras, then the two dense ones, 16-byte aligned
    host = np.zeros(_stage_bound(g._compact + (ax, bx)), np.uint8)
    info = _packer().compact_stage(*g._compact, *g._compact_dims, 64, host.ctypes.data, host.nbytes, *g._compact_extra)
    copied, counts, off, total, (oa, ob) = info
    plain = _packer().compact_stage(*g._compact, 133, 147, 64, 0, 0)  # (the codes alone: the same plan and sections)
    assert copied and plain[1] == counts and plain[2] == off and total <= host.nbytes
    assert off[5] + 8 * counts[3] <= oa and oa + len(ax) <= ob and ob + len(bx) <= total
    assert oa % 16 == 0 and ob % 16 == 0
    assert bytes(host[oa:oa + len(ax)]) == bytes(ax) and bytes(host[ob:ob + len(bx)]) == bytes(bx)
    assert not host[oa:oa + 4 * da].any()  # the pad atom's row
    # decode from the image's own bytes
    n_at, n_pairs = counts[1], (counts[2] - 1) // 2
    sect = [bytes(host[off[0]:off[0] + 16 * counts[0]]), bytes(host[off[1]:off[1] + 4 * counts[0]]),
            bytes(host[off[2]:off[2] + 16 * n_at]), bytes(host[off[3]:off[3] + 16 * n_pairs])]
    h = BatchMolGraph.from_compact(*sect, *g._compact_dims, bytes(host[oa:oa + len(ax)]), bytes(host[ob:ob + len(bx)]),
                                   da, db)
    for attr in ('f_atoms', 'f_bonds', 'w_atoms', 'w_bonds', 'b2a', 'b2revb', 'a2b'):
        a, b = getattr(ref, attr).numpy(), getattr(h, attr).numpy()
        assert a.dtype == b.dtype and a.shape == b.shape, attr
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), attr
    assert ref.f_atoms.shape[1] == 133 + da and ref.f_bonds.shape[1] == 147 + da + db
    # the batch's own lazy view (tail mode) as well
    t = BatchMolGraph(mols, device_bond_features=True)
    assert t._compact_extra is not None
    assert np.array_equal(t.f_bonds.numpy().view(np.uint8), ref.f_bonds.numpy().view(np.uint8))


def test_no_extras_is_unchanged():
    mols = synthetic.make_batch('polymer', 3, 5)
    g = BatchMolGraph(mols)
    assert g._compact_extra is None and len(g._compact) == 4
    info = _packer().compact_stage(*g._compact, 133, 147, 64, 0, 0)
    assert len(info) == 4


def test_refusal_reasons():
    mols = _mols(3, 2)
    mols[0].f_bonds[4][-1] = mols[0].f_bonds[4][-1] + 1.0  # b1 of a pair only
    g = BatchMolGraph(mols)
    assert g._compact is None and 'two directions' in g._compact_why
    mols = _mols(3, 2)
    mols[0].overwrite_default_atom_features = True
    g = BatchMolGraph(mols)
    assert g._compact is None and 'overwrite_default' in g._compact_why
    mols = _mols(3, 2)
    mols[0].overwrite_default_bond_features = True
    g = BatchMolGraph(mols)
    assert g._compact is None and 'overwrite_default' in g._compact_why
    for da, db in ((65, 0), (0, 65)):
        g = BatchMolGraph(_mols(da, db))
        assert g._compact is None and 'at most 64' in g._compact_why
    # such batches keep the host-built path
    assert g.f_bonds.shape[1] == 147 + 65
    # an atom extra that differs between a bond row and its source atom's row
    mols = _mols(3, 2)
    mols[0].f_bonds[2][134] += 0.5
    g = BatchMolGraph(mols)
    assert g._compact is None and 'source atom' in g._compact_why


def test_nan_extras_encode_bitwise():
    mols = _mols(2, 2)
    mols[0].f_atoms[1][134] = float('nan')
    for b in range(mols[0].n_bonds):
        if mols[0].b2a[b] == 1:
            mols[0].f_bonds[b][134] = float('nan')
    mols[0].f_bonds[0][-1] = mols[0].f_bonds[1][-1] = float('nan')
    g = BatchMolGraph(mols)
    assert g._compact is not None, g._compact_why


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_number_unchanged_and_the_header_says_so():
    assert _native.ABI_VERSION == 12 and _native.lib().wdmpnn_abi_version() == 12
    text = open(HEADER).read()
    assert '#define WDMPNN_ABI_VERSION 12' in text
    assert 'appended at the tail of WdGraph and WdCompact' in text


def test_grown_structs_match_the_header(tmp_path):
    structs = (('WdGraph', _native.WdGraph), ('WdCompact', _native.WdCompact))
    src = tmp_path / 'layout.c'
    body = ''
    want = []
    for name, S in structs:
        body += f'  printf(" %zu", sizeof({name}));\n'
        want.append(ctypes.sizeof(S))
        for f, _ in S._fields_:
            body += f'  printf(" %zu", offsetof({name}, {f}));\n'
            want.append(getattr(S, f).offset)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wdmpnn.h"\nint main(void) {\n' + body +
                   '  printf("\\n"); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC', 'gcc'), '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    # appended at the end, after everything ABI 12 had
    G, C = _native.WdGraph, _native.WdCompact
    assert [f for f, _ in G._fields_][-4:] == ['atom_extra', 'bond_extra', 'atom_extra_dim', 'bond_extra_dim']
    assert [f for f, _ in C._fields_][-4:] == ['atom_extra_dim', 'bond_extra_dim', 'atom_extra', 'bond_extra']
    assert G.atom_extra.offset > G.blk_max_atoms.offset and C.atom_extra_dim.offset > C.block_nnz.offset


def _compact_struct(da, db, bits=14):
    c = _native.WdCompact()
    c.n_mols, c.n_atoms, c.n_bonds, c.n_blocks = 2, 11, 21, 1
    c.atom_fdim, c.bond_fdim, c.nnz_msg, c.nnz_agg = 133 + da, 133 + da + bits + db, 40, 20
    c.atom_extra_dim, c.bond_extra_dim = da, db
    return c


def test_library_reads_the_grown_compact_struct():
    """wdmpnn_graph_bytes (host only) sees the extra dims: the widened rows enlarge the graph, the caps hold."""
    L = _native.lib()
    n0, n1 = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.wdmpnn_graph_bytes(ctypes.byref(_compact_struct(0, 0)), ctypes.byref(n0)) == 0
    assert L.wdmpnn_graph_bytes(ctypes.byref(_compact_struct(40, 10)), ctypes.byref(n1)) == 0
    # 147 -> 197 columns: ld_bonds 160 -> 224, ld_atoms 160 -> 192 (rounded to 32), fp32 rows + 6-byte planes
    assert n1.value - n0.value == (128 * 64 + 128 * 32) * 10 + 64 * 32 * 6
    assert L.wdmpnn_graph_bytes(ctypes.byref(_compact_struct(64, 64)), ctypes.byref(n1)) == 0
    for da, db, bits in ((65, 0, 14), (0, 65, 14), (-1, 0, 14), (3, 2, 17)):
        assert L.wdmpnn_graph_bytes(ctypes.byref(_compact_struct(da, db, bits)), ctypes.byref(n1)) == -1001, (da, db, bits)
    assert L.wdmpnn_graph_bytes(ctypes.byref(_compact_struct(3, 2, 16)), ctypes.byref(n1)) == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_graph_table_and_slot_batch_refuse_extras():
    mols = _mols(3, 2)
    with pytest.raises(ValueError, match='--resident_graphs'):
        GraphTable([g for g in mols if g.n_atoms], 'cpu')
    with pytest.raises(ValueError, match='--number_of_molecules'):
        SlotBatch([mols, mols])
    assert len(SlotBatch([mols])) == 1  # one molecule per row: an ordinary batch


# ------------------------------------------------------------------------------------------------ command line
BASE = ['--data_path', 'd.csv', '--graphs_path', 'g.npz', '--save_dir', 'out']
PRED = ['--test_path', 't.csv', '--graphs_path', 'g.npz', '--preds_path', 'p.csv', '--checkpoint_path', 'm.pt']


def test_cli_arguments():
    from chemprop_amd import cli
    a = cli.parse_args(BASE)
    assert a.bond_features_path is None and a.no_bond_features_scaling is False
    a = cli.parse_args(BASE + ['--atom_features_path', 'a.npz', '--no_atom_descriptor_scaling', '--bond_features_path',
                               'b.npz', '--no_bond_features_scaling'])
    # (the run the reference spells --atom_descriptors feature --atom_descriptors_path a.npz)
    assert (a.atom_descriptors, a.atom_descriptors_path, a.no_atom_descriptor_scaling) == ('feature', 'a.npz', True)
    assert (a.bond_features_path, a.no_bond_features_scaling) == ('b.npz', True)
    with pytest.raises(ValueError, match='--atom_features_path F.npz'):  # the reference's spelling names the flag
        cli.parse_args(BASE + ['--atom_descriptors', 'feature', '--atom_descriptors_path', 'a.npz'])
    with pytest.raises(ValueError, match='cannot be combined'):
        cli.parse_args(BASE + ['--atom_features_path', 'a.npz', '--atom_descriptors', 'descriptor',
                               '--atom_descriptors_path', 'd.npz'])
    with pytest.raises(ValueError, match='pandas'):
        cli.parse_args(BASE + ['--atom_features_path', 'a.pkl'])
    cli.check_atom_descriptor_args('feature', 'a.npz')  # (the mode itself is supported: run_training, checkpoints)
    with pytest.raises(ValueError, match='needs --atom_descriptors_path'):
        cli.check_atom_descriptor_args('feature', None)
    with pytest.raises(ValueError, match='without --bond_features_path'):
        cli.parse_args(BASE + ['--no_bond_features_scaling'])
    with pytest.raises(ValueError, match='pandas'):
        cli.parse_args(BASE + ['--bond_features_path', 'b.pkl'])
    with pytest.raises(ValueError, match='RDKit'):
        cli.parse_args(BASE + ['--bond_features_path', 'b.sdf'])
    many = ['--number_of_molecules', '2', '--extra_graphs_path', 'g2.npz']
    with pytest.raises(ValueError, match='number_of_molecules'):
        cli.parse_args(BASE + many + ['--bond_features_path', 'b.npz'])
    with pytest.raises(ValueError, match='number_of_molecules'):
        cli.parse_args(BASE + many + ['--atom_features_path', 'a.npz'])
    assert cli.parse_predict_args(PRED).bond_features_path is None
    assert cli.parse_predict_args(PRED + ['--bond_features_path', 'b.npz']).bond_features_path == 'b.npz'
    assert cli.parse_fingerprint_args(PRED + ['--bond_features_path', 'b.npz']).bond_features_path == 'b.npz'
    with pytest.raises(ValueError, match='pandas'):
        cli.parse_predict_args(PRED + ['--bond_features_path', 'b.pkl'])


def test_feature_files_are_checked(tmp_path):
    from chemprop_amd import cli
    graphs = synthetic.make_batch('polymer', 3, 2)
    good_a = [np.full((g.n_atoms, 2), 1.0 + k) for k, g in enumerate(graphs)]
    good_b = [np.full((g.n_bonds // 2, 3), 2.0 + k) for k, g in enumerate(graphs)]
    good_b[1][0, 0] = np.nan
    pa, pb = str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')
    np.savez(pa, *good_a)
    np.savez(pb, *good_b)
    got = cli.load_bond_features(pb, graphs)
    assert [x.shape for x in got] == [x.shape for x in good_b] and got[1][0, 0] == 0.0 and got[1].dtype == np.float64
    assert all(np.array_equal(x, y) for x, y in zip(cli.load_atom_descriptors(pa, graphs), good_a))

    def bad(arrays, match, loader=cli.load_bond_features):
        p = str(tmp_path / 'bad.npz')
        np.savez(p, *arrays)
        with pytest.raises(ValueError, match=match):
            loader(p, graphs)
    bad(good_b[:2], 'holds 2 bond feature arrays for 3 molecules')
    bad([good_b[0], good_b[1][:-1], good_b[2][:-1]], 'array 1 has .*the number of bonds is different from the length of '
                                                     'the extra bond features')
    bad([good_b[0], good_b[1], good_b[2][:, :2]], 'array 2 has 2 features per bond, array 0 has 3')
    bad([good_b[0], good_b[1].ravel(), good_b[2]], 'array 1 has shape')
    bad(good_a, 'array 0 has .*the number of bonds is different')  # (an atom file given as the bond file)
    bad([good_a[0], good_a[1][:-1], good_a[2]], 'array 1 has .*the number of atoms is different from the length of the '
                                                'extra atom features', cli.load_atom_descriptors)


def test_scalers_fit_the_training_rows_and_are_saved_under_the_reference_keys(tmp_path):
    import torch
    from chemprop_amd import TrainArgs, cli
    from chemprop_amd import featurization as F
    from chemprop_amd.model import MoleculeModel
    rng = np.random.default_rng(4)
    graphs = synthetic.make_batch('polymer', 5, 2)
    xa = [rng.standard_normal((g.n_atoms, 2)) * 3 + 1 for g in graphs]
    xb = [rng.standard_normal((g.n_bonds // 2, 3)) - 2 for g in graphs]
    train_idx = [3, 0, 4]
    sa, sca = cli.scale_atom_descriptors(xa, train_idx)
    sb, scb = cli.scale_atom_descriptors(xb, train_idx)
    for sc, arrays, scaled in ((sca, xa, sa), (scb, xb, sb)):
        rows = np.vstack([arrays[i] for i in train_idx])
        assert np.allclose(sc.means, rows.mean(0), rtol=1e-13) and np.allclose(sc.stds, rows.std(0), rtol=1e-13)
        assert not np.allclose(sc.means, np.vstack(arrays).mean(0), rtol=1e-3)  # (not every split's rows)
        assert all(np.allclose(s, (a - sc.means) / sc.stds) for s, a in zip(scaled, arrays))
    args = TrainArgs(hidden_size=16, atom_descriptors='feature', atom_descriptors_path='a.npz', atom_features_size=2,
                     bond_features_size=3, bond_features_path='b.npz', device=torch.device('cpu'))
    try:
        cli.set_feature_sizes(args)
        assert (F.get_atom_fdim(), F.get_bond_fdim()) == (135, 152)
        model = MoleculeModel(args)
        assert (model.encoder.atom_fdim, model.encoder.bond_fdim) == (135, 152) and model.encoder.atom_descriptors is None
        path = str(tmp_path / 'm.pt')
        cli.save_checkpoint(path, model, None, None, args, sca, scb)
        F.set_extra_atom_fdim(0)
        F.set_extra_bond_fdim(0)
        state = torch.load(path, weights_only=True)
        assert state['atom_descriptor_scaler'] == {'means': list(sca.means), 'stds': list(sca.stds)}
        assert state['bond_feature_scaler'] == {'means': list(scb.means), 'stds': list(scb.stds)}
        for k, v in (('atom_descriptors', 'feature'), ('atom_features_size', 2), ('bond_features_size', 3),
                     ('atom_descriptors_path', 'a.npz'), ('bond_features_path', 'b.npz'), ('atom_descriptors_size', 0)):
            assert state['args'][k] == v, k
        back = cli.load_scalers(path)
        assert np.array_equal(back[2].means, sca.means) and np.array_equal(back[3].stds, scb.stds)
        assert back[3].replace_nan_token == 0
        again = cli.load_checkpoint(path, 'cpu')  # (sets the widths the model was built with)
        assert again.encoder.encoder[0].W_i.weight.shape == (16, 152)
        assert (again.encoder.atom_features_size, again.encoder.bond_features_size) == (2, 3)
        # a model's graphs at prediction time: its own scalers, refusals by width and presence
        from chemprop_amd.ensemble import model_graphs
        wide = model_graphs(path, again, graphs, xa, xb)
        want = cli.join_extra_features(graphs, sa, sb)
        assert all(np.array_equal(np.float32(a.f_bonds), np.float32(b.f_bonds)) for a, b in zip(wide, want))
        with pytest.raises(ValueError, match='--bond_features_path'):
            model_graphs(path, again, graphs, xa, None)
        with pytest.raises(ValueError, match='--atom_descriptors_path'):
            model_graphs(path, again, graphs, None, xb)
        with pytest.raises(ValueError, match='trained with 2 extra atom features'):
            model_graphs(path, again, graphs, [a[:, :1] for a in xa], xb)
        plain = MoleculeModel(TrainArgs(hidden_size=16, device=torch.device('cpu')))
        assert model_graphs(None, plain, graphs) is graphs
        with pytest.raises(ValueError, match='trained without extra bond features'):
            model_graphs(None, plain, graphs, None, xb)
    finally:
        F.set_extra_atom_fdim(0)
        F.set_extra_bond_fdim(0)
