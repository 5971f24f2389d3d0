"""Resident graph tables on the GPU (chemprop_amd.graph_table, ``wdmpnn_gather_compact``): the image gathered on
the device is byte for byte the image ``compact_stage`` stages for ``BatchMolGraph`` of the same molecules, the
graph built from it equals the list path's array by array, and training steps, side inputs, two-molecule rows and
``chemprop_train --resident_graphs`` give bitwise the list path's results.  Every check is bitwise."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import graph_table_cases as cases
from chemprop_amd import AtomDescriptorTable, FeatureTable, GraphTable, TrainArgs, _native, cli, synthetic
from chemprop_amd import train as T
from chemprop_amd.featurization import BatchMolGraph, _packer, get_bond_fdim
from chemprop_amd.graph_io import load_graphs, save_graphs
from chemprop_amd.model import MoleculeModel
from chemprop_amd.slots import SlotBatch
from test_compact import _arrays

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
HERE = os.path.dirname(os.path.abspath(__file__))
CSV = os.path.join(HERE, 'data', 'polymer10.csv')
NPZ = os.path.join(HERE, 'data', 'polymer10_graphs.npz')


@pytest.fixture(scope='module')
def pool():
    return cases.gpu_pool()


@pytest.fixture(scope='module')
def table(pool):
    return GraphTable(pool, DEV)


def _polymers(pool):
    return [i for i, g in enumerate(pool) if g.n_bonds > 60 and i > 3]


IMAGE_CASES = {
    'one': lambda pool: [5],
    'one_atom_alone': lambda pool: [cases.ONE_ATOM],
    'twice': lambda pool: [6, 9, 6],
    'reversed': lambda pool: list(range(len(pool)))[::-1][:9],
    'three_blocks': lambda pool: _polymers(pool)[:6] + [cases.ONE_ATOM, cases.WEIGHTS] + _polymers(pool)[:3],
    'limits': lambda pool: [cases.ATOMS_64, cases.BONDS_128],
}


@pytest.mark.parametrize('block_target', [64, 1])
@pytest.mark.parametrize('name', list(IMAGE_CASES))
def test_gathered_image_and_graph_equal_the_list_paths(pool, name, block_target):
    ids = IMAGE_CASES[name](pool)
    t = GraphTable(pool, DEV, block_target=block_target)
    want_g = BatchMolGraph([pool[i] for i in ids], block_target=block_target)
    host = np.zeros(1 << 18, np.uint8)
    copied, counts, off, total = _packer().compact_stage(*want_g._compact, *want_g._compact_dims, block_target,
                                                         host.ctypes.data, host.nbytes)
    assert copied
    B, V1, E1, nblk = counts[:4]
    if name == 'three_blocks':
        assert nblk >= 3
    torch.full((1 << 16,), -1, dtype=torch.int32, device=DEV)  # (dirty the allocator's free blocks)
    got_g = t.rows(ids).batch()
    dg = got_g.device_graph(DEV, False, get_bond_fdim())
    assert dg.gathered and dg.built_on_device and '_compact' not in got_g.__dict__  # (nothing assembled on the host)
    assert dg.h2d_bytes < 64 * B + 3 * 256  # the plan alone crosses the bus
    img = dg.views['compact'].cpu().numpy()
    assert img.nbytes == total
    sizes = dict(mols=16 * B, xn=4 * B, atoms=16 * V1, pairs=8 * (E1 - 1), blocks=32 * nblk, block_nnz=8 * nblk)
    for (section, n), o in zip(sizes.items(), off):
        assert bytes(img[o:o + n]) == bytes(host[o:o + n]), section
    want = want_g.device_graph(DEV, False, get_bond_fdim())
    assert want.built_on_device and not getattr(want, 'gathered', False)
    for f in ('n_atoms', 'n_bonds', 'n_mols', 'atom_fdim', 'bond_fdim', 'ld_atoms', 'ld_bonds', 'n_blocks',
              'blk_max_bonds', 'blk_max_atoms'):
        assert getattr(dg.struct, f) == getattr(want.struct, f), f
    a, b = _arrays(dg), _arrays(want)
    bad = [k for k in a if not np.array_equal(a[k], b[k])]
    assert not bad, bad
    assert got_g.device_graph(DEV, False, get_bond_fdim()) is dg  # cached like any device graph


def test_gather_on_a_side_stream(pool, table):
    """Gather and build run on the stream current at the call; the table was uploaded on another."""
    ids = [7, cases.WEIGHTS, 5]
    want = BatchMolGraph([pool[i] for i in ids]).device_graph(DEV, False, get_bond_fdim())
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        dg = table.rows(ids).batch().device_graph(DEV, False, get_bond_fdim())
    assert dg.home_stream == side.cuda_stream and side.cuda_stream in table._streams
    side.synchronize()
    a, b = _arrays(dg), _arrays(want)
    assert not [k for k in a if not np.array_equal(a[k], b[k])]


# ------------------------------------------------------------------------------------------------ steps
def _model(seed=3, **kw):
    args = TrainArgs(hidden_size=64, depth=3, dataset_type='regression', num_tasks=1, device=DEV, **kw)
    m = MoleculeModel(args)
    synthetic.fill_parameters(m, seed)
    return m.to(DEV).train()


def _run_steps(make_batch, n_steps, model_kw, side=None, torch_seed=11):
    """``n_steps`` training steps (HipAdam) on the batches ``make_batch(k)`` -> (graphs, targets, step kwargs):
    per step the loss, every gradient and every parameter."""
    m = _model(**model_kw)
    opt = T.build_optimizer(m, 1e-3)
    assert isinstance(opt, T.HipAdam)
    torch.manual_seed(torch_seed)  # (the encoder's dropout seeds are drawn from torch's generator)
    out = []
    for k in range(n_steps):
        g, targets, kw = make_batch(k)
        loss = T.train_step(m, g, targets, T.get_loss_func('regression'), opt, **kw)
        out.append((loss.detach().clone(),
                    {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None},
                    {n: p.detach().clone() for n, p in m.named_parameters()}))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for k, ((la, ga, pa), (lb, gb, pb)) in enumerate(zip(a, b)):
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), (k, la, lb)
        assert set(ga) == set(gb) and ga
        for n in ga:
            assert torch.equal(ga[n].view(torch.int32), gb[n].view(torch.int32)), (k, 'grad', n)
        for n in pa:
            assert torch.equal(pa[n].view(torch.int32), pb[n].view(torch.int32)), (k, 'param', n)


def _order(n, seed=1):
    return [int(i) for i in np.random.default_rng(seed).permutation(n)]


def _targets(pos):
    return [[0.1 * (p % 7) - 0.3] for p in pos]


@pytest.mark.parametrize('dropout', [0.0, 0.2])
def test_three_training_steps_equal_the_list_paths(pool, table, dropout):
    """B = 7, hidden 64, depth 3, regression, HipAdam: three steps over different slices of a shuffled order."""
    order = _order(len(pool))
    assert len(order) >= 21
    index = table.index(order)

    def resident(k):
        return [index[7 * k:7 * k + 7].batch()], _targets(order[7 * k:7 * k + 7]), {}

    def listed(k):
        return [BatchMolGraph([pool[i] for i in order[7 * k:7 * k + 7]])], _targets(order[7 * k:7 * k + 7]), {}
    _same(_run_steps(resident, 3, dict(dropout=dropout)), _run_steps(listed, 3, dict(dropout=dropout)))


@pytest.mark.parametrize('shared', [False, True])
def test_two_molecule_rows_equal_slot_batches(shared):
    a, b = synthetic.make_batch('polymer', 12, 41), synthetic.make_batch('qm9', 12, 42)
    t = GraphTable(list(zip(a, b)), DEV)
    order = _order(12, 2)
    index = t.index(order)
    kw = dict(number_of_molecules=2, mpn_shared=shared)

    def resident(k):
        sb = index[4 * k:4 * k + 4].slot_batch(shared=shared)
        assert isinstance(sb, SlotBatch) and (sb.merged is not None) == shared
        return sb, _targets(order[4 * k:4 * k + 4]), {}

    def listed(k):
        pos = order[4 * k:4 * k + 4]
        return SlotBatch([[a[p] for p in pos], [b[p] for p in pos]], shared=shared), _targets(pos), {}
    got = _run_steps(resident, 3, kw)
    _same(got, _run_steps(listed, 3, kw))
    g = index[0:4].slot_batch(shared=shared)
    dgs = [x.device_graph(DEV, False, get_bond_fdim()) for x in list(g) + ([g.merged] if shared else [])]
    assert all(d.gathered for d in dgs)


@pytest.mark.parametrize('side', ['features', 'descriptors'])
def test_side_inputs_from_the_same_index_positions(pool, table, side):
    order = _order(len(pool), 3)[:14]
    index = table.index(order)
    if side == 'features':
        ft = FeatureTable(np.random.default_rng(4).normal(size=(len(pool), 5)), DEV)
        sidx = ft.index(order)
        model_kw = dict(use_input_features=True, features_size=5)
        key = 'features_batch'
    else:
        dt = AtomDescriptorTable(synthetic.random_descriptors(pool, 4, 5), DEV)
        sidx = dt.index(order)
        model_kw = dict(atom_descriptors='descriptor', atom_descriptors_size=4)
        key = 'atom_descriptors_batch'
        sidx[0:7].bind(index[0:7].batch())  # bind accepts the batch (sizes from the host plan)

    def resident(k):
        return [index[7 * k:7 * k + 7].batch()], _targets(order[7 * k:7 * k + 7]), {key: sidx[7 * k:7 * k + 7]}

    def listed(k):
        pos = order[7 * k:7 * k + 7]
        return [BatchMolGraph([pool[i] for i in pos])], _targets(pos), {key: sidx[7 * k:7 * k + 7]}
    _same(_run_steps(resident, 2, model_kw), _run_steps(listed, 2, model_kw))


# ------------------------------------------------------------------------------------------------ CLI
def _outputs(d, ensemble):
    out = {f: open(os.path.join(d, f), 'rb').read() for f in ('test_preds.csv', 'test_scores.json')}
    dirs = [os.path.join(d, f'model_{k}') for k in range(ensemble)] if ensemble > 1 else [d]
    for k, md in enumerate(dirs):
        out[f'log{k}'] = open(os.path.join(md, 'train_val_loss_log.csv'), 'rb').read()
        for ck in ('model.pt', 'best_model.pt'):
            sd = torch.load(os.path.join(md, ck), weights_only=True)['state_dict']
            out[f'{ck}{k}'] = {n: v.cpu() for n, v in sd.items()}
    return out


@pytest.mark.parametrize('case', ['single', 'ensemble', 'refused'])
def test_chemprop_train_resident_graphs_changes_nothing(tmp_path, capsys, case):
    npz = NPZ
    if case == 'refused':  # one training graph leaves the categorical layout: the table refuses the split
        graphs = load_graphs(NPZ)
        k = cli.random_split(10, (0.8, 0.1, 0.1), 0)[0][2]
        graphs[k].f_atoms[0][5] = 0.5
        npz = str(tmp_path / 'g.npz')
        save_graphs(npz, graphs)
    ensemble = 2 if case == 'ensemble' else 1
    argv = ['--data_path', CSV, '--graphs_path', npz, '--polymer', '--epochs', '2', '--batch_size', '3',
            '--hidden_size', '64', '--ensemble_size', str(ensemble), '--save_dir']
    cli.chemprop_train(argv + [str(tmp_path / 'a')])
    capsys.readouterr()
    cli.chemprop_train(argv + [str(tmp_path / 'b'), '--resident_graphs'])
    said = [ln for ln in capsys.readouterr().out.splitlines() if '--resident_graphs' in ln]
    if case == 'refused':
        assert len(said) == 1 and 'list path' in said[0] and 'does not encode compactly' in said[0]
    else:
        assert not said
    a, b = _outputs(str(tmp_path / 'a'), ensemble), _outputs(str(tmp_path / 'b'), ensemble)
    assert set(a) == set(b)
    for f in a:
        if isinstance(a[f], dict):
            assert set(a[f]) == set(b[f])
            for n in a[f]:
                assert torch.equal(a[f][n], b[f][n]), (f, n)
        else:
            assert a[f] == b[f], f
    assert json.load(open(tmp_path / 'b' / 'test_scores.json'))


def test_cli_gathers_its_training_batches(tmp_path, monkeypatch):
    """With the flag the training steps' graphs come from ``wdmpnn_gather_compact``, one table per run."""
    from chemprop_amd import graph_table
    built, gathered = [], []
    real_init, real_dg = graph_table.GraphTable.__init__, graph_table._TableSource.device_graph
    monkeypatch.setattr(graph_table.GraphTable, '__init__',
                        lambda self, *a, **k: (built.append(1), real_init(self, *a, **k))[1])
    monkeypatch.setattr(graph_table._TableSource, 'device_graph',
                        lambda self, g, dev: (gathered.append(len(self.mol_ids)), real_dg(self, g, dev))[1])
    cli.chemprop_train(['--data_path', CSV, '--graphs_path', NPZ, '--polymer', '--epochs', '2', '--batch_size', '3',
                        '--hidden_size', '64', '--ensemble_size', '2', '--resident_graphs', '--save_dir',
                        str(tmp_path / 'o')])
    assert built == [1] and gathered == [3, 3, 2] * 4  # 8 training rows, 2 epochs, 2 members


# ------------------------------------------------------------------------------------------------ library
def test_library_refusals_on_the_gpu(table):
    L = _native.lib()
    idx = table.index([0, 1])
    g = _native.WdGatherCompact()
    assert L.wdmpnn_gather_compact(None, None) == -1000
    assert L.wdmpnn_gather_compact(ctypes.byref(g), None) == 0  # n_mols == 0: a no-op whatever the pointers
    g.n_mols, g.n_rows, g.n_slots = 2, 2, 1
    g.t_atoms, g.t_pairs, g.t_xn = table._d_atoms.data_ptr(), table._d_pairs.data_ptr(), table._d_xn.data_ptr()
    g.t_first, g.ids = table._d_first.data_ptr(), idx._idx.data_ptr()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    g.mols, g.xn, g.atoms = buf.data_ptr(), buf.data_ptr() + 256, buf.data_ptr() + 512
    assert L.wdmpnn_gather_compact(ctypes.byref(g), None) == -1000  # pairs is NULL
    g.pairs = buf.data_ptr() + 2048
    neg = _native.WdGatherCompact.from_buffer_copy(g)
    neg.n_mols = -1
    assert L.wdmpnn_gather_compact(ctypes.byref(neg), None) == -1001
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched
