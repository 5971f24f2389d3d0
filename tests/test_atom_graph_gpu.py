"""Atom-message graphs built on the device (``wdmpnn_build_graph_atom``): the device-built graph against the
host-packed one array by array, the encoder on both bitwise (and against the fp32 oracle at 1e-5), the direct
training step against the autograd step bitwise, batches of a resident table, and ``chemprop_train
--atom_messages`` end to end with ``chemprop_predict`` and ``chemprop_fingerprint`` on its checkpoint."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import TrainArgs, cli, synthetic
from chemprop_amd.featurization import BatchMolGraph, get_atom_fdim, get_bond_fdim
from chemprop_amd.graph_table import GraphTable
from chemprop_amd.model import MoleculeModel
from chemprop_amd.mpn import MPNEncoder
from chemprop_amd.train import _direct_encoder, _frozen_plan, _fusable_head, build_optimizer, get_loss_func, train_step
from oracle import mpn_ref
from test_atom_graph_host import batches, rows_without_zeros, static_layout
from test_compact import _read

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
HERE = os.path.dirname(os.path.abspath(__file__))
CSV = os.path.join(HERE, 'data', 'polymer10.csv')
NPZ = os.path.join(HERE, 'data', 'polymer10_graphs.npz')
FB = get_bond_fdim(atom_messages=True)


def cases():
    """The four batches of the host tests + one with extra atom / bond features (4, 3): (name, molecules, Fb')."""
    wide = synthetic.with_extra_features(synthetic.make_batch('polymer', 6, 8) +
                                         synthetic.edge_case_batch(3, star_leaves=11), 4, 3, 2)
    return [(n, m, FB) for n, m in batches()] + [('extras', wide, FB + 3)]


# ------------------------------------------------------------------------------------------------ 1. the graph
DENSE = ('f_atoms', 'f_bonds', 'f_atoms_x6', 'f_bonds_x6', 'f_atoms_blk_x6', 'atom_feat_sum_x6', 'w_atoms', 'mol_start',
         'mol_size', 'xn', 'b2revb', 'blocks', 'bond_blk_row', 'msg_ell_idx', 'msg_ell_coef')
SCALARS = ('n_atoms', 'n_bonds', 'n_mols', 'atom_fdim', 'bond_fdim', 'ld_atoms', 'ld_bonds', 'bond_col0', 'n_blocks',
           'atom_messages', 'blk_max_bonds', 'blk_max_atoms', 'desc_dim')
LISTS = (('feat', 'bond_feat_gather'), ('msg', 'msg_gather'), ('agg', 'atom_gather'), ('msg_t', 'msg_gather_t'),
         ('agg_t', 'atom_gather_t'))


def _arrays(dg):
    """Every array of an atom-message DeviceGraph, read back: the dense ones as bytes, the lists as Csr-like
    (ptr, idx, coef) with their 8 dummy entries, the atom ELL rows."""
    from chemprop_amd.featurization import Csr
    s = dg.struct
    V1, E1, B, nblk = s.n_atoms, s.n_bonds, s.n_mols, s.n_blocks
    Vap, Rbp = -(-V1 // 128) * 128, -(-E1 // 128) * 128
    lda, ldb = s.ld_atoms, s.ld_bonds
    where = {'f_atoms': (s.f_atoms, Vap * lda * 4), 'f_bonds': (s.f_bonds, Rbp * ldb * 4),
             'f_atoms_x6': (s.f_atoms_x6, Vap * lda * 6), 'f_bonds_x6': (s.f_bonds_x6, Rbp * ldb * 6),
             'f_atoms_blk_x6': (s.f_atoms_blk_x6, nblk * 64 * lda * 6),
             'atom_feat_sum_x6': (s.atom_feat_sum_x6, Vap * ldb * 6), 'w_atoms': (s.w_atoms, V1 * 4),
             'mol_start': (s.mol_start, B * 4), 'mol_size': (s.mol_size, B * 4), 'xn': (s.degree_of_polym, B * 4),
             'b2revb': (s.b2revb, E1 * 4), 'blocks': (s.blocks, nblk * 32), 'bond_blk_row': (s.bond_blk_row, Rbp * 4),
             'msg_ell_idx': (s.msg_ell_idx, Vap * 8), 'msg_ell_coef': (s.msg_ell_coef, Vap * 32),
             'atom_ell_idx': (s.atom_ell_idx, Vap * 8), 'atom_ell_coef': (s.atom_ell_coef, Vap * 32)}
    for name, (p, n) in where.items():
        assert p, name
    out = {k: _read(dg, p, n) for k, (p, n) in where.items()}
    for name, field in LISTS:
        c = getattr(s, field)
        ptr = _read(dg, c.ptr, (V1 + 1) * 4).view(np.int32)
        n = int(ptr[-1])
        idx = _read(dg, c.idx, (n + 8) * 4).view(np.int32)  # (the 8 dummy entries past the end are readable)
        coef = _read(dg, c.coef, (n + 8) * 4).view(np.float32)
        out[name] = Csr(ptr, idx[:n], coef[:n])
    return out


def _check_graph(d_dev, d_host, g_host):
    """Check 1 of a device-built atom-message graph against the host-built one of the same molecules."""
    assert d_dev.built_on_device and not d_host.built_on_device
    for f in SCALARS:
        assert getattr(d_dev.struct, f) == getattr(d_host.struct, f), f
    s = d_dev.struct
    assert s.atom_messages == 1 and s.bond_col0 == 0
    assert not (s.atom_codes or s.bond_src_blk or s.bond_tail or s.atom_extra or s.bond_extra)  # (not code-capable)
    a, b = _arrays(d_dev), _arrays(d_host)
    bad = [k for k in DENSE if not np.array_equal(a[k], b[k])]
    assert not bad, bad
    spec = static_layout(g_host)
    for name, _ in LISTS:
        # entry for entry the host packer's list once the zero coefficients are dropped ...
        assert rows_without_zeros(a[name]) == rows_without_zeros(b[name]), name
        # ... and exactly the static-offset layout (kept zeros, the pad entry of every msg row, row 0)
        for part in ('ptr', 'idx', 'coef'):
            assert np.array_equal(getattr(a[name], part), getattr(spec[name], part)), (name, part)
    # atom ELL: slot q = entry q of the atom_gather row (zeros included), block-local; bit 7 of slot 7 = more
    V1 = s.n_atoms
    blocks = a['blocks'].view(np.int32).reshape(-1, 8)
    first = np.zeros(V1, np.int64)
    for _, _, as_, an in blocks[:, :4].tolist():
        first[as_:as_ + an] = as_
    ell_idx, ell_coef = a['atom_ell_idx'].reshape(-1, 8), a['atom_ell_coef'].view(np.float32).reshape(-1, 8)
    agg = a['agg']
    for r in range(V1):
        lo, hi = int(agg.ptr[r]), int(agg.ptr[r + 1])
        n = min(8, hi - lo)
        want_idx = np.zeros(8, np.uint8)
        want_idx[:n] = agg.idx[lo:lo + n] - first[r]
        if hi - lo > 8:
            want_idx[7] |= 0x80
        want_coef = np.zeros(8, np.float32)
        want_coef[:n] = agg.coef[lo:lo + n]
        assert np.array_equal(ell_idx[r], want_idx) and np.array_equal(ell_coef[r], want_coef), r
    assert not ell_idx[V1:].any() and not ell_coef[V1:].any()


@pytest.mark.parametrize('case', range(5))
def test_device_built_graph_equals_host_built(case):
    name, mols, fb = cases()[case]
    g_dev, g_host = BatchMolGraph(mols), BatchMolGraph(mols, compact=False)
    assert g_dev._compact is not None, g_dev._compact_why
    d_dev, d_host = g_dev.device_graph(DEV, True, fb), g_host.device_graph(DEV, True, fb)
    _check_graph(d_dev, d_host, g_host)
    # the image is the bond-mode one: the same bytes cross the bus
    assert d_dev.h2d_bytes == g_dev.device_graph(DEV, False).h2d_bytes
    if name != 'extras':  # (test_compact's bound for the same batches; extras add their dense sections)
        assert d_dev.h2d_bytes <= (16 if name.startswith('polymer') else 24) * (g_dev.n_bonds - 1) + 6 * 256
    # one graph for inference and training, whatever atom_blocks says
    assert g_dev.device_graph(DEV, True, fb, False) is d_dev and g_dev.device_graph(DEV, True, fb, True) is d_dev
    assert g_dev.device_graph(DEV, True) is not None


# ------------------------------------------------------------------------------------------------ 2. the encoder
def _encoder_outputs(enc, g):
    with torch.no_grad():
        inf = enc.eval()(g)
    enc.zero_grad()
    out = enc.train()(g)
    out.square().sum().backward()
    return [inf, out.detach()] + [p.grad.clone() for p in enc.parameters() if p.grad is not None]


@pytest.mark.parametrize('bias', [False, True])  # blocked inference / unblocked
@pytest.mark.parametrize('case', [0, 3])  # polymer 8; the weight cases (kept zeros, rows longer than the ELL)
def test_encoder_is_bitwise_the_host_graphs(case, bias):
    name, mols = batches()[case]
    args = TrainArgs(hidden_size=64, depth=3, atom_messages=True, bias=bias)
    enc = MPNEncoder(args, get_atom_fdim(), FB)
    synthetic.fill_parameters(enc, 7)
    p = {n: t.detach().clone() for n, t in enc.named_parameters()}
    g_dev, g_host = BatchMolGraph(mols), BatchMolGraph(mols, compact=False)
    ref = mpn_ref.encoder_forward(p, g_host, args)
    enc = enc.to(DEV)
    a, b = _encoder_outputs(enc, g_dev), _encoder_outputs(enc, g_host)
    assert g_dev.device_graph(DEV, True, FB).built_on_device and not g_host.device_graph(DEV, True, FB).built_on_device
    assert len(a) == len(b) >= 5
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), k
    assert golden_io.normwise(a[0].cpu().numpy(), ref.numpy()) <= 1e-5
    assert golden_io.normwise(a[1].cpu().numpy(), ref.numpy()) <= 1e-5


# ------------------------------------------------------------------------------------------------ 3. the step
MOLS = [synthetic.make_batch('polymer', 8, 40 + k) for k in range(3)]


def _model(freeze_encoder=False):
    args = TrainArgs(hidden_size=64, depth=3, atom_messages=True, dataset_type='regression', num_tasks=2, device=DEV)
    m = MoleculeModel(args)
    synthetic.fill_parameters(m, 3)
    if freeze_encoder:
        for p in m.encoder.parameters():
            p.requires_grad_(False)
    return m.to(DEV).train()


def _targets(k):
    rng = np.random.default_rng(90 + k)
    return rng.normal(size=(8, 2)).tolist()


def _three_steps(direct, freeze_encoder):
    m = _model(freeze_encoder)
    opt = build_optimizer(m, 1e-3)
    assert type(opt).__name__ == 'HipAdam'
    lf = get_loss_func('regression')
    losses = [float(train_step(m, [BatchMolGraph(MOLS[k])], _targets(k), lf, opt, dataset_type='regression',
                               direct=direct)) for k in range(3)]
    return losses, {n: p.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize('freeze_encoder', [False, True])
def test_direct_step_is_bitwise_the_autograd_step(freeze_encoder):
    m = _model(freeze_encoder)
    head = _fusable_head(m, get_loss_func('regression'), 'regression')
    batch = [BatchMolGraph(MOLS[0])]
    assert head is not None and m.encoder.encoder[0].atom_messages
    if freeze_encoder:  # the direct path this model takes
        plan = _frozen_plan(m, batch, None, head)
        assert plan is not None and plan.enc_frozen and _direct_encoder(m, batch, None, head) is None
    else:
        assert _direct_encoder(m, batch, None, head) is m.encoder.encoder[0]
    (la, pa), (lb, pb) = _three_steps(True, freeze_encoder), _three_steps(False, freeze_encoder)
    assert la == lb and all(np.isfinite(la))
    assert list(pa) == list(pb) and all(torch.equal(pa[n], pb[n]) for n in pa)
    start = dict(_model(freeze_encoder).named_parameters())  # (it trained: the steps moved what was not frozen)
    assert torch.equal(pa['encoder.encoder.0.W_h.weight'], start['encoder.encoder.0.W_h.weight']) is freeze_encoder
    assert not torch.equal(pa['ffn.1.weight'], start['ffn.1.weight'])


# ------------------------------------------------------------------------------------------------ 4. resident table
def test_resident_table_batches():
    pool = synthetic.make_batch('polymer', 16, 77)
    table = GraphTable(pool, DEV)
    order = np.random.default_rng(5).permutation(16).tolist()
    index = table.index(order)
    for s in (0, 8):
        ids = order[s:s + 8]
        g = index[s:s + 8].batch()
        dg = g.device_graph(DEV, True, FB)
        assert dg.gathered and dg.built_on_device and '_compact' not in g.__dict__  # (nothing assembled on the host)
        assert dg.h2d_bytes < 64 * 8 + 3 * 256  # the plan alone crosses the bus
        mols = [pool[i] for i in ids]
        fresh = BatchMolGraph(mols)
        assert g.max_num_bonds == fresh.max_num_bonds
        g_host = BatchMolGraph(mols, compact=False)
        _check_graph(dg, g_host.device_graph(DEV, True, FB), g_host)
        # device-built against device-built: every array, the lists with their kept zeros
        a, b = _arrays(dg), _arrays(fresh.device_graph(DEV, True, FB))
        for k in a:
            if k in dict(LISTS):
                assert all(np.array_equal(getattr(a[k], q), getattr(b[k], q)) for q in ('ptr', 'idx', 'coef')), k
            else:
                assert np.array_equal(a[k], b[k]), k
        assert g.device_graph(DEV, True, FB) is dg


# ------------------------------------------------------------------------------------------------ 5. command line
def _outputs(d):
    out = {f: open(os.path.join(d, f), 'rb').read() for f in ('test_preds.csv', 'test_scores.json',
                                                               'train_val_loss_log.csv')}
    for ck in ('model.pt', 'best_model.pt'):
        sd = torch.load(os.path.join(d, ck), weights_only=True)['state_dict']
        out[ck] = {n: v.cpu() for n, v in sd.items()}
    return out


def test_chemprop_train_atom_messages_end_to_end(tmp_path):
    argv = ['--data_path', CSV, '--graphs_path', NPZ, '--polymer', '--epochs', '2', '--batch_size', '3',
            '--hidden_size', '64', '--atom_messages', '--save_dir']
    s1 = cli.chemprop_train(argv + [str(tmp_path / 'a')])
    s2 = cli.chemprop_train(argv + [str(tmp_path / 'b'), '--resident_graphs'])
    assert s1 == s2 and np.isfinite(s1['rmse'][0])
    a, b = _outputs(tmp_path / 'a'), _outputs(tmp_path / 'b')
    for k in a:
        if isinstance(a[k], dict):
            assert list(a[k]) == list(b[k]) and all(torch.equal(a[k][n], b[k][n]) for n in a[k]), k
        else:
            assert a[k] == b[k], k
    ck = str(tmp_path / 'a' / 'best_model.pt')
    raw = torch.load(ck, weights_only=True)
    assert raw['args']['atom_messages'] is True
    assert tuple(raw['state_dict']['encoder.encoder.0.W_h.weight'].shape) == (64, 64 + FB)
    assert tuple(raw['state_dict']['encoder.encoder.0.W_i.weight'].shape) == (64, get_atom_fdim())
    # chemprop_predict on the checkpoint reproduces the run's test predictions
    split = json.load(open(tmp_path / 'a' / 'split_indices.json'))
    written = list(csv.reader(open(tmp_path / 'a' / 'test_preds.csv')))
    table = list(csv.reader(open(CSV)))
    assert [r[0] for r in written[1:]] == [table[1 + i][0] for i in split['test']]
    emb = str(tmp_path / 'emb.npy')
    common = ['--test_path', CSV, '--graphs_path', NPZ, '--checkpoint_path', ck, '--batch_size', '3']
    mean = cli.chemprop_predict(common + ['--preds_path', str(tmp_path / 'p.csv'), '--save_graph_embeddings',
                                          '--graph_embeddings_path', emb])
    want = np.array([[float(c) for c in r[1:]] for r in written[1:]])
    assert mean.shape == (10, 1) and golden_io.normwise(mean[split['test']], want) <= 1e-5
    assert np.load(emb).shape == (10, 64)
    fp = cli.chemprop_fingerprint(common + ['--preds_path', str(tmp_path / 'fp.csv'), '--fingerprint_type', 'MPN'])
    assert fp.shape == (10, 64, 1) and np.isfinite(fp).all()
    assert len(list(csv.reader(open(tmp_path / 'fp.csv')))[0]) == 1 + 64
