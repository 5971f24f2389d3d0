"""Models of several molecules per input (``number_of_molecules > 1``, with and without ``mpn_shared``) on the GPU:
prediction through ``forward_many`` and ``wdmpnn_slots_join``, the direct training step against the autograd step
(bitwise for distinct encoders) and against the reference's own losses and gradients
(tests/golden/multi_molecule, tools/make_multi_molecule_golden.py), and the command line end to end.

TOL is the project's parity bound (README "Parity"): 1e-5 normwise, ``golden_io.normwise``."""
import copy
import csv
import json
import os

import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import FeatureTable, _native, cli, synthetic
from chemprop_amd import mpn as mpn_mod
from chemprop_amd import train as T
from chemprop_amd.graph_io import save_graphs
from chemprop_amd.model import MoleculeModel
from chemprop_amd.predict import device_predictions
from chemprop_amd.slots import SlotBatch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TOL = 1e-5


def _model(case):
    a = copy.copy(case.args)
    a.device = DEV
    m = MoleculeModel(a)
    synthetic.fill_parameters(m, case.seed)
    return m.to(DEV)


def _extras(name):
    z = np.load(os.path.join(golden_io.GOLDEN_DIR, f'{name}.npz'), allow_pickle=False)
    targets = [[None if np.isnan(v) else float(v) for v in row] for row in z['targets']]
    grads = {k[len('train_grad/'):]: z[k] for k in z.files if k.startswith('train_grad/')}
    return targets, z['target_weights'].tolist(), z['data_weights'].tolist(), float(z['train_loss']), grads


class _Counter:
    """Counts the calls of the native wrappers a prediction takes and of the model's own encoder forward."""

    def __init__(self, monkeypatch):
        self.n = {'forward_many': 0, 'slots_join': 0, 'mpn_forward': 0}
        real_many, real_join, real_fwd = mpn_mod.MPNEncoder.forward_many, _native.slots_join, mpn_mod.MPN.forward

        def many(enc, graphs):
            self.n['forward_many'] += 1
            return real_many(enc, graphs)

        def join(*a, **k):
            self.n['slots_join'] += 1
            return real_join(*a, **k)

        def fwd(mod, *a, **k):
            self.n['mpn_forward'] += 1
            return real_fwd(mod, *a, **k)
        monkeypatch.setattr(mpn_mod.MPNEncoder, 'forward_many', many)
        monkeypatch.setattr(_native, 'slots_join', join)
        monkeypatch.setattr(mpn_mod.MPN, 'forward', fwd)


@pytest.mark.parametrize('as_slots', [False, True])
def test_two_molecule_predictions_run_natively_and_match_the_reference(monkeypatch, as_slots):
    """model_two_mols_features_cls (B = 4, H = 32, 5 features, 3-layer FFN, two encoders): ``device_predictions``
    on a plain list and on a SlotBatch within TOL of the reference's output, through one ``forward_many`` per slot
    encoder and one ``wdmpnn_slots_join``, never the model's own forward."""
    case = golden_io.load('model_two_mols_features_cls')
    m = _model(case).eval()
    table = FeatureTable(np.stack(case.features), DEV)
    batch = SlotBatch(case.mol_lists) if as_slots else list(case.graphs)
    count = _Counter(monkeypatch)
    got = list(device_predictions(m, [batch], table))
    assert len(got) == 1 and got[0][0] == 0
    assert count.n == {'forward_many': 2, 'slots_join': 1, 'mpn_forward': 0}
    err = golden_io.normwise(got[0][1].cpu().numpy(), case.output)
    print(f'two molecules, predictions ({"SlotBatch" if as_slots else "list"}): {err:.2e}')
    assert err <= TOL
    # the FFN input: [enc_0 | enc_1 | features], bitwise the model's own torch.cat
    x = list(device_predictions(m, [batch], table, latent='MPN'))[0][1]
    assert tuple(x.shape) == (4, 2 * 32 + 5)
    with torch.no_grad():
        want = torch.cat([m.encoder.encoder[k](case.graphs[k]) for k in range(2)] + [table.data], dim=1)
    assert torch.equal(x.view(torch.int32), want.view(torch.int32))
    alone = list(device_predictions(m, [batch], None, latent='MPN'))[0][1]
    assert torch.equal(alone, x[:, :64])


def test_direct_step_of_two_encoders_is_the_autograd_step_bitwise():
    """Two copies of model_two_mols_features_cls, two consecutive steps with HipAdam: the direct step
    (``_direct_slots``) against ``direct=False``.  Losses, every gradient after step 1 and every parameter after step
    2 are bitwise equal; the optimizer rewrote both encoders' training packs, so only the first forward of each
    encoder packed."""
    case = golden_io.load('model_two_mols_features_cls')
    loss_func = T.get_loss_func('classification')
    table = FeatureTable(np.stack(case.features), DEV)
    targets = [[1.0, 0.0], [0.0, None], [1.0, 1.0], [0.0, 1.0]]
    res = []
    for direct in (True, False):
        m = _model(case).train()
        opt = T.build_optimizer(m, 1e-3)
        assert isinstance(opt, T.HipAdam)
        encs = list(m.encoder.encoder)
        assert encs[0] is not encs[1]
        packs = [[], []]
        for k, enc in enumerate(encs):
            real = enc._packed_params
            enc._packed_params = (lambda real, log: lambda *a, **kw: (log.append(1), real(*a, **kw))[1])(real, packs[k])
        batch = SlotBatch(case.mol_lists) if direct else list(case.graphs)
        if direct:
            head = T._fusable_head(m, loss_func, 'classification')
            plan = T._direct_slots(m, batch, table.rows(range(4)), head)
            assert plan is not None and plan.n == 2 and not plan.shared and len(plan.encoders) == 2
            assert T._direct_slots(m, list(case.graphs), table.rows(range(4)), head) is not None  # (a plain list too)
        losses, grads, n_packs = [], None, []
        for step in range(2):
            losses.append(T.train_step(m, batch, targets, loss_func, opt, dataset_type='classification',
                                       features_batch=table.rows(range(4)), direct=direct))
            n_packs.append([len(p) for p in packs])
            if direct:  # the pack-cache state: both packs are keyed to the parameters' post-step state
                for enc in encs:
                    assert enc._train_pack is not None and enc._train_pack['key'][1] == mpn_mod._OPT_STEPS[0]
            if step == 0:
                grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        for enc in encs:
            del enc._packed_params
        res.append((torch.stack(losses).cpu(), grads, {n: p.detach().clone() for n, p in m.named_parameters()},
                    n_packs))
    (l_d, g_d, p_d, packs_d), (l_a, g_a, p_a, packs_a) = res
    assert packs_d == [[1, 1], [1, 1]], packs_d   # no pack before step 2's forwards
    assert packs_a == [[1, 1], [2, 2]], packs_a   # (the autograd path packs before every forward)
    assert torch.equal(l_d.view(torch.int32), l_a.view(torch.int32)), (l_d, l_a)
    assert set(g_d) == set(g_a) and len(g_d) == len([n for n, p in p_d.items() if 'cached_zero' not in n])
    for n in g_a:
        assert torch.equal(g_d[n].view(torch.int32), g_a[n].view(torch.int32)), n
    for n in p_a:
        assert torch.equal(p_d[n].view(torch.int32), p_a[n].view(torch.int32)), n


def _step(m, batch, case, extras, direct=True):
    targets, tw, dw, _, _ = extras
    kind = case.args.dataset_type
    feats = None if case.features is None else FeatureTable(np.stack(case.features), DEV).rows(range(len(targets)))
    opt = T.build_optimizer(m, 1e-4)
    loss = T.train_step(m, batch, targets, T.get_loss_func(kind), opt, dataset_type=kind, features_batch=feats,
                        target_weights=tw, data_weights=dw, direct=direct)
    return float(loss), {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()
                         if p.grad is not None}


@pytest.mark.parametrize('name', ['shared_two_regression', 'three_mols_features_cls'])
def test_direct_step_matches_the_reference(name):
    """(a) mpn_shared, 2 molecules (polymer + qm9), B = 5, H = 32, regression: one forward and one backward over the
    merged batch; the shared weights' gradient is the sum over the slots, as in the reference.  (b) three encoders,
    H = 30 (the join's word path), B = 3, classification with a missing target, 4 features.  The direct step's loss
    and every gradient within TOL normwise of the reference's."""
    full = f'multi_molecule/{name}'
    case = golden_io.load(full)
    extras = _extras(full)
    shared = bool(case.args.mpn_shared)
    m = _model(case).train()
    batch = SlotBatch(case.mol_lists, shared=shared)
    head = T._fusable_head(m, T.get_loss_func(case.args.dataset_type), case.args.dataset_type)
    feats = None if case.features is None else FeatureTable(np.stack(case.features), DEV).rows(range(len(extras[0])))
    plan = T._direct_slots(m, batch, feats, head)
    assert plan is not None and plan.shared == shared and len(plan.encoders) == (1 if shared else 3)
    if shared:  # a shared model given a plain list keeps the autograd path
        assert T._direct_slots(m, list(case.graphs), feats, head) is None
    loss, grads = _step(m, batch, case, extras)
    want_loss, want = extras[3], extras[4]
    err = abs(loss - want_loss) / abs(want_loss)
    print(f'{name}: loss {loss:.7g} vs {want_loss:.7g} ({err:.2e})')
    assert err <= TOL
    assert set(grads) == set(want)
    for n in sorted(want):
        e = golden_io.normwise(grads[n], want[n])
        print(f'{name}: grad {n}: {e:.2e}')
        assert e <= TOL, (n, e)


def test_shared_encoder_merged_batch_against_the_reference_and_the_per_slot_path():
    """(a): the prediction through ``.merged`` within TOL of the reference's; the merged direct step's gradients
    within TOL of the per-slot autograd path's (not bitwise: the merged batch cuts its molecule blocks
    differently, so the fp16-pair scale words differ)."""
    full = 'multi_molecule/shared_two_regression'
    case = golden_io.load(full)
    extras = _extras(full)
    m = _model(case).eval()
    batch = SlotBatch(case.mol_lists, shared=True)
    assert batch.merged is not None
    seen = []
    real = mpn_mod.MPNEncoder.forward_many
    try:
        mpn_mod.MPNEncoder.forward_many = lambda enc, graphs: (seen.append(list(graphs)), real(enc, graphs))[1]
        got = list(device_predictions(m, [batch]))[0][1]
        plain = list(device_predictions(m, [list(case.graphs)]))[0][1]
    finally:
        mpn_mod.MPNEncoder.forward_many = real
    assert len(seen) == 2 and seen[0] == [batch.merged] and seen[1] == list(case.graphs)
    for what, out in (('merged', got), ('flattened', plain)):
        err = golden_io.normwise(out.cpu().numpy(), case.output)
        print(f'shared, predictions ({what}): {err:.2e}')
        assert err <= TOL
    loss_m, g_m = _step(_model(case).train(), batch, case, extras)
    loss_s, g_s = _step(_model(case).train(), list(case.graphs), case, extras, direct=False)
    assert abs(loss_m - loss_s) <= TOL * abs(loss_s)
    assert set(g_m) == set(g_s)
    for n in sorted(g_s):
        e = golden_io.normwise(g_m[n], g_s[n])
        print(f'shared: merged vs per-slot grad {n}: {e:.2e}')
        assert e <= TOL, (n, e)


# ---------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------
def _read(path):
    with open(path) as f:
        return list(csv.reader(f))


def _write(path, rows):
    with open(path, 'w', newline='') as f:
        csv.writer(f).writerows(rows)


@pytest.fixture(scope='module')
def cli_data(tmp_path_factory):
    """40 rows of a polymer (slot 0) and a small molecule (slot 1, written as a one-fragment polymer string without
    rules, as ``--polymer`` reads every SMILES column), one target."""
    from chemprop_amd import polymer
    tmp = tmp_path_factory.mktemp('multi_molecule')
    rng = np.random.default_rng(9)
    n = 40
    solvents = ['CCO|1.0|', 'O|1.0|', 'CC(C)=O|1.0|', 'c1ccccc1|1.0|']
    rows, g0 = [], []
    g1 = synthetic.make_batch('qm9', n, 77)
    for k in range(n):
        fa = float(rng.choice([0.25, 0.5, 0.75]))
        s = f'[*:1]c1ccc([*:2])cc1.[*:3]CC[*:4]|{fa}|{1 - fa}|<1-3:0.5:0.5<2-4:0.5:0.5<1-2:0.5:0.5~{10:g}'
        g0.append(polymer.synthetic_polymer_graph(s, seed=k))
        rows.append([s, solvents[k % 4], f'{2 * fa + 0.3 * (k % 4) + 0.1 * rng.normal():.6g}'])
    paths = {k: str(tmp / v) for k, v in (('csv', 'd.csv'), ('npz', 'p.npz'), ('npz2', 's.npz'))}
    _write(paths['csv'], [['polymer', 'solvent', 'y']] + rows)
    save_graphs(paths['npz'], g0)
    save_graphs(paths['npz2'], g1)
    return tmp, paths


@pytest.mark.parametrize('shared', [False, True])
def test_cli_trains_predicts_and_fingerprints_two_molecule_models(cli_data, shared):
    """40 rows, 2 slots, H = 32, 2 epochs, with and without ``--mpn_shared``: the run writes its checkpoints;
    ``predict --checkpoint_dir`` with ``--extra_graphs_path`` reproduces the run's test predictions (within TOL: the
    run scores through the model's own forward, the prediction run through the native loop); ``fingerprint
    --fingerprint_type MPN`` writes 2 x 32 columns; both refuse a missing ``--extra_graphs_path``."""
    tmp, paths = cli_data
    d = tmp / ('shared' if shared else 'own')
    argv = ['--data_path', paths['csv'], '--graphs_path', paths['npz'], '--extra_graphs_path', paths['npz2'],
            '--number_of_molecules', '2', '--polymer', '--epochs', '2', '--warmup_epochs', '1', '--batch_size', '8',
            '--hidden_size', '32', '--save_dir', str(d)] + (['--mpn_shared'] if shared else [])
    scores = cli.chemprop_train(argv)
    assert np.isfinite(scores['rmse'][0])
    assert {'best_model.pt', 'model.pt', 'test_preds.csv', 'split_indices.json'} <= set(os.listdir(d))
    state = torch.load(str(d / 'best_model.pt'), weights_only=True)
    assert state['args']['number_of_molecules'] == 2 and state['args']['mpn_shared'] is shared
    assert state['args']['task_names'] == ['y']
    sd = state['state_dict']  # (a shared encoder is stored under both slots' names, as the reference stores it)
    assert torch.equal(sd['encoder.encoder.0.W_h.weight'], sd['encoder.encoder.1.W_h.weight']) is shared
    split = json.load(open(d / 'split_indices.json'))
    table = _read(paths['csv'])
    written = _read(d / 'test_preds.csv')
    assert written[0] == ['polymer', 'solvent', 'y'] and len(written) == 1 + len(split['test'])
    assert [r[:2] for r in written[1:]] == [table[1 + i][:2] for i in split['test']]
    out = str(tmp / f'preds_{int(shared)}.csv')
    common = ['--test_path', paths['csv'], '--graphs_path', paths['npz'], '--preds_path', out, '--checkpoint_dir',
              str(d), '--batch_size', '8']
    mean = cli.chemprop_predict(common + ['--extra_graphs_path', paths['npz2']])
    rows = _read(out)
    assert rows[0] == ['polymer', 'solvent', 'y'] and len(rows) == 41
    assert [r[:2] for r in rows[1:]] == [r[:2] for r in table[1:]]
    want = np.array([[float(r[2])] for r in written[1:]])
    err = golden_io.normwise(mean[split['test']], want)
    print(f'cli ({"shared" if shared else "own encoders"}): predict vs the run\'s test predictions {err:.2e}')
    assert err <= TOL
    fp_out = str(tmp / f'fp_{int(shared)}.csv')
    fp = cli.chemprop_fingerprint(['--test_path', paths['csv'], '--graphs_path', paths['npz'], '--preds_path', fp_out,
                                   '--checkpoint_dir', str(d), '--batch_size', '8', '--fingerprint_type', 'MPN',
                                   '--extra_graphs_path', paths['npz2']])
    assert fp.shape == (40, 64, 1)
    rows = _read(fp_out)
    assert rows[0] == ['polymer', 'solvent'] + [f'fp_{j}' for j in range(64)] and len(rows) == 41
    assert [r[:2] for r in rows[1:]] == [r[:2] for r in table[1:]]
    with pytest.raises(ValueError, match='extra_graphs_path'):
        cli.chemprop_predict(common)
    with pytest.raises(ValueError, match='extra_graphs_path'):
        cli.chemprop_fingerprint(common + ['--fingerprint_type', 'MPN'])
