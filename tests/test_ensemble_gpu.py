"""Ensembles on the GPU: ``wdmpnn_ensemble_add`` and ``wdmpnn_ensemble_sid`` against the reference's numbers
(tests/golden/ensemble/ensemble_ref.npz, made by tools/make_ensemble_golden.py), ``EnsembleAccumulator``,
``predict_ensemble``, ``chemprop_train --ensemble_size`` and ``chemprop_predict`` end to end.

The bounds: the mean of M values within ``4 * 2^-52 * M * max|v|`` of ``sum / M`` and the variance within
``16 * 2^-52 * M * (|mean| + sd) * sd`` of ``np.var`` per cell (the rounding of Welford's ``d`` and of its product
over M updates; sum of squares in fp64 and Welford in fp32 miss the second bound on block 1 by orders of magnitude);
the pairwise SID within 1e-12 relative of the reference's ``roundrobin_sid`` (fp64 agrees to 4e-16, an fp32 kernel
lands at 1e-7)."""
import csv
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import _native, cli, polymer
from chemprop_amd.ensemble import EnsembleAccumulator, predict_ensemble
from chemprop_amd.graph_io import load_graphs, save_graphs

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EPS = 2.0 ** -52
SENTINEL = -12345.678
ROW_BLOCKS = ((0, 2), (2, 3))


@pytest.fixture(scope='module')
def ref():
    return dict(np.load(os.path.join(golden_io.GOLDEN_DIR, 'ensemble', 'ensemble_ref.npz'), allow_pickle=False))


# ---------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------
def _add_models(block, M, scale=None, with_m2=True):
    """Models 0 .. M of ``block`` (fp32 [models][5][W]) through wdmpnn_ensemble_add in two row blocks, with
    ld_pred = W + 3 and ld_acc = W + 1: (mean, m2, slabs) as float64 numpy arrays, padding included."""
    _, N, W = block.shape
    ld_pred, ld_acc = W + 3, W + 1
    mean = torch.full((N, ld_acc), SENTINEL, dtype=torch.float64, device=DEV)
    m2 = torch.full((N, ld_acc), SENTINEL, dtype=torch.float64, device=DEV)
    slabs = torch.full((M, N, ld_acc), SENTINEL, dtype=torch.float64, device=DEV)
    sm = ss = None
    if scale is not None:
        sm, ss = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in scale)
    for k in range(M):
        for row0, B in ROW_BLOCKS:
            pred = torch.full((B, ld_pred), 777.0, dtype=torch.float32)
            pred[:, :W] = torch.from_numpy(block[k, row0:row0 + B])
            pred = pred.to(DEV)
            e = _native.WdEnsembleAdd()
            e.pred, e.ld_pred, e.B, e.W, e.k, e.row0 = pred.data_ptr(), ld_pred, B, W, k, row0
            e.scale_mean, e.scale_std = _native.ptr(sm) or None, _native.ptr(ss) or None
            e.mean, e.m2, e.keep, e.ld_acc = mean.data_ptr(), m2.data_ptr() if with_m2 else None, \
                slabs[k].data_ptr(), ld_acc
            _native.check(_native.lib().wdmpnn_ensemble_add(ctypes.byref(e), _native.current_stream(DEV)), 'add')
    torch.cuda.synchronize()
    return mean.cpu().numpy(), m2.cpu().numpy(), slabs.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize('W', [3, 7])
def test_model_0_initialises_with_the_scalers_own_rounding(ref, W):
    """k = 0: mean and keep are ``pred.astype(float64) * std + mean_s`` bit for bit (a rounded product, then a
    rounded sum: numpy's, and the reference scaler's), m2 is 0, the padding column stays as it was."""
    block = ref[f'b2_w{W}']
    scale = (ref[f'scale_mean_w{W}'], ref[f'scale_std_w{W}'])
    mean, m2, slabs = _add_models(block, 1, scale)
    want = block[0].astype(np.float64) * scale[1] + scale[0]
    assert np.array_equal(_bits(want), _bits(ref[f'b2_w{W}_inv'][0]))
    assert np.array_equal(_bits(mean[:, :W]), _bits(want)) and np.array_equal(_bits(slabs[0][:, :W]), _bits(want))
    assert np.all(m2[:, :W] == 0)
    for a in (mean, m2, slabs[0]):
        assert np.all(a[:, W] == SENTINEL)
    # without a scaler: the fp32 value as a double
    mean, m2, slabs = _add_models(ref[f'b1_w{W}'], 1)
    assert np.array_equal(_bits(mean[:, :W]), _bits(ref[f'b1_w{W}'][0].astype(np.float64)))
    assert np.array_equal(mean[:, :W], ref[f'b1_w{W}_mean_m1']) and np.all(m2[:, :W] == 0)
    assert np.all(ref[f'b1_w{W}_var_m1'] == 0)


@pytest.mark.parametrize('W', [3, 7])
@pytest.mark.parametrize('M', [1, 2, 5])
@pytest.mark.parametrize('name', ['b1', 'b2'])
def test_mean_and_variance_against_numpy(ref, name, M, W):
    block = ref[f'{name}_w{W}']
    scale = (ref[f'scale_mean_w{W}'], ref[f'scale_std_w{W}']) if name == 'b2' else None
    v = ref[f'b2_w{W}_inv'] if name == 'b2' else block.astype(np.float64)
    mean, m2, slabs = _add_models(block, M, scale)
    var = m2[:, :W] / M
    want_mean, want_var = ref[f'{name}_w{W}_mean_m{M}'], ref[f'{name}_w{W}_var_m{M}']
    nan = np.isnan(want_mean)
    assert np.array_equal(nan, np.isnan(v[:M]).any(axis=0))
    if name == 'b2':  # one NaN cell in model 1: that cell alone is NaN once model 1 is in
        assert int(nan.sum()) == (1 if M >= 2 else 0) and (M < 2 or nan[3, W - 2])
    else:
        assert not nan.any()
    assert np.array_equal(np.isnan(mean[:, :W]), nan) and np.array_equal(np.isnan(var), nan)
    ok = ~nan
    vmax = np.abs(np.where(np.isnan(v[:M]), 0, v[:M])).max(axis=0)
    err = np.abs(mean[:, :W] - want_mean)
    print(f'{name} W={W} M={M}: mean err {np.nanmax(err / vmax):.2e} (bound {4 * EPS * M:.2e})')
    assert np.all(err[ok] <= (4 * EPS * M * vmax)[ok])
    sd = np.sqrt(want_var)
    bound = 16 * EPS * M * (np.abs(want_mean) + sd) * sd
    verr = np.abs(var - want_var)
    print(f'{name} W={W} M={M}: variance err {np.nanmax(verr):.2e} (bound {np.nanmin(bound):.2e} .. {np.nanmax(bound):.2e})')
    assert np.all(verr[ok] <= bound[ok])
    if M == 1:
        assert np.all(var == 0)
    # the kept slabs are the models' own values, the padding column of every buffer is untouched
    assert np.array_equal(_bits(slabs[:, :, :W]), _bits(v[:M]))
    for a in (mean, m2) + tuple(slabs):
        assert np.all(a[:, W] == SENTINEL)


def test_add_without_m2_or_keep_writes_the_mean_alone(ref):
    block = ref['b1_w3']
    mean, m2, _ = _add_models(block, 2, with_m2=False)
    assert np.all(m2 == SENTINEL)
    assert np.all(np.abs(mean[:, :3] - ref['b1_w3_mean_m2']) <= 4 * EPS * 2 * np.abs(block[:2]).max(axis=0))


SID_CASES = [(3, 33, 2, None), (3, 33, 3, None), (3, 33, 3, 1e-3), (2, 300, 5, None), (2, 33, 1, None)]


@pytest.mark.parametrize('N,T,M,threshold', SID_CASES)
def test_pairwise_sid_against_the_reference(ref, N, T, M, threshold):
    key = f'sid_{N}_{T}_{M}'
    spectra = ref[key].astype(np.float64)
    want = ref[f'{key}_thr_out' if threshold else f'{key}_out']
    assert spectra.shape == (M, N, T) and np.isnan(spectra[:, 1, T - 9:]).all() and want.shape == (N,)
    ld, stride = T + 2, N * (T + 2) + 5
    buf = torch.full((M * stride,), float('nan'), dtype=torch.float64)
    for m in range(M):
        buf[m * stride:m * stride + N * ld].view(N, ld)[:, :T] = torch.from_numpy(spectra[m])
    buf = buf.to(DEV)
    out = torch.full((N + 2,), SENTINEL, dtype=torch.float64, device=DEV)
    s = _native.WdEnsembleSid()
    s.preds, s.model_stride, s.ld, s.M, s.N, s.T = buf.data_ptr(), stride, ld, M, N, T
    s.threshold, s.out = threshold or 0.0, out.data_ptr()
    _native.check(_native.lib().wdmpnn_ensemble_sid(ctypes.byref(s), _native.current_stream(DEV)), 'sid')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[N:] == SENTINEL)
    if M == 1:
        assert np.isnan(want).all() and np.isnan(got[:N]).all()
        return
    rel = np.abs(got[:N] - want) / np.abs(want)
    print(f'{key} threshold {threshold}: relative error {rel.max():.2e}')
    assert np.all(want > 0) and np.all(rel <= 1e-12)


def test_accumulator_on_the_device(ref):
    """The class around the kernels: two row blocks, three models, a scaler; ``mean`` / ``variance`` /
    ``individual`` / ``roundrobin_sid`` as device tensors; the order of the models is enforced."""
    block = ref['b2_w7']
    sc = cli.StandardScaler(ref['scale_mean_w7'], ref['scale_std_w7'])
    acc = EnsembleAccumulator(5, 7, DEV, variance=True, keep=True, n_models=3)
    for k in range(3):
        for row0, B in ROW_BLOCKS:
            acc.add(torch.from_numpy(block[k, row0:row0 + B]).to(DEV), row0, k, sc)
        with pytest.raises(ValueError):
            acc.add(torch.from_numpy(block[k, :2]).to(DEV), 0, k, sc)       # the same block again
    with pytest.raises(ValueError):
        acc.add(torch.from_numpy(block[3, :2]).to(DEV), 0, 3, sc)           # a fourth model of three
    v = ref['b2_w7_inv'][:3]
    ind = acc.individual()
    assert ind.device == DEV and ind.dtype == torch.float64 and tuple(ind.shape) == (3, 5, 7)
    assert np.array_equal(_bits(ind.cpu().numpy()), _bits(v))
    mean, var = acc.mean().cpu().numpy(), acc.variance().cpu().numpy()
    ok = ~np.isnan(v).any(axis=0)
    assert np.array_equal(~np.isnan(mean), ok) and np.array_equal(~np.isnan(var), ok)
    assert np.allclose(mean[ok], (v.sum(axis=0) / 3)[ok], rtol=1e-14, atol=0)
    assert np.allclose(var[ok], np.var(v, axis=0)[ok], rtol=1e-12, atol=0)
    # spectra through the accumulator: the kept slabs feed the SID kernel
    spectra = ref['sid_2_300_5']
    acc = EnsembleAccumulator(2, 300, DEV, keep=True, n_models=5)
    for k in range(5):
        acc.add(torch.from_numpy(spectra[k]).to(DEV), 0, k)
    got = acc.roundrobin_sid().cpu().numpy()
    assert np.all(np.abs(got - ref['sid_2_300_5_out']) <= 1e-12 * ref['sid_2_300_5_out'])
    acc = EnsembleAccumulator(2, 300, DEV, keep=True, n_models=1)
    acc.add(torch.from_numpy(spectra[0]).to(DEV), 0, 0)
    assert np.isnan(acc.roundrobin_sid().cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------
# chemprop_train --ensemble_size, predict_ensemble, chemprop_predict
# ---------------------------------------------------------------------------------------------------
def _write(path, rows):
    with open(path, 'w', newline='') as f:
        csv.writer(f).writerows(rows)


def _read(path):
    with open(path) as f:
        return list(csv.reader(f))


def _polymers(n, rng):
    rows, graphs, fas = [], [], []
    for k in range(n):
        fa = float(rng.choice([0.25, 0.5, 0.75]))
        s = f'[*:1]c1ccc([*:2])cc1.[*:3]CC[*:4]|{fa}|{1 - fa}|<1-3:0.5:0.5<2-4:0.5:0.5<1-2:0.5:0.5~{10:g}'
        rows.append(s)
        graphs.append(polymer.synthetic_polymer_graph(s, seed=k))
        fas.append(fa)
    return rows, graphs, fas


def _cli_data(tmp, n=16):
    """16 synthetic polymers with one regression target and a three-column features file (a constant column, a NaN
    cell), as test_features_gpu builds them."""
    rng = np.random.default_rng(4)
    smiles, graphs, fas = _polymers(n, rng)
    rows = [[s, f'{2 * fa + 0.1 * rng.normal():.6g}'] for s, fa in zip(smiles, fas)]
    feats = rng.standard_normal((n, 3)) * np.array([3.0, 1.0, 10.0]) + np.array([1.0, 0.0, -5.0])
    feats[:, 1] = 2.5
    feats[3, 2] = np.nan
    paths = {k: str(tmp / v) for k, v in (('csv', 'd.csv'), ('npz', 'd.npz'), ('feat', 'f.csv'))}
    _write(paths['csv'], [['smiles', 'y']] + rows)
    save_graphs(paths['npz'], graphs)
    _write(paths['feat'], [['f0', 'f1', 'f2']] + [['nan' if np.isnan(v) else repr(float(v)) for v in r] for r in feats])
    return paths, feats


def _train_argv(paths):
    return ['--data_path', paths['csv'], '--graphs_path', paths['npz'], '--polymer', '--epochs', '2',
            '--warmup_epochs', '1', '--batch_size', '4', '--hidden_size', '48']


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """One ``chemprop_train --ensemble_size 2`` regression run, shared by the tests below."""
    tmp = tmp_path_factory.mktemp('ensemble')
    paths, feats = _cli_data(tmp)
    d = tmp / 'e'
    scores = cli.chemprop_train(_train_argv(paths) + ['--ensemble_size', '2', '--save_dir', str(d)])
    return dict(tmp=tmp, paths=paths, feats=feats, dir=d, scores=scores,
                ckpts=[str(d / f'model_{k}' / 'best_model.pt') for k in range(2)])


def test_ensemble_training_writes_one_directory_per_model(run):
    d = run['dir']
    for k in range(2):
        assert sorted(os.listdir(d / f'model_{k}')) == ['best_model.pt', 'model.pt', 'test_scores.json',
                                                        'train_val_loss_log.csv']
        own = json.load(open(d / f'model_{k}' / 'test_scores.json'))
        assert set(own) == {'rmse'} and np.isfinite(own['rmse'][0])
        assert len(_read(d / f'model_{k}' / 'train_val_loss_log.csv')) == 3
    assert sorted(os.listdir(d)) == ['model_0', 'model_1', 'split_indices.json', 'test_preds.csv', 'test_scores.csv',
                                     'test_scores.json']
    assert json.load(open(d / 'test_scores.json')) == run['scores'] and np.isfinite(run['scores']['rmse'][0])
    states = [torch.load(p, weights_only=True) for p in run['ckpts']]
    assert any(not torch.equal(states[0]['state_dict'][k], states[1]['state_dict'][k]) for k in states[0]['state_dict'])
    for s in states:  # the checkpoints carry what chemprop_predict reads
        assert s['args']['task_names'] == ['y'] and s['args']['ensemble_size'] == 2 and s['args']['polymer'] is True
    split = json.load(open(d / 'split_indices.json'))
    assert len(split['test']) == 2 and len(split['best_epoch']) == 2


def test_test_preds_are_the_float64_mean_of_the_models(run):
    split = json.load(open(run['dir'] / 'split_indices.json'))
    graphs = load_graphs(run['paths']['npz'])
    test_graphs = [graphs[i] for i in split['test']]
    mean, var, ind = predict_ensemble(run['ckpts'], test_graphs, 4, variance=True, individual=True)
    assert mean.dtype == np.float64 and mean.shape == (2, 1) and var.shape == (2, 1) and ind.shape == (2, 2, 1)
    written = _read(run['dir'] / 'test_preds.csv')
    assert written[0] == ['smiles', 'y'] and len(written) == 3
    got = np.array([[float(c) for c in r[1:]] for r in written[1:]])
    bound = 4 * EPS * 2 * np.abs(ind).max()
    assert np.all(np.abs(got - ind.sum(axis=0) / 2) <= bound) and np.all(np.abs(got - mean) <= bound)
    assert np.all(np.abs(var - np.var(ind, axis=0)) <= 16 * EPS * 2 * (np.abs(mean) + np.sqrt(var)) * np.sqrt(var))
    assert np.all(ind[0] != ind[1])
    # each model's own predictions: the untouched per-model loop on that checkpoint
    for k, path in enumerate(run['ckpts']):
        m = cli.load_checkpoint(path, 'cuda:0')
        own = np.array(cli.predict(m, graphs, split['test'], 4, cli.load_scalers(path)[0]))
        assert golden_io.normwise(ind[k], own) <= 1e-5
    # models handed over one by one, from a generator
    gen = ((cli.load_checkpoint(p, 'cuda:0'),) + tuple(cli.load_scalers(p)[:2]) for p in run['ckpts'])
    again = predict_ensemble(gen, test_graphs, 4, individual=True, n_models=2)
    assert np.array_equal(again[0], mean) and again[1] is None and np.array_equal(again[2], ind)
    with pytest.raises(ValueError):  # a model without input features, given features
        predict_ensemble(run['ckpts'], test_graphs, 4, features=np.zeros((2, 3)))


def test_default_layout_is_unchanged(run):
    """Without ``--ensemble_size`` (and with ``--ensemble_size 1``) the run writes what it always wrote; model 0 of
    the ensemble is that very model: same seed, same stream of shuffles."""
    for extra, name in (([], 's'), (['--ensemble_size', '1'], 's1')):
        d = run['tmp'] / name
        cli.chemprop_train(_train_argv(run['paths']) + extra + ['--save_dir', str(d)])
        assert sorted(os.listdir(d)) == ['best_model.pt', 'model.pt', 'split_indices.json', 'test_preds.csv',
                                         'test_scores.csv', 'test_scores.json', 'train_val_loss_log.csv']
        single = torch.load(str(d / 'best_model.pt'), weights_only=True)
        first = torch.load(run['ckpts'][0], weights_only=True)
        assert all(torch.equal(single['state_dict'][k], first['state_dict'][k]) for k in first['state_dict'])
        assert isinstance(json.load(open(d / 'split_indices.json'))['best_epoch'], int)


def test_chemprop_predict_on_a_checkpoint_directory(run):
    out = str(run['tmp'] / 'preds' / 'p.csv')
    mean = cli.chemprop_predict(['--test_path', run['paths']['csv'], '--graphs_path', run['paths']['npz'],
                                 '--preds_path', out, '--checkpoint_dir', str(run['dir']), '--batch_size', '4',
                                 '--ensemble_variance', '--individual_ensemble_predictions'])
    rows = _read(out)
    # the task column replaces the input's target column of the same name, as the reference's row dict does
    assert rows[0] == ['smiles', 'y', 'y_model_0', 'y_model_1', 'y_epi_unc'] and len(rows) == 17
    assert [r[0] for r in rows[1:]] == [r[0] for r in _read(run['paths']['csv'])[1:]]
    vals = np.array([[float(c) for c in r[1:]] for r in rows[1:]])
    y, models, unc = vals[:, 0], vals[:, 1:3], vals[:, 3]
    assert np.array_equal(y, mean[:, 0])
    assert np.all(np.abs(y - models.mean(axis=1)) <= 4 * EPS * 2 * np.abs(models).max(axis=1))
    sd = models.std(axis=1)
    assert np.all(np.abs(unc - np.var(models, axis=1)) <= 16 * EPS * 2 * (np.abs(y) + sd) * sd) and np.all(unc > 0)
    # one checkpoint, the SMILES column alone
    one = str(run['tmp'] / 'preds' / 'one.csv')
    cli.chemprop_predict(['--test_path', run['paths']['csv'], '--graphs_path', run['paths']['npz'], '--preds_path', one,
                          '--checkpoint_path', run['ckpts'][1], '--drop_extra_columns'])
    rows = _read(one)
    assert rows[0] == ['smiles', 'y'] and len(rows) == 17
    assert golden_io.normwise(np.array([float(r[1]) for r in rows[1:]]), models[:, 1]) <= 1e-5


def test_ensemble_with_a_features_file(run):
    paths, feats = run['paths'], run['feats']
    d = run['tmp'] / 'f'
    cli.chemprop_train(_train_argv(paths) + ['--features_path', paths['feat'], '--ensemble_size', '2',
                                             '--save_dir', str(d)])
    ckpts = [str(d / f'model_{k}' / 'best_model.pt') for k in range(2)]
    graphs = load_graphs(paths['npz'])
    mean, _, ind = predict_ensemble(ckpts, graphs, 4, features=feats, individual=True)
    assert mean.shape == (16, 1) and np.isfinite(mean).all()
    for k, path in enumerate(ckpts):  # each model's own features scaler, then the per-model loop
        data_scaler, features_scaler = cli.load_scalers(path)[:2]
        m = cli.load_checkpoint(path, 'cuda:0')
        assert m.ffn[1].in_features == 51
        own = np.array(cli.predict(m, graphs, list(range(16)), 4, data_scaler, None, features_scaler.transform(feats)))
        assert golden_io.normwise(ind[k], own) <= 1e-5
    split = json.load(open(d / 'split_indices.json'))
    written = np.array([[float(c) for c in r[1:]] for r in _read(d / 'test_preds.csv')[1:]])
    assert np.all(np.abs(written - mean[split['test']]) <= 4 * EPS * 2 * np.abs(ind).max())
    # the features matter, and so does their scaling
    other = predict_ensemble(ckpts, graphs, 4, features=feats[::-1].copy())[0]
    assert not np.allclose(other, mean, rtol=1e-5, atol=0)
    raw = predict_ensemble(ckpts, graphs, 4, features=np.nan_to_num(feats), features_scaling=False)[0]
    assert not np.allclose(raw, mean, rtol=1e-5, atol=0)
    with pytest.raises(ValueError):
        predict_ensemble(ckpts, graphs, 4)                               # features missing
    with pytest.raises(ValueError):
        predict_ensemble(ckpts, graphs, 4, features=feats[:, :2])        # another width
    with pytest.raises(ValueError):                                      # a regression and a features model
        cli.chemprop_predict(['--test_path', paths['csv'], '--graphs_path', paths['npz'], '--preds_path',
                              str(run['tmp'] / 'x.csv'), '--checkpoint_paths', run['ckpts'][0], ckpts[0]])
    out = str(run['tmp'] / 'pf.csv')
    got = cli.chemprop_predict(['--test_path', paths['csv'], '--graphs_path', paths['npz'], '--preds_path', out,
                                '--checkpoint_dir', str(d), '--features_path', paths['feat'], '--batch_size', '4'])
    assert np.array_equal(got, mean) and _read(out)[0] == ['smiles', 'y']


def test_models_the_native_head_refuses_take_their_own_forward():
    """70 regression outputs are beyond the native heads (64): ``predict_ensemble`` runs ``model(...)`` per batch
    into the same accumulator.  And the torch normalisation that path gives a spectra model is the native one."""
    from chemprop_amd import TrainArgs, ensemble, train
    from chemprop_amd.featurization import BatchMolGraph
    from chemprop_amd.model import MoleculeModel
    _, graphs, _ = _polymers(10, np.random.default_rng(2))
    members = []
    for k in range(2):
        torch.manual_seed(k)
        m = MoleculeModel(TrainArgs(hidden_size=48, num_tasks=70, device=DEV)).to(DEV).eval()
        assert train._predict_head(m) is None
        members.append(m)
    mean, var, ind = predict_ensemble(members, graphs, 4, variance=True, individual=True)
    with torch.no_grad():
        want = np.stack([torch.cat([m([BatchMolGraph(graphs[s:s + 4])]) for s in range(0, 10, 4)]).cpu().numpy()
                         for m in members]).astype(np.float64)
    assert ind.shape == (2, 10, 70) and np.array_equal(ind, want)
    assert np.all(np.abs(mean - want.sum(axis=0) / 2) <= 4 * EPS * 2 * np.abs(want).max(axis=0))
    sd = want.std(axis=0)
    assert np.all(np.abs(var - np.var(want, axis=0)) <= 16 * EPS * 2 * (np.abs(mean) + sd) * sd)
    torch.manual_seed(3)
    s = MoleculeModel(TrainArgs(hidden_size=48, num_tasks=T_SPEC, dataset_type='spectra', device=DEV)).to(DEV).eval()
    g = BatchMolGraph(graphs[:4])
    mask = torch.ones((4, T_SPEC), dtype=torch.bool, device=DEV)
    mask[1, T_SPEC - 3:] = False
    with torch.no_grad():
        native = train.head_predict(s, s.encoder([g]), normalize=True, mask=mask).cpu().numpy()
        torch_path = ensemble._fallback_predict(s, g, None, mask).cpu().numpy()
    assert np.array_equal(np.isnan(native), ~mask.cpu().numpy()) and np.array_equal(np.isnan(torch_path), np.isnan(native))
    assert golden_io.normwise(np.nan_to_num(torch_path), np.nan_to_num(native)) <= 1e-5


T_SPEC = 12


def _pairwise_sid(models):
    """spectra_utils-style pairwise SID of ``[M][T]`` spectra (NaN in model 0 = excluded), in numpy."""
    keep = ~np.isnan(models[0])
    p = models[:, keep]
    total, pairs = 0.0, 0
    for a in range(len(p)):
        for b in range(a + 1, len(p)):
            total += float(np.sum(p[a] * np.log(p[a] / p[b]) + p[b] * np.log(p[b] / p[a])))
            pairs += 1
    return total / pairs


def test_spectra_ensemble_end_to_end(tmp_path):
    rng = np.random.default_rng(9)
    smiles, graphs, fas = _polymers(16, rng)
    rows = []
    for s, fa in zip(smiles, fas):
        spec = np.exp(-0.5 * ((np.arange(T_SPEC) - (2 + 8 * fa)) / 2.0) ** 2) + 0.05 * rng.random(T_SPEC)
        rows.append([s] + [f'{v:.6g}' for v in spec])
    phases = [k % 2 for k in range(16)]
    names = [f'b{t}' for t in range(T_SPEC)]
    paths = {k: str(tmp_path / v) for k, v in (('csv', 's.csv'), ('npz', 's.npz'), ('phase', 'ph.csv'), ('mask', 'm.csv'))}
    _write(paths['csv'], [['smiles'] + names] + rows)
    save_graphs(paths['npz'], graphs)
    _write(paths['phase'], [['p0', 'p1']] + [[int(p == 0), int(p == 1)] for p in phases])
    _write(paths['mask'], [['phase'] + names, ['p0'] + [1] * T_SPEC, ['p1'] + [1] * (T_SPEC - 3) + [0] * 3])
    d = tmp_path / 'e'
    scores = cli.chemprop_train(_train_argv(paths) + ['--dataset_type', 'spectra', '--phase_features_path', paths['phase'],
                                                      '--spectra_phase_mask_path', paths['mask'], '--ensemble_size', '2',
                                                      '--save_dir', str(d)])
    assert set(scores) == {'sid'} and np.isfinite(scores['sid'][0])
    split = json.load(open(d / 'split_indices.json'))
    for i, r in zip(split['test'], _read(d / 'test_preds.csv')[1:]):
        assert [c == '' for c in r[1:]] == [phases[i] == 1 and t >= T_SPEC - 3 for t in range(T_SPEC)]
    out = str(tmp_path / 'p.csv')
    cli.chemprop_predict(['--test_path', paths['csv'], '--graphs_path', paths['npz'], '--preds_path', out,
                          '--checkpoint_dir', str(d), '--phase_features_path', paths['phase'], '--batch_size', '4',
                          '--ensemble_variance', '--individual_ensemble_predictions', '--drop_extra_columns'])
    got = _read(out)
    assert got[0] == ['smiles'] + names + [f'{n}_model_{k}' for n in names for k in range(2)] + ['epi_unc']
    assert len(got) == 17
    for i, r in enumerate(got[1:]):
        cells = np.array([float('nan') if c == '' else float(c) for c in r[1:]])
        mean, models, unc = cells[:T_SPEC], cells[T_SPEC:3 * T_SPEC].reshape(T_SPEC, 2).T, cells[-1]
        excluded = np.array([phases[i] == 1 and t >= T_SPEC - 3 for t in range(T_SPEC)])
        assert np.array_equal(np.isnan(mean), excluded)
        assert np.array_equal(np.isnan(models), np.stack([excluded, excluded]))
        assert abs(np.nansum(models[0]) - 1) <= 1e-5 and abs(np.nansum(models[1]) - 1) <= 1e-5
        assert np.all(np.abs(mean - models.mean(axis=0))[~excluded] <= 4 * EPS * 2 * models.max(axis=0)[~excluded])
        want = _pairwise_sid(models)
        assert want > 0 and abs(unc - want) <= 1e-9 * want, (i, unc, want)
    # one spectra model: no pairs, the spread is NaN (an empty cell)
    one = str(tmp_path / 'one.csv')
    cli.chemprop_predict(['--test_path', paths['csv'], '--graphs_path', paths['npz'], '--preds_path', one,
                          '--checkpoint_path', str(d / 'model_0' / 'best_model.pt'), '--phase_features_path',
                          paths['phase'], '--ensemble_variance', '--drop_extra_columns'])
    rows = _read(one)
    assert rows[0] == ['smiles'] + names + ['epi_unc'] and all(r[-1] == '' for r in rows[1:])


def test_multiclass_ensemble_end_to_end(tmp_path):
    rng = np.random.default_rng(11)
    smiles, graphs, fas = _polymers(16, rng)
    paths = {'csv': str(tmp_path / 'm.csv'), 'npz': str(tmp_path / 'm.npz')}
    _write(paths['csv'], [['smiles', 'kind']] + [[s, str(int(4 * fa) - 1)] for s, fa in zip(smiles, fas)])
    save_graphs(paths['npz'], graphs)
    d = tmp_path / 'e'
    scores = cli.chemprop_train(_train_argv(paths) + ['--dataset_type', 'multiclass', '--multiclass_num_classes', '3',
                                                      '--ensemble_size', '2', '--save_dir', str(d)])
    assert set(scores) == {'cross_entropy'} and np.isfinite(scores['cross_entropy'][0])
    cols = [f'kind_class_{i}' for i in range(3)]
    written = _read(d / 'test_preds.csv')
    assert written[0] == ['smiles'] + cols and len(written) == 3
    out = str(tmp_path / 'p.csv')
    mean = cli.chemprop_predict(['--test_path', paths['csv'], '--graphs_path', paths['npz'], '--preds_path', out,
                                 '--checkpoint_dir', str(d), '--batch_size', '4', '--ensemble_variance',
                                 '--individual_ensemble_predictions'])
    assert mean.shape == (16, 3)
    got = _read(out)
    assert got[0] == ['smiles', 'kind'] + cols + [f'{c}_model_{k}' for c in cols for k in range(2)] + \
        [f'{c}_epi_unc' for c in cols]
    vals = np.array([[float(c) for c in r[2:]] for r in got[1:]])
    probs, models, unc = vals[:, :3], vals[:, 3:9].reshape(16, 3, 2), vals[:, 9:]
    assert np.allclose(probs.sum(axis=1), 1, rtol=0, atol=1e-6) and np.all(probs > 0)
    assert np.allclose(models.sum(axis=1), 1, rtol=0, atol=1e-6)
    assert np.all(np.abs(probs - models.mean(axis=2)) <= 4 * EPS * 2 * models.max(axis=2))
    sd = models.std(axis=2)
    assert np.all(np.abs(unc - np.var(models, axis=2)) <= 16 * EPS * 2 * (probs + sd) * sd)
    split = json.load(open(d / 'split_indices.json'))
    test_rows = np.array([[float(c) for c in r[1:]] for r in written[1:]])
    assert np.all(np.abs(test_rows - probs[split['test']]) <= 4 * EPS * 2 * models.max(axis=2)[split['test']])
