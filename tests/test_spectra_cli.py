"""``chemprop_train --dataset_type spectra``: the arguments, the metric validation, the phase files, and one run end
to end on the GPU (normalised targets, phase features as input features, predictions normalised on the device
under the phase mask, the checkpoint)."""
import csv
import json
import math

import numpy as np
import pytest
import torch

from chemprop_amd import cli, polymer, spectra_utils
from chemprop_amd.graph_io import load_graphs, save_graphs

ARGV = ['--data_path', 'd.csv', '--graphs_path', 'g.npz', '--save_dir', 'out']


def test_parse_args_accepts_the_spectra_flags():
    """``parse_args(argv, spectra=True)`` is the parser ``chemprop_train`` uses; without the keyword the parser keeps
    refusing ``--dataset_type spectra`` (an existing test pins that)."""
    with pytest.raises(SystemExit):
        cli.parse_args(ARGV + ['--dataset_type', 'spectra'])
    a = cli.parse_args(ARGV + ['--dataset_type', 'spectra'], spectra=True)
    assert a.dataset_type == 'spectra' and a.spectra_activation == 'exp' and a.spectra_target_floor == 1e-8
    assert a.alternative_loss_function is None and a.spectra_phase_mask_path is None and a.phase_features_path is None
    a = cli.parse_args(ARGV + ['--dataset_type', 'spectra', '--spectra_activation', 'softplus',
                               '--spectra_target_floor', '1e-6', '--alternative_loss_function', 'wasserstein',
                               '--spectra_phase_mask_path', 'm.csv', '--phase_features_path', 'p.csv',
                               '--metric', 'wasserstein', '--extra_metrics', 'sid'], spectra=True)
    assert (a.spectra_activation, a.spectra_target_floor, a.alternative_loss_function) == ('softplus', 1e-6, 'wasserstein')
    assert (a.spectra_phase_mask_path, a.phase_features_path, a.metric, a.extra_metrics) == \
        ('m.csv', 'p.csv', 'wasserstein', ['sid'])
    assert cli.parse_args(ARGV, spectra=True).dataset_type == 'regression'
    with pytest.raises(SystemExit):
        cli.parse_args(ARGV + ['--dataset_type', 'spectra', '--spectra_activation', 'relu'], spectra=True)
    with pytest.raises(SystemExit):
        cli.parse_args(ARGV + ['--dataset_type', 'spectra', '--alternative_loss_function', 'mse'], spectra=True)


def test_metric_validation_follows_the_dataset_type():
    with pytest.raises(ValueError, match='Metric "rmse" invalid for dataset type "spectra"'):
        cli.parse_args(ARGV + ['--dataset_type', 'spectra', '--metric', 'rmse'], spectra=True)
    with pytest.raises(ValueError, match='Metric "sid" invalid for dataset type "regression"'):
        cli.parse_args(ARGV + ['--metric', 'sid'], spectra=True)
    with pytest.raises(ValueError, match='wasserstein'):
        cli.parse_args(ARGV + ['--dataset_type', 'multiclass', '--extra_metrics', 'wasserstein'], spectra=True)
    with pytest.raises(ValueError, match='Alternative loss'):
        cli.parse_args(ARGV + ['--alternative_loss_function', 'wasserstein'], spectra=True)
    with pytest.raises(ValueError, match='spectra_target_floor'):
        cli.parse_args(ARGV + ['--dataset_type', 'spectra', '--spectra_target_floor', '0'], spectra=True)
    assert cli.parse_args(ARGV + ['--metric', 'mae', '--extra_metrics', 'r2'], spectra=True).metric == 'mae'


def test_spectra_scores_cover_all_positions_together():
    preds = [[0.2, 0.3, 0.5], [1.0, 1.0, None]]
    targets = [[0.25, 0.25, 0.5], [0.4, 0.6, None]]
    res = cli.evaluate_predictions(preds, targets, 3, ['sid', 'wasserstein'], 'spectra')
    assert res == {'sid': [spectra_utils.sid_metric(preds, targets)],
                   'wasserstein': [spectra_utils.wasserstein_metric(preds, targets)]}
    q = np.array([[0.2, 0.3, 0.5], [0.5, 0.5, 1.0]])
    y = np.array([[0.25, 0.25, 0.5], [0.4, 0.6, 1.0]])
    assert res['sid'][0] == pytest.approx(float(np.mean((q * np.log(q / y) + y * np.log(y / q)).sum(axis=1))), rel=1e-12)
    assert math.isnan(cli.evaluate_predictions([], [], 3, ['sid'], 'spectra')['sid'][0])


def _write(path, rows):
    with open(path, 'w', newline='') as f:
        csv.writer(f).writerows(rows)


def test_phase_files_are_read_and_checked(tmp_path):
    p = str(tmp_path / 'phase.csv')
    _write(p, [['gas', 'liquid'], ['1', '0'], ['0', '1'], ['0', '1']])
    assert cli.load_phase_features(p, 3).tolist() == [[1, 0], [0, 1], [0, 1]]
    with pytest.raises(ValueError, match='2 CSV rows'):
        cli.load_phase_features(p, 2)
    _write(p, [['gas', 'liquid'], ['1', '1']])
    with pytest.raises(ValueError, match='one-hot'):
        cli.load_phase_features(p, 1)
    m = str(tmp_path / 'mask.csv')
    _write(m, [['phase', 'a', 'b', 'c'], ['gas', '1', '1', '0'], ['liquid', '0', '1', '1']])
    assert spectra_utils.load_phase_mask(m) == [[1, 1, 0], [0, 1, 1]]
    _write(m, [['phase', 'a'], ['gas', '2']])
    with pytest.raises(ValueError, match='0s and 1s'):
        spectra_utils.load_phase_mask(m)


T, PHASES = 33, 2


def _spectra_data(tmp_path, n=12):
    """n synthetic polymer rows with T = 33 spectrum bins, alternating between 2 phases; phase 1 excludes the last
    8 bins; a few cells are empty."""
    rng = np.random.default_rng(9)
    rows, graphs, phases = [], [], []
    for k in range(n):
        fa = float(rng.choice([0.25, 0.5, 0.75]))
        s = f'[*:1]c1ccc([*:2])cc1.[*:3]CC[*:4]|{fa}|{1 - fa}|<1-3:0.5:0.5<2-4:0.5:0.5<1-2:0.5:0.5~{10:g}'
        centre = 8 + 16 * fa
        spec = np.exp(-0.5 * ((np.arange(T) - centre) / 4.0) ** 2) + 0.05 * rng.random(T)
        cells = ['' if rng.random() < 0.05 else f'{v:.6g}' for v in spec]
        rows.append([s] + cells)
        graphs.append(polymer.synthetic_polymer_graph(s, seed=k))
        phases.append(k % PHASES)
    paths = {k: str(tmp_path / v) for k, v in (('csv', 's.csv'), ('npz', 's.npz'), ('phase', 'phase.csv'),
                                               ('mask', 'mask.csv'))}
    _write(paths['csv'], [['smiles'] + [f'b{t}' for t in range(T)]] + rows)
    save_graphs(paths['npz'], graphs)
    _write(paths['phase'], [['p0', 'p1']] + [[int(p == 0), int(p == 1)] for p in phases])
    _write(paths['mask'], [['phase'] + [f'b{t}' for t in range(T)], ['p0'] + [1] * T,
                           ['p1'] + [1] * (T - 8) + [0] * 8])
    return paths, phases


@pytest.mark.gpu
def test_chemprop_train_spectra_end_to_end(tmp_path):
    """12 rows, 33 bins, 2 phases, 2 epochs: one finite sid score, test predictions that sum to 1 over their
    non-empty cells with the phase-excluded cells empty, a checkpoint that reloads as a spectra model and
    reproduces the predictions; then the Wasserstein loss and metric."""
    paths, phases = _spectra_data(tmp_path)
    argv = ['--data_path', paths['csv'], '--graphs_path', paths['npz'], '--dataset_type', 'spectra', '--polymer',
            '--epochs', '2', '--warmup_epochs', '1', '--batch_size', '4', '--hidden_size', '48',
            '--split_sizes', '0.5', '0.25', '0.25',
            '--phase_features_path', paths['phase'], '--spectra_phase_mask_path', paths['mask'], '--save_dir']
    d = tmp_path / 'a'
    scores = cli.chemprop_train(argv + [str(d)])
    assert set(scores) == {'sid'} and len(scores['sid']) == 1 and math.isfinite(scores['sid'][0])
    assert json.load(open(d / 'test_scores.json')) == scores
    split = json.load(open(d / 'split_indices.json'))
    preds = list(csv.reader(open(d / 'test_preds.csv')))
    assert preds[0] == ['smiles'] + [f'b{t}' for t in range(T)] and len(preds) == 1 + len(split['test']) == 4
    got = []
    for i, r in zip(split['test'], preds[1:]):
        cells = r[1:]
        empty = [c == '' for c in cells]
        assert empty == [phases[i] == 1 and t >= T - 8 for t in range(T)]
        vals = [float(c) for c in cells if c != '']
        assert abs(sum(vals) - 1) <= 1e-5 and min(vals) > 0
        got.append([float('nan') if c == '' else float(c) for c in cells])
    assert any(phases[i] == 1 for i in split['test'])
    m = cli.load_checkpoint(str(d / 'best_model.pt'), 'cuda:0')
    assert m.spectra and m.ffn[4].out_features == T and m.ffn[1].in_features == 48 + PHASES
    assert type(m.ffn[5]).__name__ == '_Exp'
    state = torch.load(str(d / 'best_model.pt'), weights_only=True)
    assert state['args']['dataset_type'] == 'spectra' and state['args']['spectra_target_floor'] == 1e-8
    assert state['args']['phase_features_path'] == paths['phase'] and state['data_scaler'] is None
    graphs = load_graphs(paths['npz'])
    feats = cli.load_phase_features(paths['phase'], 12)
    mask = spectra_utils.phase_row_mask(feats, spectra_utils.load_phase_mask(paths['mask']))
    again = cli.predict(m, graphs, split['test'], 4, None, None, feats, mask[split['test']])
    again = np.array([[float('nan') if v is None else v for v in r] for r in again])
    assert np.array_equal(np.isnan(again), np.isnan(np.array(got)))
    assert np.allclose(np.nan_to_num(again), np.nan_to_num(np.array(got)), rtol=1e-5, atol=1e-9)
    log = list(csv.reader(open(d / 'train_val_loss_log.csv')))
    assert log[0] == ['epoch', 'train_loss', 'train_avg_sid', 'val_avg_sid'] and len(log) == 3
    assert all(math.isfinite(float(v)) for row in log[1:] for v in row)
    # the alternative loss and its metric
    w = cli.chemprop_train(argv + [str(tmp_path / 'w'), '--alternative_loss_function', 'wasserstein',
                                   '--metric', 'wasserstein'])
    assert set(w) == {'wasserstein'} and len(w['wasserstein']) == 1 and math.isfinite(w['wasserstein'][0])
