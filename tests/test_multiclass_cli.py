"""``chemprop_train --dataset_type multiclass`` (chemprop_amd.cli): the flags, class-index targets, the
``cross_entropy`` and ``accuracy`` metrics (evaluate.py:72-74, utils.py:416-432), per-class prediction
columns, and on the GPU an end-to-end run on a generated polymer set."""
import csv
import json
import math

import numpy as np
import pytest

from chemprop_amd import cli, polymer
from chemprop_amd.graph_io import save_graphs

ARGV = ['--data_path', 'd.csv', '--graphs_path', 'g.npz', '--save_dir', 'out']


def test_parse_args_accepts_multiclass():
    a = cli.parse_args(ARGV + ['--dataset_type', 'multiclass', '--multiclass_num_classes', '4'])
    assert a.dataset_type == 'multiclass' and a.multiclass_num_classes == 4
    assert cli.parse_args(ARGV + ['--dataset_type', 'multiclass']).multiclass_num_classes == 3
    assert cli.parse_args(ARGV).dataset_type == 'regression'
    with pytest.raises(SystemExit):
        cli.parse_args(ARGV + ['--dataset_type', 'spectra'])


# four rows, three classes; class 2 never occurs among the targets (log_loss needs labels= for that)
PROBS = [[0.7, 0.2, 0.1], [0.1, 0.8, 0.1], [0.3, 0.4, 0.3], [0.2, 0.3, 0.5]]
CLASSES = [0, 1, 1, 0]


def test_multiclass_metrics_on_a_hand_computed_example():
    ce = -(math.log(0.7) + math.log(0.8) + math.log(0.4) + math.log(0.2)) / 4
    assert cli.metric_value('cross_entropy', CLASSES, PROBS) == pytest.approx(ce, rel=1e-12)
    assert cli.metric_value('accuracy', CLASSES, PROBS) == 0.75  # argmax: 0, 1, 1, 2
    # every class present: the same formula
    ce3 = -(math.log(0.7) + math.log(0.8) + math.log(0.3) + math.log(0.5)) / 4
    assert cli.metric_value('cross_entropy', [0, 1, 2, 2], PROBS) == pytest.approx(ce3, rel=1e-12)
    assert cli.metric_value('accuracy', [0, 1, 2, 2], PROBS) == 0.75
    # scalar predictions: a 0.5 threshold (above = 1)
    assert cli.metric_value('accuracy', [1, 0, 0, 1], [0.9, 0.2, 0.6, 0.5]) == 0.5
    with pytest.raises(ValueError):
        cli.metric_value('no_such_metric', CLASSES, PROBS)


def test_evaluate_predictions_with_class_probabilities_and_a_missing_target():
    """[N][tasks][C] predictions, per task over the rows that have a target."""
    second = [[0.2, 0.2, 0.6], [0.5, 0.25, 0.25], [0.1, 0.1, 0.8], [0.3, 0.6, 0.1]]
    preds = [[a, b] for a, b in zip(PROBS, second)]
    targets = [[0, 2], [1, None], [1, 2], [0, 0]]
    res = cli.evaluate_predictions(preds, targets, 2, ['cross_entropy', 'accuracy'], 'multiclass')
    ce0 = -(math.log(0.7) + math.log(0.8) + math.log(0.4) + math.log(0.2)) / 4
    ce1 = -(math.log(0.6) + math.log(0.8) + math.log(0.3)) / 3  # (row 1 has no target for task 1)
    assert res['cross_entropy'] == pytest.approx([ce0, ce1], rel=1e-12)
    assert res['accuracy'] == pytest.approx([0.75, 2 / 3], rel=1e-12)


def _write(path, rows):
    with open(path, 'w', newline='') as f:
        csv.writer(f).writerows(rows)


def test_class_targets_are_read_as_indices_or_refused_with_the_csv_row(tmp_path):
    p = str(tmp_path / 'c.csv')
    _write(p, [['smiles', 'a', 'b'], ['C', '0', '2'], ['CC', '', '1.0'], [], ['CCC', '2', '']])
    assert cli.read_class_targets(p, 3) == [[0, 2], [None, 1], [2, None]]
    for cell in ('3', '-1', '1.5', 'x', 'nan'):
        _write(p, [['smiles', 'a', 'b'], ['C', '0', '2'], ['CC', '1', cell]])
        with pytest.raises(ValueError, match=r'row 3, column 3'):
            cli.read_class_targets(p, 3)


def _polymer_classes(tmp_path, n=60):
    """n synthetic polymer rows (as test_chemprop_train_learns_on_synthetic_polymers builds them) whose class is
    the bucket of the first monomer's fraction."""
    rng = np.random.default_rng(5)
    fractions = [0.25, 0.5, 0.75]
    rows, graphs = [], []
    for k in range(n):
        c = int(rng.integers(3))
        fa = fractions[c]
        xn = float(rng.choice([1, 10, 100, 1000]))
        s = f'[*:1]c1ccc([*:2])cc1.[*:3]CC[*:4]|{fa}|{1 - fa}|<1-3:0.5:0.5<2-4:0.5:0.5<1-2:0.5:0.5~{xn:g}'
        rows.append([s, c])
        graphs.append(polymer.synthetic_polymer_graph(s, seed=k))
    csv_path, npz_path = str(tmp_path / 'p.csv'), str(tmp_path / 'p.npz')
    _write(csv_path, [['smiles', 'y']] + rows)
    save_graphs(npz_path, graphs)
    return csv_path, npz_path


@pytest.mark.gpu
def test_chemprop_train_multiclass_end_to_end(tmp_path):
    """60 polymer rows in 3 classes, 8 epochs: deterministic test scores, per-class prediction columns that sum
    to 1, a checkpoint that reloads as a multiclass model, and a training cross-entropy that ends below its
    first epoch's value and below log(3) (the uniform guess)."""
    csv_path, npz_path = _polymer_classes(tmp_path)
    argv = ['--data_path', csv_path, '--graphs_path', npz_path, '--dataset_type', 'multiclass', '--polymer',
            '--epochs', '8', '--batch_size', '12', '--extra_metrics', 'accuracy', '--save_dir']
    s1 = cli.chemprop_train(argv + [str(tmp_path / 'a')])
    s2 = cli.chemprop_train(argv + [str(tmp_path / 'b')])
    assert s1 == s2 and set(s1) == {'cross_entropy', 'accuracy'}
    assert len(s1['cross_entropy']) == 1 and math.isfinite(s1['cross_entropy'][0])
    d = tmp_path / 'a'
    assert json.load(open(d / 'test_scores.json')) == s1
    preds = list(csv.reader(open(d / 'test_preds.csv')))
    assert preds[0] == ['smiles', 'y_class_0', 'y_class_1', 'y_class_2'] and len(preds) == 1 + 6
    for r in preds[1:]:
        p = [float(x) for x in r[1:]]
        assert abs(sum(p) - 1) <= 1e-5 and min(p) >= 0
    m = cli.load_checkpoint(str(d / 'best_model.pt'))
    assert m.multiclass and m.num_classes == 3 and m.ffn[4].out_features == 3
    log = list(csv.reader(open(d / 'train_val_loss_log.csv')))
    col = log[0].index('train_avg_cross_entropy')
    first, last = float(log[1][col]), float(log[-1][col])
    assert len(log) == 1 + 8 and last < first and last < math.log(3), (first, last)


def test_chemprop_train_refuses_a_bad_class_before_training(tmp_path):
    """The CSV is checked before a model is built or the GPU touched (no GPU is needed to be refused)."""
    csv_path, npz_path = _polymer_classes(tmp_path, 12)
    rows = list(csv.reader(open(csv_path)))
    rows[5][1] = '3'
    _write(csv_path, rows)
    with pytest.raises(ValueError, match='row 6'):
        cli.chemprop_train(['--data_path', csv_path, '--graphs_path', npz_path, '--dataset_type', 'multiclass',
                            '--polymer', '--epochs', '1', '--save_dir', str(tmp_path / 'o')])
    assert not (tmp_path / 'o' / 'model.pt').exists()
