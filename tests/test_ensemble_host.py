"""Ensembles and ``chemprop_predict``, the host side (no GPU): ``wdmpnn_ensemble_add`` and ``wdmpnn_ensemble_sid``
are declared, bound and exported with the ABI still 12 and their structs laid out as a C compiler lays out the
header's; every refusal happens before a launch; ``parse_predict_args``, ``--checkpoint_dir`` discovery,
``write_predictions``' columns, ``--ensemble_size`` and the new ``TrainArgs`` fields."""
import csv
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from chemprop_amd import TrainArgs, _native, cli
from chemprop_amd.ensemble import EnsembleAccumulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1000, -1001, -1003
SYMBOLS = ('wdmpnn_ensemble_add', 'wdmpnn_ensemble_sid')


def test_header_binding_and_library_agree_on_the_ensemble_entry_points(tmp_path):
    text = open(HEADER).read()
    assert '#define WDMPNN_ABI_VERSION 12' in text and '#define WD_ENSEMBLE_MAX_MODELS 32' in text
    assert _native.ABI_VERSION == 12 and _native.ENSEMBLE_MAX_MODELS == 32
    assert re.search(r'\bint\s+wdmpnn_ensemble_add\s*\(\s*const\s+WdEnsembleAdd\s*\*', text)
    assert re.search(r'\bint\s+wdmpnn_ensemble_sid\s*\(\s*const\s+WdEnsembleSid\s*\*', text)
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    L = _native.lib()
    assert L.wdmpnn_abi_version() == 12
    for fn in SYMBOLS:
        assert fn in _native.EXPORTED_SYMBOLS
        assert re.search(rf'\bT {fn}\b', out)
    assert L.wdmpnn_ensemble_add.argtypes[0]._type_ is _native.WdEnsembleAdd
    assert L.wdmpnn_ensemble_sid.argtypes[0]._type_ is _native.WdEnsembleSid
    structs = (('WdEnsembleAdd', _native.WdEnsembleAdd), ('WdEnsembleSid', _native.WdEnsembleSid))
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wdmpnn.h"\nint main(void) {\n' +
                   ''.join(f'  printf(" %zu", sizeof({name}));\n' +
                           ''.join(f'  printf(" %zu", offsetof({name}, {n}));\n' for n, _ in S._fields_)
                           for name, S in structs) +
                   '  printf("\\n"); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC', 'gcc'), '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, S in structs:
        want += [ctypes.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert c == want


def _fake_add(**kw):
    """A WdEnsembleAdd of made-up addresses (never dereferenced: every call below is refused, or a no-op, on the
    host)."""
    e = _native.WdEnsembleAdd()
    d = dict(pred=4096, ld_pred=6, B=4, W=3, k=1, row0=2, scale_mean=None, scale_std=None, mean=8192, m2=12288,
             keep=None, ld_acc=4)
    d.update(kw)
    for name, v in d.items():
        setattr(e, name, v)
    return e


@pytest.mark.parametrize('kw,rc', [(dict(pred=None), ERR_ARG),
                                   (dict(mean=None), ERR_ARG),
                                   (dict(B=-1), ERR_SHAPE),
                                   (dict(W=0), ERR_SHAPE),
                                   (dict(W=-3), ERR_SHAPE),
                                   (dict(ld_pred=2), ERR_SHAPE),
                                   (dict(ld_acc=2), ERR_SHAPE),
                                   (dict(row0=-1), ERR_SHAPE),
                                   (dict(k=-1), ERR_SHAPE),
                                   (dict(scale_mean=4096), ERR_SHAPE),
                                   (dict(scale_std=4096), ERR_SHAPE),
                                   (dict(k=32), ERR_UNSUPPORTED),
                                   (dict(k=1000), ERR_UNSUPPORTED)])
def test_ensemble_add_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    got = L.wdmpnn_ensemble_add(ctypes.byref(_fake_add(**kw)), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()
    with pytest.raises((ValueError, NotImplementedError, _native.NativeError)):
        _native.check(got, 'ensemble add')


def test_ensemble_add_without_rows_is_a_no_op():
    L = _native.lib()
    assert L.wdmpnn_ensemble_add(None, None) == ERR_ARG
    assert L.wdmpnn_ensemble_add(ctypes.byref(_fake_add(B=0)), None) == 0
    assert L.wdmpnn_ensemble_add(ctypes.byref(_fake_add(B=0, pred=None, mean=None, m2=None)), None) == 0
    assert L.wdmpnn_ensemble_add(ctypes.byref(_fake_add(B=0, k=31)), None) == 0


def _fake_sid(**kw):
    s = _native.WdEnsembleSid()
    d = dict(preds=4096, model_stride=70, ld=35, M=3, N=2, T=33, threshold=0.0, out=8192)
    d.update(kw)
    for name, v in d.items():
        setattr(s, name, v)
    return s


@pytest.mark.parametrize('kw,rc', [(dict(M=0), ERR_SHAPE),
                                   (dict(M=-1), ERR_SHAPE),
                                   (dict(T=0), ERR_SHAPE),
                                   (dict(N=-1), ERR_SHAPE),
                                   (dict(ld=32), ERR_SHAPE),
                                   (dict(model_stride=69), ERR_SHAPE),
                                   (dict(model_stride=-70), ERR_SHAPE),
                                   (dict(M=33), ERR_UNSUPPORTED),
                                   (dict(preds=None), ERR_ARG),
                                   (dict(out=None), ERR_ARG)])
def test_ensemble_sid_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    got = L.wdmpnn_ensemble_sid(ctypes.byref(_fake_sid(**kw)), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()
    with pytest.raises((ValueError, NotImplementedError, _native.NativeError)):
        _native.check(got, 'ensemble sid')


def test_ensemble_sid_without_rows_is_a_no_op():
    L = _native.lib()
    assert L.wdmpnn_ensemble_sid(None, None) == ERR_ARG
    assert L.wdmpnn_ensemble_sid(ctypes.byref(_fake_sid(N=0, model_stride=0)), None) == 0


def test_accumulator_misuse_is_refused_on_the_host():
    """The order checks need no device: a CPU accumulator refuses before anything would launch."""
    with pytest.raises(ValueError):
        EnsembleAccumulator(4, 3, 'cpu', keep=True)                 # keep needs n_models
    with pytest.raises(ValueError):
        EnsembleAccumulator(4, 3, 'cpu', keep=True, n_models=33)
    with pytest.raises(ValueError):
        EnsembleAccumulator(4, 0, 'cpu')
    acc = EnsembleAccumulator(4, 3, 'cpu', variance=True)
    p = torch.zeros(2, 3)
    with pytest.raises(ValueError, match='width'):
        acc.add(torch.zeros(2, 4), 0, 0)
    with pytest.raises(ValueError):
        acc.add(p, 0, 1)                                            # model 1 before model 0
    with pytest.raises(ValueError):
        acc.add(p, 3, 0)                                            # rows 3 .. 5 of 4
    with pytest.raises(ValueError):
        acc.add(p.double(), 0, 0)
    with pytest.raises(ValueError):
        acc.mean()                                                  # no model yet
    acc._count[0:2] = 1                                             # (as after add(p, 0, 0))
    with pytest.raises(ValueError):
        acc.add(p, 0, 0)                                            # the same block again
    with pytest.raises(ValueError):
        acc.add(p, 0, 2)                                            # model 1 skipped
    with pytest.raises(ValueError):
        acc.add(p, 1, 1)                                            # row 2 has no model 0 yet
    with pytest.raises(ValueError):
        acc.variance()                                              # rows 2, 3 hold nothing
    with pytest.raises(ValueError):
        acc.individual()
    with pytest.raises(ValueError):
        acc.roundrobin_sid()


def test_both_sinks_share_the_batch_check_and_the_scaler_upload():
    """``EnsembleAccumulator`` and ``Evaluator`` refuse the same bad predictions through ``PredictionSink``'s one
    check, before anything would launch, and upload a scaler once per object."""
    from chemprop_amd import Evaluator, TargetTable
    from chemprop_amd.predict import PredictionSink
    acc = EnsembleAccumulator(4, 3, 'cpu')
    ev = Evaluator(TargetTable(np.zeros((4, 3)), 'regression', 'cpu'), ['rmse'])
    for sink in (acc, ev):
        assert isinstance(sink, PredictionSink) and type(sink)._batch is PredictionSink._batch
        assert type(sink)._scale is PredictionSink._scale
        assert (sink.n_rows, sink.width, sink.device) == (4, 3, torch.device('cpu'))
        for bad, word in ((torch.zeros(2, 3, dtype=torch.float64), 'float32'),     # dtype
                          (torch.zeros(3), 'float32'),                             # rank
                          (np.zeros((2, 3), dtype=np.float32), 'float32'),         # no tensor
                          (torch.zeros(2, 4), 'width'),                            # width
                          (torch.zeros(2, 2, 2), 'width')):                        # width, taken flat
            with pytest.raises(ValueError, match=word):
                sink.add(bad, 0, 0)
        for row0 in (-1, 3, 4):                                                    # rows 3 .. 5 of 4
            with pytest.raises(ValueError, match='rows'):
                sink.add(torch.zeros(2, 3), row0, 0)
        view, B = sink._batch(torch.zeros(2, 1, 3), 2)                             # [B][tasks][classes], flat
        assert B == 2 and tuple(view.shape) == (2, 3) and view.is_contiguous()
        scaler = cli.StandardScaler(np.array([1.0, -0.5, 0.25]), np.array([2.0, 0.75, 1.0]))
        means, stds = sink._scale(scaler, 3)
        again = sink._scale(scaler, 3)
        assert len(sink._scales) == 1 and again[0] is means and again[1] is stds
        assert means.dtype == stds.dtype == torch.float64
        assert means.tolist() == [1.0, -0.5, 0.25] and stds.tolist() == [2.0, 0.75, 1.0]
        with pytest.raises(ValueError, match='scaler'):
            sink._scale(cli.StandardScaler(np.zeros(2), np.ones(2)), 3)
        with pytest.raises(ValueError, match='scaler'):
            sink._scale(cli.StandardScaler(np.zeros(3), np.ones(4)), 3)
        assert len(sink._scales) == 1
    with pytest.raises(ValueError, match='scaler'):                                # (through add: before the launch)
        acc.add(torch.zeros(2, 3), 0, 0, cli.StandardScaler(np.zeros(2), np.ones(2)))
    assert not acc._count.any() and not ev._seen.any()                             # nothing was folded
    with pytest.raises(ValueError, match='model index 1'):
        ev.add(torch.zeros(2, 3), 0, 1)                                            # the evaluator takes model 0 alone


BASE_PREDICT = ['--test_path', 't.csv', '--graphs_path', 'g.npz', '--preds_path', 'p.csv']


def test_parse_predict_args():
    a = cli.parse_predict_args(BASE_PREDICT + ['--checkpoint_dir', 'd'])
    assert (a.test_path, a.graphs_path, a.preds_path, a.checkpoint_dir) == ('t.csv', 'g.npz', 'p.csv', 'd')
    assert a.checkpoint_path is None and a.checkpoint_paths is None and a.features_path is None
    assert a.phase_features_path is None and a.batch_size == 50 and a.gpu == 0
    assert not (a.no_features_scaling or a.ensemble_variance or a.individual_ensemble_predictions or
                a.drop_extra_columns)
    assert cli.checkpoint_paths_of(cli.parse_predict_args(BASE_PREDICT + ['--checkpoint_path', 'm.pt'])) == ['m.pt']
    a = cli.parse_predict_args(BASE_PREDICT + ['--checkpoint_paths', 'a.pt', 'b.pt', '--features_path', 'f.csv',
                                               'g.npy', '--phase_features_path', 'ph.csv', '--no_features_scaling',
                                               '--batch_size', '7', '--gpu', '1', '--ensemble_variance',
                                               '--individual_ensemble_predictions', '--drop_extra_columns'])
    assert cli.checkpoint_paths_of(a) == ['a.pt', 'b.pt'] and a.features_path == ['f.csv', 'g.npy']
    assert a.phase_features_path == 'ph.csv' and a.batch_size == 7 and a.gpu == 1
    assert a.no_features_scaling and a.ensemble_variance and a.individual_ensemble_predictions and a.drop_extra_columns
    for bad in ([], ['--checkpoint_dir', 'd', '--checkpoint_path', 'm.pt'],
                ['--checkpoint_path', 'm.pt', '--checkpoint_paths', 'a.pt'], ['--checkpoint_dir', 'd', '--batch_size', '0']):
        with pytest.raises(ValueError):
            cli.parse_predict_args(BASE_PREDICT + bad)
    with pytest.raises(SystemExit):
        cli.parse_predict_args(['--checkpoint_dir', 'd'])


def test_checkpoint_dir_discovery(tmp_path):
    def touch(*parts):
        p = tmp_path.joinpath(*parts)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b'')
        return str(p)
    with pytest.raises(ValueError):
        cli.find_checkpoints(str(tmp_path))
    # a chemprop_train --ensemble_size tree: the best checkpoints alone, sorted by path
    best = [touch(f'model_{k}', 'best_model.pt') for k in (1, 0, 2)]
    for k in range(3):
        touch(f'model_{k}', 'model.pt')
        touch(f'model_{k}', 'train_val_loss_log.csv')
    assert cli.find_checkpoints(str(tmp_path)) == sorted(best)
    # a directory of other checkpoints: every .pt
    other = tmp_path / 'other'
    files = [touch('other', 'b.pt'), touch('other', 'a.pt'), touch('other', 'fold_0', 'model.pt')]
    touch('other', 'notes.txt')
    assert cli.find_checkpoints(str(other)) == sorted(files)


def _read(path):
    with open(path) as f:
        return list(csv.reader(f))


def test_write_predictions_regression(tmp_path):
    header, rows = ['smiles', 'y', 'note'], [['C', '1.5', 'a'], ['CC', '', 'b']]
    mean = np.array([[0.25, 2.0], [0.5, -1.0]])
    ind = np.stack([mean + 1, mean - 1, mean])
    var = np.var(ind, axis=0)
    path = str(tmp_path / 'sub' / 'p.csv')
    assert cli.write_predictions(path, header, rows, ['t0', 't1'], mean) == ['smiles', 'y', 'note', 't0', 't1']
    got = _read(path)
    assert got[0] == ['smiles', 'y', 'note', 't0', 't1'] and got[1] == ['C', '1.5', 'a', '0.25', '2.0']
    assert got[2] == ['CC', '', 'b', '0.5', '-1.0']
    cli.write_predictions(path, header, rows, ['t0', 't1'], mean, spread=var, individual=ind)
    got = _read(path)
    assert got[0] == ['smiles', 'y', 'note', 't0', 't1', 't0_model_0', 't0_model_1', 't0_model_2', 't1_model_0',
                      't1_model_1', 't1_model_2', 't0_epi_unc', 't1_epi_unc']
    assert [float(v) for v in got[2][3:]] == [0.5, -1.0, 1.5, -0.5, 0.5, 0.0, -2.0, -1.0, var[1, 0], var[1, 1]]
    cli.write_predictions(path, header, rows, ['t0', 't1'], mean, spread=var, drop_extra_columns=True)
    got = _read(path)
    assert got[0] == ['smiles', 't0', 't1', 't0_epi_unc', 't1_epi_unc'] and got[1][0] == 'C' and len(got[1]) == 5
    cli.write_predictions(path, header, rows, ['t0', 't1'], mean, individual=ind[:2], drop_extra_columns=True)
    assert _read(path)[0] == ['smiles', 't0', 't1', 't0_model_0', 't0_model_1', 't1_model_0', 't1_model_1']
    with pytest.raises(ValueError):
        cli.write_predictions(path, header, rows, ['t0'], mean)
    with pytest.raises(ValueError):
        cli.write_predictions(path, header, rows[:1], ['t0', 't1'], mean)


def test_write_predictions_multiclass(tmp_path):
    header, rows = ['smiles', 'a', 'b'], [['C', '0', '2']]
    mean = np.arange(6.0).reshape(1, 6) / 10          # 2 tasks x 3 classes, flat
    ind = np.stack([mean, mean]).reshape(2, 1, 2, 3)  # [M][N][tasks][classes] is taken flat as well
    path = str(tmp_path / 'p.csv')
    cli.write_predictions(path, header, rows, ['a', 'b'], mean, 'multiclass', 3, spread=np.zeros((1, 6)),
                          individual=ind)
    got = _read(path)
    cols = ['a_class_0', 'a_class_1', 'a_class_2', 'b_class_0', 'b_class_1', 'b_class_2']
    assert got[0] == header + cols + [f'{c}_model_{k}' for c in cols for k in range(2)] + [f'{c}_epi_unc' for c in cols]
    assert [float(v) for v in got[1][3:9]] == mean[0].tolist()
    assert [float(v) for v in got[1][9:21]] == [v for v in mean[0].tolist() for _ in range(2)]


def test_write_predictions_spectra_leaves_excluded_cells_empty(tmp_path):
    header, rows = ['smiles', 's0', 's1', 's2'], [['C', '1', '2', '3'], ['CC', '1', '2', '3']]
    mean = np.array([[0.2, 0.3, 0.5], [0.4, 0.6, np.nan]])
    ind = np.stack([mean, mean])
    path = str(tmp_path / 'p.csv')
    names = ['s0', 's1', 's2']
    cli.write_predictions(path, header, rows, names, mean, 'spectra', spread=np.array([0.01, np.nan]), individual=ind,
                          drop_extra_columns=True)
    got = _read(path)
    assert got[0] == ['smiles'] + names + [f'{n}_model_{k}' for n in names for k in range(2)] + ['epi_unc']
    assert got[1] == ['C', '0.2', '0.3', '0.5', '0.2', '0.2', '0.3', '0.3', '0.5', '0.5', '0.01']
    assert got[2] == ['CC', '0.4', '0.6', '', '0.4', '0.4', '0.6', '0.6', '', '', '']
    # prediction columns named like input columns (a training CSV) take their place, as the reference's row dict
    assert cli.write_predictions(path, header, rows, names, mean, 'spectra', spread=np.array([0.01, 0.02])) == \
        header + ['epi_unc']
    assert _read(path)[2] == ['CC', '0.4', '0.6', '', '0.02']


def test_update_prediction_args(tmp_path):
    def ckpt(name, **args):
        path = str(tmp_path / name)
        torch.save({'args': args, 'state_dict': {}}, path)
        return path
    a = ckpt('a.pt', dataset_type='regression', num_tasks=2, task_names=['u', 'v'], polymer=True)
    b = ckpt('b.pt', dataset_type='regression', num_tasks=2)
    info = cli.update_prediction_args([a, b])
    assert info['dataset_type'] == 'regression' and info['task_names'] == ['u', 'v'] and info['polymer'] is True
    assert info['width'] == 2 and info['multiclass_num_classes'] == 1 and info['spectra_phase_mask_path'] is None
    assert cli.update_prediction_args([b])['task_names'] == ['task_0', 'task_1']      # an older checkpoint
    m = ckpt('m.pt', dataset_type='multiclass', num_tasks=2, multiclass_num_classes=4, task_names=['u', 'v'])
    info = cli.update_prediction_args([m])
    assert info['width'] == 8 and info['multiclass_num_classes'] == 4
    s = ckpt('s.pt', dataset_type='spectra', num_tasks=2, spectra_phase_mask_path='mask.csv')
    assert cli.update_prediction_args([s])['spectra_phase_mask_path'] == 'mask.csv'
    for bad in ([a, s], [a, ckpt('c.pt', dataset_type='regression', num_tasks=3)], [a, m], []):
        with pytest.raises(ValueError):
            cli.update_prediction_args(bad)
    torch.save({'state_dict': {}}, str(tmp_path / 'bare.pt'))
    with pytest.raises(ValueError):
        cli.update_prediction_args([str(tmp_path / 'bare.pt')])


def test_ensemble_size_argument_and_train_args_fields():
    base = ['--data_path', 'd.csv', '--graphs_path', 'g.npz', '--save_dir', 'out']
    assert cli.parse_args(base).ensemble_size == 1
    assert cli.parse_args(base + ['--ensemble_size', '3']).ensemble_size == 3
    for bad in ('0', '-2', '33'):
        with pytest.raises(ValueError):
            cli.parse_args(base + ['--ensemble_size', bad])
    t = TrainArgs()
    assert t.ensemble_size == 1 and t.task_names is None
    t = TrainArgs(ensemble_size=3, task_names=['a', 'b'], num_tasks=2, device=torch.device('cpu'))
    plain = {k: cli._plain(v) for k, v in vars(t).items()}
    assert plain['task_names'] == ['a', 'b'] and plain['ensemble_size'] == 3
    fields = set(TrainArgs.__dataclass_fields__)
    again = TrainArgs(**{k: v for k, v in plain.items() if k in fields and k != 'device'}, device=torch.device('cpu'))
    assert again.task_names == ['a', 'b'] and again.ensemble_size == 3
    rows = cli.prediction_rows(np.array([[0.5, np.nan]]), 'spectra')
    assert rows == [[0.5, None]]
    assert cli.prediction_rows(np.arange(6.0).reshape(1, 6), 'multiclass', 3) == [[[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]]
