"""Scoring a split on the device (evaluate.py:11-110 of the reference: ``evaluate`` / ``evaluate_predictions``).

``cli.predict`` + ``cli.evaluate_predictions`` copy every batch's predictions to the host, turn them into Python
floats and call sklearn once per task and metric.  Here the targets of a split are uploaded once
(``TargetTable``), every batch's fp32 predictions are folded where the head wrote them into float64 partial sums
(``Evaluator.add``: one ``wdmpnn_eval_add`` or ``wdmpnn_eval_spectra`` launch, no host sync), and ``scores()``
copies a few numbers per task back and finishes the metrics on the host in float64.  ``evaluate`` fills an
evaluator through ``ensemble.accumulate_model`` from ``predict.device_predictions``, the package's one prediction
loop, and returns its scores.

The metrics computed from partials: rmse, mse, mae, r2 (regression); auc, cross_entropy, accuracy
(classification); cross_entropy, accuracy (multiclass); sid, wasserstein (spectra).  Any other metric that
``cli.metric_value`` knows is computed by it from one copy of the kept predictions.  The dict ``scores()`` returns
has the structure of ``cli.evaluate_predictions``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native
from .features import FeatureTable
from .predict import PredictionSink

DEVICE_METRICS = {'regression': ('rmse', 'mse', 'mae', 'r2'),
                  'classification': ('auc', 'cross_entropy', 'accuracy'),
                  'multiclass': ('cross_entropy', 'accuracy'),
                  'spectra': ('sid', 'wasserstein')}
_NAN = float('nan')


def _target_array(targets, num_tasks: Optional[int]) -> np.ndarray:
    """``targets`` (rows of floats with None = missing, or a float array with NaN = missing) as float64 ``[N][T]``."""
    if isinstance(targets, np.ndarray) and targets.dtype.kind == 'f':
        a = np.array(targets, dtype=np.float64)
    else:
        a = np.array([[np.nan if x is None else x for x in r] for r in targets], dtype=np.float64)
    if a.size == 0 and a.ndim < 2:
        a = a.reshape(0, 0 if num_tasks is None else num_tasks)
    if a.ndim != 2:
        raise ValueError(f'targets of shape {a.shape}: one row per molecule, one column per task')
    if num_tasks is not None and a.shape[1] != num_tasks:
        raise ValueError(f'targets of {a.shape[1]} columns for {num_tasks} tasks')
    return np.ascontiguousarray(a)


class TargetTable:
    """The targets of one split, resident on ``device`` as float64 ``[N][T]`` with NaN for a missing target (one
    upload), and everything a metric needs that depends on the targets alone, precomputed in numpy float64:

    ``counts`` ``[T]``: the present targets of every task; ``means`` and ``ss_tot`` ``[T]``: their mean and
    ``sum (t - mean)^2`` (r2's denominator, as sklearn forms it); ``n_pos`` / ``n_neg`` ``[T]``: the targets equal
    to 1 / to 0, and ``all_zero`` / ``all_one``: whether a task's present targets are all 0 / all 1 (true for a task
    without targets, as ``all`` of nothing is).

    ``targets``: rows of floats with None = missing, or a float array with NaN = missing.  ``multiclass``: every
    present target must be an integer class index in ``[0, num_classes)`` (``ValueError`` naming the first offender,
    as ``train.check_class_targets``); ``classification``: 0 or 1.  ``num_tasks`` gives the width of an empty
    split."""

    def __init__(self, targets, dataset_type: str, device, num_classes: int = 0, num_tasks: Optional[int] = None):
        if dataset_type not in DEVICE_METRICS:
            raise ValueError(f'dataset type "{dataset_type}" (one of {", ".join(DEVICE_METRICS)})')
        a = _target_array(targets, num_tasks)
        present = ~np.isnan(a)
        self.dataset_type, self.device = dataset_type, torch.device(device)
        self.n_rows, self.num_tasks = int(a.shape[0]), int(a.shape[1])
        self.num_classes = int(num_classes) if dataset_type == 'multiclass' else 1
        if dataset_type == 'multiclass':
            from .train import _check_class_indices
            if self.num_classes < 2:
                raise ValueError('a multiclass target table needs num_classes >= 2')
            _check_class_indices(np.where(present, a, 0.0), present.astype(np.float64), self.num_classes)
        elif dataset_type == 'classification':
            bad = present & (a != 0) & (a != 1)
            if bad.any():
                r, t = (int(v) for v in np.argwhere(bad)[0])
                raise ValueError(f'classification target {float(a[r, t])!r} in row {r}, task {t} is neither 0 nor 1')
        T = self.num_tasks
        self.host, self.present = a, present
        self.counts = present.sum(axis=0).astype(np.int64)
        self.means, self.ss_tot = np.full(T, np.nan), np.full(T, np.nan)
        for t in range(T):  # per task over the present rows, with sklearn's own operations (r2_score)
            vt = a[present[:, t], t]
            if len(vt):
                self.means[t] = np.average(vt, axis=0)
                self.ss_tot[t] = ((vt - self.means[t]) ** 2).sum(axis=0, dtype=np.float64)
        self.n_pos = (present & (a == 1)).sum(axis=0).astype(np.int64)
        self.n_neg = (present & (a == 0)).sum(axis=0).astype(np.int64)
        self.all_zero = self.n_neg == self.counts
        self.all_one = self.n_pos == self.counts
        self.data = torch.from_numpy(a).to(self.device)

    def __len__(self) -> int:
        return self.n_rows

    def rows(self) -> List[List[Optional[float]]]:
        """The targets as ``cli.evaluate_predictions`` takes them: lists with None = missing (multiclass: ints)."""
        conv = int if self.dataset_type == 'multiclass' else float
        return [[None if math.isnan(v) else conv(v) for v in r] for r in self.host.tolist()]


def finish_scores(table: TargetTable, metrics: Sequence[str], partials=None, sid=None, wasserstein=None,
                  auc_counts=None) -> Dict[str, list]:
    """The metrics of ``DEVICE_METRICS`` from the device's partial sums, on the host in float64, in the structure
    of ``cli.evaluate_predictions``.  ``partials`` ``[T][4]`` (``wdmpnn.h`` names the slots), ``sid`` /
    ``wasserstein`` ``[N]`` per-row terms, ``auc_counts`` ``[T][blocks]`` integers.  A regression or multiclass
    task without targets is skipped; a classification task whose targets or present predictions are all 0 or all 1
    gives NaN for every metric; an empty split gives NaNs."""
    kind, T, n_rows = table.dataset_type, table.num_tasks, table.n_rows
    for m in metrics:
        if m not in DEVICE_METRICS[kind]:
            raise ValueError(f'Metric "{m}" is not computed from partial sums for dataset type "{kind}".')
    if kind == 'spectra':
        rows = {'sid': sid, 'wasserstein': wasserstein}
        return {m: [float(np.mean(np.asarray(rows[m], dtype=np.float64))) if n_rows else _NAN] for m in metrics}
    if n_rows == 0:
        return {m: [_NAN] * T for m in metrics}
    part = np.asarray(partials, dtype=np.float64).reshape(T, _native.EVAL_SLOTS)
    out = {m: [] for m in metrics}
    for t in range(T):
        n = int(table.counts[t])
        if kind == 'classification':
            if table.all_zero[t] or table.all_one[t] or part[t, 2] == n or part[t, 3] == n:
                for m in metrics:
                    out[m].append(_NAN)
                continue
        if n == 0:
            continue
        for m in metrics:
            if m == 'mse':
                v = part[t, 0] / n
            elif m == 'rmse':
                v = math.sqrt(part[t, 0] / n)
            elif m == 'mae':
                v = part[t, 1] / n
            elif m == 'r2':  # sklearn's r2_score: undefined below two samples; a constant target gives 1 or 0
                if n < 2:
                    v = _NAN
                elif table.ss_tot[t] == 0:
                    v = 1.0 if part[t, 0] == 0 else 0.0
                else:
                    v = 1.0 - part[t, 0] / table.ss_tot[t]
            elif m == 'cross_entropy':
                v = part[t, 0] / n
            elif m == 'accuracy':
                v = part[t, 1] / n
            else:  # auc: every (positive, negative) pair counts 2 when ordered, 1 when tied
                total = int(np.asarray(auc_counts, dtype=np.int64).reshape(T, -1)[t].sum())
                v = total / (2.0 * float(table.n_pos[t]) * float(table.n_neg[t]))
            out[m].append(float(v))
    return out


class Evaluator(PredictionSink):
    """Running scores of one split's predictions against its ``TargetTable``.

    ``add(pred, row0)`` folds a batch (float32 on the table's device, ``[B][tasks]``, ``[B][tasks][classes]`` or
    ``[B][T]`` spectra positions) for rows ``row0 .. row0 + B``: one launch, no host sync; as a ``PredictionSink``
    it has ``EnsembleAccumulator.add``'s ``(pred, row0, k, scaler)``, of which it takes model 0 alone.  ``scaler``:
    the regression targets' scaler (``means`` / ``stds``), applied to the predictions in double as
    ``scaler.inverse_transform`` does.  ``keep``: also hold the (inverse-scaled) predictions, ``[N][W]`` float64
    for regression and float32 (exactly what the head wrote) otherwise; AUC and the metrics outside
    ``DEVICE_METRICS`` read them, so they switch it on themselves.  Every row is added once.  ``scores()``: one
    small device-to-host copy, then ``finish_scores``."""
    _noun = 'split'

    def __init__(self, table: TargetTable, metrics: Sequence[str], dataset_type: Optional[str] = None, scaler=None,
                 keep: bool = False):
        dataset_type = table.dataset_type if dataset_type is None else dataset_type
        if dataset_type != table.dataset_type:
            raise ValueError(f'an evaluator for "{dataset_type}" on a "{table.dataset_type}" target table')
        if scaler is not None and dataset_type != 'regression':
            raise ValueError('a target scaler belongs to regression')
        super().__init__(table.n_rows, table.num_tasks * table.num_classes, table.device)
        self.table, self.metrics, self.dataset_type, self.scaler = table, list(metrics), dataset_type, scaler
        self._native_metrics = [m for m in self.metrics if m in DEVICE_METRICS[dataset_type]]
        self._host_metrics = [m for m in self.metrics if m not in DEVICE_METRICS[dataset_type]]
        self._auc = dataset_type == 'classification' and 'auc' in self.metrics
        keep = bool(keep or self._auc or self._host_metrics)
        self._keep_f32 = dataset_type != 'regression'
        self._kept = torch.empty((self.n_rows, self.width), device=self.device,
                                 dtype=torch.float32 if self._keep_f32 else torch.float64) if keep else None
        # one buffer for everything scores() copies back: the partials, the row terms, the AUC integers
        T, N = table.num_tasks, self.n_rows
        spectra = dataset_type == 'spectra'
        self._blocks = (N + 255) // 256
        n_part = 0 if spectra else T * _native.EVAL_SLOTS
        n_sid = N if spectra and 'sid' in self.metrics else 0
        n_wass = N if spectra and ('wasserstein' in self.metrics or not n_sid) else 0
        n_auc = T * self._blocks if self._auc else 0
        self._small = torch.zeros(n_part + n_sid + n_wass + n_auc, dtype=torch.float64, device=self.device)
        cuts = np.cumsum([0, n_part, n_sid, n_wass, n_auc]).tolist()
        self._cuts = cuts
        self._partials, self._sid, self._wass, auc = (self._small[cuts[i]:cuts[i + 1]] for i in range(4))
        self._sid = self._sid if n_sid else None
        self._wass = self._wass if n_wass else None
        self._auc_counts = auc.view(torch.int64) if n_auc else None
        self._seen = np.zeros(N, dtype=bool)  # (host bookkeeping: every row is added once)

    def add(self, pred: torch.Tensor, row0: int, k: int = 0, scaler=None) -> None:
        pred, B = self._batch(pred, row0)
        if k != 0:
            raise ValueError(f'Evaluator.add scores one model\'s predictions (got model index {k})')
        if self._seen[row0:row0 + B].any():
            raise ValueError(f'rows {row0} .. {row0 + B} hold predictions already: every row is added once')
        scaler = self.scaler if scaler is None else scaler
        if scaler is not None and self.dataset_type != 'regression':
            raise ValueError('a target scaler belongs to regression')
        table = self.table
        stream = _native.current_stream(self.device)
        if self.dataset_type == 'spectra':
            e = _native.WdEvalSpectra()
            e.pred, e.ld_pred, e.B, e.T, e.ld_targets = pred.data_ptr(), self.width, B, self.width, table.num_tasks
            e.row0, e.N, e.targets = row0, self.n_rows, table.data.data_ptr()
            e.sid, e.wasserstein = _native.ptr(self._sid), _native.ptr(self._wass)
            e.keep, e.ld_keep, e.keep_f32 = _native.ptr(self._kept), self.width, int(self._keep_f32)
            _native.check(_native.lib().wdmpnn_eval_spectra(ctypes.byref(e), stream), 'eval spectra')
        else:
            e = _native.WdEvalAdd()
            e.pred, e.ld_pred, e.B, e.tasks, e.classes = pred.data_ptr(), self.width, B, table.num_tasks, \
                table.num_classes
            e.kind, e.ld_targets = _native.EVAL_KINDS[self.dataset_type], table.num_tasks
            e.row0, e.N, e.targets = row0, self.n_rows, table.data.data_ptr()
            if scaler is not None:
                means, stds = self._scale(scaler, table.num_tasks)
                e.scale_mean, e.scale_std = means.data_ptr(), stds.data_ptr()
            e.partials = self._partials.data_ptr()
            e.keep, e.ld_keep, e.keep_f32 = _native.ptr(self._kept), self.width, int(self._keep_f32)
            _native.check(_native.lib().wdmpnn_eval_add(ctypes.byref(e), stream), 'eval add')
        self._seen[row0:row0 + B] = True

    def predictions(self) -> torch.Tensor:
        """The kept (inverse-scaled) predictions ``[N][W]`` on the device: float64 for regression, else float32."""
        if self._kept is None:
            raise ValueError('Evaluator(keep=True) holds the predictions')
        self._complete()
        return self._kept

    def _complete(self) -> None:
        if not self._seen.all():
            raise ValueError(f'{int((~self._seen).sum())} of the split\'s {self.n_rows} rows hold no predictions yet')

    def scores(self) -> Dict[str, list]:
        self._complete()
        table = self.table
        if self._auc and self.n_rows:
            a = _native.WdEvalAuc()
            a.preds, a.targets, a.N = self._kept.data_ptr(), table.data.data_ptr(), self.n_rows
            a.tasks, a.ld_preds, a.ld_targets, a.preds_f32 = table.num_tasks, self.width, table.num_tasks, \
                int(self._keep_f32)
            a.counts = self._auc_counts.data_ptr()
            _native.check(_native.lib().wdmpnn_eval_auc(ctypes.byref(a), _native.current_stream(self.device)),
                          'eval auc')
        small = self._small.cpu().numpy() if self._small.numel() else np.zeros(0)
        c = self._cuts
        done = finish_scores(table, self._native_metrics, small[c[0]:c[1]],
                             small[c[1]:c[2]] if self._sid is not None else None,
                             small[c[2]:c[3]] if self._wass is not None else None,
                             small[c[3]:c[4]].view(np.int64) if self._auc_counts is not None else None)
        if self._host_metrics:  # a metric outside DEVICE_METRICS: cli.metric_value on one copy of the predictions
            from . import cli
            rows = cli.prediction_rows(self._kept.cpu().numpy(), self.dataset_type, table.num_classes)
            done.update(cli.evaluate_predictions(rows, table.rows(), table.num_tasks, self._host_metrics,
                                                 self.dataset_type))
        return {m: done[m] for m in self.metrics}


def evaluate(model, batches, table: TargetTable, metrics: Sequence[str], scaler=None,
             features: Optional[FeatureTable] = None, row_mask: Optional[torch.Tensor] = None,
             encodings: Optional[torch.Tensor] = None, evaluator: Optional[Evaluator] = None,
             atom_descriptors=None) -> Dict[str, list]:
    """The scores of ``model`` on one split: its ``BatchMolGraph`` s ``batches`` (row order = batch order), the split's
    ``features`` table, a spectra model's ``row_mask`` and the split's cached ``encodings`` (``batches`` may then be
    a plain batch size) go through ``ensemble.accumulate_model`` into an ``Evaluator``, as
    ``predict.device_predictions`` describes them; no host sync before ``scores()``.  ``evaluator``: fill this one
    (made by the caller, say with ``keep=True`` to read ``predictions()`` afterwards) instead of a fresh one.
    ``atom_descriptors``: the split's ``AtomDescriptorTable`` for a descriptor model."""
    from .ensemble import accumulate_model
    ev = Evaluator(table, metrics, table.dataset_type, scaler) if evaluator is None else evaluator
    if ev.table is not table:
        raise ValueError('evaluate: the evaluator given scores another target table')
    if table.n_rows:
        accumulate_model(ev, 0, model, batches, scaler, features, row_mask, encodings,
                         atom_descriptors=atom_descriptors)
    return ev.scores()
