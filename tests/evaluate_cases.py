"""Shared data of tests/test_evaluate_host.py and tests/test_evaluate_gpu.py: hand-made fp32 predictions and
targets for each dataset type, the yardstick (the CLI's own ``evaluate_predictions``, so sklearn, on the same fp32
predictions), a numpy restatement of the partial sums ``wdmpnn_eval_add`` / ``wdmpnn_eval_spectra`` /
``wdmpnn_eval_auc`` form, and the comparison at the issue's tolerance.

Tolerance (derived, not measured): all arithmetic is double; a score sums at most about 1000 terms here with about
five roundings per term, so its error is bounded by about 5 * 1000 * 2^-53 = 5.5e-13; 1e-11 leaves room for ``log``
differing from numpy's by an ulp and for sklearn's trapezoid arithmetic.  Relative for the summed metrics, absolute
for r2 and auc (which can be near 0); accuracy, the NaN pattern and the list lengths are equal exactly."""
import math
import warnings

import numpy as np

from chemprop_amd import cli

TIGHT = 1e-11
PARITY = 1e-5   # the project's bound between two launch paths of one model
ABSOLUTE = ('r2', 'auc')


class Case:
    def __init__(self, dataset_type, preds, targets, metrics, scaler=None, num_classes=1):
        self.dataset_type, self.metrics, self.scaler, self.num_classes = dataset_type, list(metrics), scaler, num_classes
        self.preds = np.ascontiguousarray(preds, dtype=np.float32)      # [N][W]
        self.targets = np.ascontiguousarray(targets, dtype=np.float64)  # [N][T], NaN = missing
        self.n, self.num_tasks = self.targets.shape

    def target_rows(self):
        conv = int if self.dataset_type == 'multiclass' else float
        return [[None if math.isnan(v) else conv(v) for v in r] for r in self.targets.tolist()]

    def values(self):
        """The predictions as the host path sees them: float64 of the fp32 values, inverse-scaled for regression."""
        v = self.preds.astype(np.float64)
        if self.scaler is not None:
            v = self.scaler.inverse_transform(v)
        return v

    def want(self, values=None):
        """The yardstick: ``cli.evaluate_predictions`` (sklearn) on the prediction rows."""
        v = self.values() if values is None else values
        rows = cli.prediction_rows(v, self.dataset_type, self.num_classes)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')  # (sklearn: r2 of one sample; fp32 probabilities that sum to 1 +- 1e-7)
            return cli.evaluate_predictions(rows, self.target_rows(), self.num_tasks, self.metrics, self.dataset_type)


def regression_case():
    """N = 37, T = 3: scattered missing targets, a task without any target, a task with a single one; a scaler
    with distinct means and stds."""
    rng = np.random.default_rng(37)
    n = 37
    preds = rng.standard_normal((n, 3)).astype(np.float32)
    scaler = cli.StandardScaler(np.array([1.5, -2.0, 0.25]), np.array([2.0, 0.5, 3.0]))
    targets = scaler.inverse_transform(preds.astype(np.float64)) + 0.3 * rng.standard_normal((n, 3))
    targets[rng.random(n) < 0.2, 0] = np.nan
    targets[:, 1] = np.nan
    targets[:, 2] = np.nan
    targets[20, 2] = 0.75
    return Case('regression', preds, targets, ['rmse', 'mse', 'mae', 'r2'], scaler)


def classification_case():
    """N = 300 (two AUC row blocks, a ragged second tile), T = 4: fp32 predictions with groups of exact ties and the
    values 0.0, 1.0 (clipping) and 0.5 (the threshold); task 1's targets are all 1, task 2's present predictions all
    0, task 3 has a single positive row."""
    rng = np.random.default_rng(300)
    n = 300
    levels = np.array([0.0, 0.0625, 0.2, 0.3, 0.5, 0.5, 0.7, 0.9, 1.0], dtype=np.float32)
    preds = levels[rng.integers(0, len(levels), (n, 4))]
    loose = rng.random((n, 4)) < 0.3
    preds = np.where(loose, rng.random((n, 4)).astype(np.float32), preds).astype(np.float32)
    targets = (rng.random((n, 4)) < 0.2 + 0.6 * preds).astype(np.float64)
    targets[rng.random((n, 4)) < 0.15] = np.nan
    targets[:, 1] = np.where(np.isnan(targets[:, 1]), np.nan, 1.0)
    preds[~np.isnan(targets[:, 2]), 2] = 0.0
    targets[:, 3] = np.where(np.isnan(targets[:, 3]), np.nan, 0.0)
    targets[257, 3] = 1.0                 # the only positive, in the second row block
    preds[257, 3] = 0.7                   # tied with some negatives
    assert 0.0 in preds[:, 0] and 1.0 in preds[:, 0] and 0.5 in preds[:, 0]
    return Case('classification', preds, targets, ['auc', 'cross_entropy', 'accuracy'])


def multiclass_case():
    """N = 37, two tasks of three classes: class 2 never occurs in task 1's targets, row 5 has two equal maxima,
    row 6 a probability of exactly 0 at its true class."""
    rng = np.random.default_rng(3)
    n = 37
    logits = rng.standard_normal((n, 2, 3))
    p = np.exp(logits)
    p = (p / p.sum(axis=2, keepdims=True)).astype(np.float32)
    targets = rng.integers(0, 3, (n, 2)).astype(np.float64)
    targets[:, 1] = rng.integers(0, 2, n)
    targets[rng.random((n, 2)) < 0.2] = np.nan
    p[5, 0] = [0.4, 0.4, 0.2]
    targets[5, 0] = 1.0                   # list.index(max) says 0: counted wrong
    p[6, 0] = [0.0, 0.5, 0.5]
    targets[6, 0] = 0.0
    p[7, 1] = [0.25, 0.25, 0.5]
    targets[7, 1] = 0.0
    return Case('multiclass', p.reshape(n, 6), targets, ['cross_entropy', 'accuracy'], num_classes=3)


def spectra_case(n=9, T=70, seed=0):
    """Normalised spectra: rows 0 .. n/3 have their first T/5 positions excluded by their phase (NaN predictions,
    missing targets), targets are missing here and there, and the last row has a single present target."""
    rng = np.random.default_rng(seed + T)
    raw = np.exp(rng.standard_normal((n, T))).astype(np.float64)
    traw = np.exp(rng.standard_normal((n, T)))
    included = np.ones((n, T), dtype=bool)
    included[:max(n // 3, 1), :T // 5] = False
    present = included & (rng.random((n, T)) > 0.1)
    present[n - 1] = False
    present[n - 1, T // 2] = True
    raw = np.where(included, raw, 0.0)
    preds = np.where(included, raw / raw.sum(axis=1, keepdims=True), np.nan).astype(np.float32)
    traw = np.where(present, traw, 0.0)
    targets = np.where(present, traw / traw.sum(axis=1, keepdims=True), np.nan)
    return Case('spectra', preds, targets, ['sid', 'wasserstein'])


# ---------------------------------------------------------------------------------------------------
# the device's sums, restated in numpy (include/wdmpnn.h names the slots)
# ---------------------------------------------------------------------------------------------------
EPS = 2.0 ** -52


def numpy_partials(case):
    """(partials [T][4], auc counts [T][1] or None) as the kernels define them."""
    T, C = case.num_tasks, case.num_classes
    part = np.zeros((T, 4))
    counts = np.zeros((T, 1), dtype=np.int64) if case.dataset_type == 'classification' else None
    v = case.values()
    for t in range(T):
        tg = case.targets[:, t]
        ok = ~np.isnan(tg)
        if case.dataset_type == 'regression':
            e = v[ok, t] - tg[ok]
            part[t, 0], part[t, 1] = (e * e).sum(), np.abs(e).sum()
        elif case.dataset_type == 'classification':
            p, one = v[ok, t], tg[ok] == 1
            part[t, 0] = -np.log(np.clip(np.where(one, p, 1.0 - p), EPS, 1 - EPS)).sum()
            part[t, 1] = ((p > 0.5) == one).sum()
            part[t, 2], part[t, 3] = (p == 0).sum(), (p == 1).sum()
            pos, neg = p[one], p[tg[ok] == 0]
            counts[t, 0] = 2 * (neg[None, :] < pos[:, None]).sum() + (neg[None, :] == pos[:, None]).sum()
        else:
            p = v[ok, t * C:(t + 1) * C]
            cls = tg[ok].astype(int)
            part[t, 0] = -np.log(np.clip(p[np.arange(len(cls)), cls], EPS, 1 - EPS)).sum()
            part[t, 1] = (np.array([list(r).index(max(r)) for r in p.tolist()], dtype=int) == cls).sum()
    return part, counts


def numpy_spectra_rows(case):
    """(sid [N], wasserstein [N]) per row, as wdmpnn_eval_spectra defines them."""
    p = case.preds.astype(np.float64)
    present = ~np.isnan(case.targets)
    z = np.where(present & ~np.isnan(p), p, 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        q = z / z.sum(axis=1, keepdims=True)
        y = np.where(present, case.targets, 0.0)
        terms = np.where(present, q * np.log(q / np.where(present, y, 1.0)) +
                         y * np.log(np.where(present, y, 1.0) / q), 0.0)
    return terms.sum(axis=1), np.abs(np.cumsum(y, axis=1) - np.cumsum(q, axis=1)).sum(axis=1)


def assert_scores_close(got, want, tol=TIGHT, what=''):
    """Same metrics in the same order, lists of the same lengths, the same NaN pattern, accuracy exactly equal,
    r2 / auc within ``tol`` absolute, every other metric within ``tol`` relative; each figure is printed first."""
    assert list(got) == list(want), (what, list(got), list(want))
    for m in want:
        g, w = np.asarray(got[m], dtype=np.float64), np.asarray(want[m], dtype=np.float64)
        assert g.shape == w.shape, (what, m, got[m], want[m])
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, m, got[m], want[m])
        ok = ~np.isnan(w)
        err = np.abs(g - w)[ok]
        if m not in ABSOLUTE:
            err = err / np.where(w[ok] == 0, 1.0, np.abs(w[ok]))  # (a score of exactly 0: absolute)
        print(f'{what} {m}: got {g.tolist()} want {w.tolist()} '
              f'{"abs" if m in ABSOLUTE else "rel"} err {err.max() if err.size else 0.0:.3e} (bound {tol:g})')
        if m == 'accuracy' and tol == TIGHT:
            assert np.array_equal(g[ok], w[ok]), (what, m, got[m], want[m])
        else:
            assert np.all(err <= tol), (what, m, got[m], want[m])
