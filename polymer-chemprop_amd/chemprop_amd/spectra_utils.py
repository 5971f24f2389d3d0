"""Spectra losses, normalisation and metrics (``chemprop/spectra_utils.py``), vectorised and without progress
bars.  The torch losses serve the torch path of the training step (``fused_head=False``) and are the oracle of
the native spectra head (``wdmpnn_head_spectra``); the numpy functions run on the host."""
from __future__ import annotations

import csv
from typing import List, Optional, Sequence

import numpy as np
import torch


def _normalized(preds: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """The model's spectra with the masked-out positions zeroed, every row divided by its sum."""
    s = torch.where(mask, preds, torch.zeros_like(preds))
    return s / s.sum(dim=1, keepdim=True)


def sid_loss(preds: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """spectra_utils.py:9-39 without a threshold (the training call passes none): per position, with p the
    row-normalised masked prediction, ``p log(p / y) + y log(y / p)``; 0 where the mask is False.  ``[B][T]``."""
    one = torch.ones_like(preds)
    p = torch.where(mask, _normalized(preds, mask), one)
    y = torch.where(mask, targets, one)
    return torch.log(p / y) * p + torch.log(y / p) * y


def wasserstein_loss(preds: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """spectra_utils.py:86-114 without a threshold: ``|cumsum(y) - cumsum(p)|`` per position, the cumulative sum
    of the targets over the raw row (missing entries as given: the training step passes 0).  ``[B][T]``."""
    return torch.abs(torch.cumsum(targets, dim=1) - torch.cumsum(_normalized(preds, mask), dim=1))


def _rows(spectra) -> tuple:
    """(values with 0 for None / NaN, present mask) of a list of rows or an array, float64 ``[N][T]``."""
    a = np.array([[np.nan if x is None else x for x in r] for r in spectra], dtype=np.float64) \
        if not isinstance(spectra, np.ndarray) else spectra.astype(np.float64)
    a = a.reshape(len(a), -1)
    present = ~np.isnan(a)
    return np.where(present, a, 0.0), present


def phase_row_mask(phase_features, phase_mask) -> np.ndarray:
    """``(phase_features @ phase_mask) != 0`` (spectra_utils.py:194): the positions each row's phase includes."""
    return np.matmul(np.asarray(phase_features, dtype=np.float64), np.asarray(phase_mask, dtype=np.float64)) != 0


def normalize_spectra(spectra, phase_features=None, phase_mask=None, excluded_sub_value=None,
                      threshold: Optional[float] = None) -> List[List[Optional[float]]]:
    """spectra_utils.py:162-208: values below ``threshold`` raised to it, positions that are missing (None / NaN)
    or excluded by the row's phase (``phase_features @ phase_mask`` == 0) set to 0, every row divided by its sum,
    the excluded positions replaced by ``excluded_sub_value``.  One vectorised pass (the reference works in
    batches of 50 with the same result)."""
    if len(spectra) == 0:
        return []
    a, mask = _rows(spectra)
    if threshold is not None:
        a = np.where(a < threshold, threshold, a)
    if phase_mask is not None and phase_features is not None:
        mask = mask & phase_row_mask(phase_features, phase_mask)
    a = np.where(mask, a, 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        a = a / a.sum(axis=1, keepdims=True)
    out = a.astype(object)
    out[~mask] = excluded_sub_value
    return out.tolist()


def _metric_rows(model_spectra, target_spectra, threshold):
    preds, _ = _rows(model_spectra)
    targets, mask = _rows(target_spectra)
    if threshold is not None:
        preds = np.where(preds < threshold, threshold, preds)
    preds = np.where(mask, preds, 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        preds = preds / preds.sum(axis=1, keepdims=True)
    return preds, targets, mask


def sid_metric(model_spectra, target_spectra, threshold: Optional[float] = None) -> float:
    """spectra_utils.py:42-83: the mean over the rows of ``sum_t p log(p / y) + y log(y / p)`` over the present
    targets (None / NaN = missing), p the row-normalised prediction.  Deviation: the reference ends with
    ``np.mean(loss)`` on its last batch of 50 rows only; this is the documented meaning, the mean over ALL rows
    (equal whenever there are at most 50 rows)."""
    p, y, mask = _metric_rows(model_spectra, target_spectra, threshold)
    p = np.where(mask, p, 1.0)
    y = np.where(mask, y, 1.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        loss = p * np.log(p / y) + y * np.log(y / p)
    return float(np.mean(loss.sum(axis=1)))


def wasserstein_metric(model_spectra, target_spectra, threshold: Optional[float] = None) -> float:
    """spectra_utils.py:117-159: the mean over the rows of ``sum_t |cumsum(y)_t - cumsum(p)_t|`` (missing targets
    as 0).  The same deviation as ``sid_metric``: the mean runs over all rows, not the reference's last batch."""
    p, y, _ = _metric_rows(model_spectra, target_spectra, threshold)
    return float(np.mean(np.abs(np.cumsum(y, axis=1) - np.cumsum(p, axis=1)).sum(axis=1)))


def load_phase_mask(path: str) -> List[List[int]]:
    """spectra_utils.py:244-261: a CSV with a header row and a label column; every other cell is 0 or 1, one row
    per phase, one column per spectrum position."""
    data = []
    with open(path) as f:
        reader = csv.reader(f)
        next(reader)
        for line in reader:
            if any(x not in ('0', '1') for x in line[1:]):
                raise ValueError('Phase mask must contain only 0s and 1s, with 0s indicating exclusion regions.')
            data.append([int(x) for x in line[1:]])
    return data
