"""The one loop that walks a split for prediction, and what its sinks share.

``device_predictions`` yields every batch's predictions where the head wrote them: the batches in groups of eight
through ``MPNEncoder.forward_many`` (or the split's cached ``train.frozen_encodings``), ``join_features`` for a
model with input features, the native prediction head; no host sync.  Its callers differ in where a batch goes:
``cli.predict`` copies it to the host, ``ensemble.accumulate_model`` hands it to a ``PredictionSink`` -- the
``EnsembleAccumulator`` of an ensemble, or the ``Evaluator`` of ``evaluate.evaluate``.
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from .features import FeatureTable, join_features


class PredictionSink:
    """What takes the predictions of a data set of ``n_rows`` rows and ``width`` cells per row (tasks, spectrum
    positions, or tasks x classes taken flat) on ``device``, batch by batch: the checks of a batch and the upload
    of a target scaler.  ``_noun`` names the subclass's rows in the messages."""
    _noun = 'sink'

    def __init__(self, n_rows: int, width: int, device):
        self.n_rows, self.width = int(n_rows), int(width)
        self.device = torch.empty(0, device=device).device  # (with its index, as a tensor's device has it)
        self._scales = {}

    def _batch(self, pred: torch.Tensor, row0: int) -> Tuple[torch.Tensor, int]:
        """``pred`` (float32 on the sink's device, ``[B][width]`` or ``[B][tasks][classes]``) for rows ``row0 ..
        row0 + B`` as (a contiguous ``[B][width]`` view, B); ``ValueError`` for anything else."""
        if not torch.is_tensor(pred) or pred.dtype != torch.float32 or pred.device != self.device or pred.dim() < 2:
            raise ValueError(f'{type(self).__name__}.add expects float32 predictions [B][width] on the '
                             f'{self._noun}\'s device')
        pred = pred.detach().reshape(pred.shape[0], -1).contiguous()
        B = int(pred.shape[0])
        if pred.shape[1] != self.width:
            raise ValueError(f'predictions of width {pred.shape[1]} for the {self._noun}\'s width {self.width}')
        if row0 < 0 or row0 + B > self.n_rows:
            raise ValueError(f'rows {row0} .. {row0 + B} outside the {self._noun}\'s {self.n_rows} rows')
        return pred, B

    def _scale(self, scaler, n: int):
        """(means, stds) of ``scaler``, ``n`` of each, as float64 device tensors, uploaded once per scaler."""
        hit = self._scales.get(id(scaler))
        if hit is None:
            means = np.ascontiguousarray(np.asarray(scaler.means, dtype=np.float64).reshape(-1))
            stds = np.ascontiguousarray(np.asarray(scaler.stds, dtype=np.float64).reshape(-1))
            if means.shape != (n,) or stds.shape != (n,):
                raise ValueError(f'a scaler of {means.shape[0]} means and {stds.shape[0]} stds for {n} columns')
            hit = (scaler, torch.from_numpy(means).to(self.device), torch.from_numpy(stds).to(self.device))
            self._scales[id(scaler)] = hit
        return hit[1], hit[2]


def _fallback_predict(model, batch, feats, mask) -> torch.Tensor:
    """A model whose FFN the native prediction heads refuse: its own forward (a spectra model's output
    normalised per row with torch ops, as ``head_predict(normalize=True)`` does it natively)."""
    out = model([batch], feats)
    if getattr(model, 'spectra', False):
        m = torch.ones_like(out, dtype=torch.bool) if mask is None else mask.bool()
        s = torch.where(m, out, torch.zeros_like(out))
        out = torch.where(m, s / s.sum(dim=1, keepdim=True), torch.full_like(out, float('nan')))
    return out


@torch.no_grad()
def device_predictions(model, batches, features: Optional[FeatureTable] = None,
                       row_mask: Optional[torch.Tensor] = None, encodings: Optional[torch.Tensor] = None,
                       own_forward: bool = False, n_rows: Optional[int] = None
                       ) -> Iterator[Tuple[int, torch.Tensor]]:
    """``(row0, predictions)`` of ``model`` for every ``BatchMolGraph`` of ``batches`` (row order = batch order):
    eval mode, ``no_grad``, float32 on the device, no host sync.  ``features``: the model's input features of
    every row, as the model sees them; ``row_mask``: a spectra model's included positions, bool or uint8
    ``[rows][T]`` on the device (ignored for other models): its predictions are normalised per row, the excluded
    positions NaN.  The batches run in groups of up to eight through ``forward_many``, then per batch
    ``join_features`` and the native prediction head; a model whose FFN the native heads refuse runs its own
    forward (``_fallback_predict``).

    ``encodings``: the rows' cached ``train.frozen_encodings``; the head runs straight from them, in the batch
    sizes of ``batches`` (which may then be a plain batch size as well; ``NotImplementedError`` without a native
    head).  ``own_forward``: every batch through ``model([batch], feats)`` and nothing else.  ``n_rows``: the rows
    the caller expects.  Molecules, feature rows and encodings that do not cover the same rows, or features for a
    model that takes none (or the reverse), are a ``ValueError`` before anything is launched."""
    from .train import _predict_head, head_predict  # (here: importing the package does not import the training code)
    model.eval()
    mpn = model.encoder
    if isinstance(batches, int):
        if batches < 1 or encodings is None:
            raise ValueError('a plain batch size must be at least 1 and needs encodings')
        sizes = [min(batches, len(encodings) - s) for s in range(0, len(encodings), batches)]
    else:
        sizes = [len(b.a_scope) for b in batches]
    starts = np.cumsum([0] + sizes).tolist()
    n = starts[-1] if n_rows is None else n_rows
    if starts[-1] != n or (features is not None and len(features) != n) or \
            (encodings is not None and len(encodings) != n):
        raise ValueError(f'{starts[-1]} molecules, {None if features is None else len(features)} feature rows and '
                         f'{None if encodings is None else len(encodings)} encodings for {n} rows')
    needs = bool(getattr(mpn, 'use_input_features', False))
    if needs != (features is not None):
        raise ValueError('the model takes input features and none were given' if needs else
                         'the model takes no input features, but features were given')
    if own_forward and encodings is not None:
        raise ValueError('own_forward runs the encoder: it takes no encodings')
    head = None if own_forward else _predict_head(model)
    if encodings is not None and head is None:
        raise NotImplementedError('predictions from encodings: the model\'s FFN is not one the native heads run')
    findex = features.index(range(n)) if features is not None and n else None
    spectra = bool(getattr(model, 'spectra', False))
    many = encodings is None and head is not None and not mpn.features_only and len(mpn.encoder) == 1 and \
        mpn.atom_descriptors is None
    for g0 in range(0, len(sizes), 8):
        embs = mpn.encoder[0].forward_many(batches[g0:g0 + 8]) if many else [None] * len(sizes[g0:g0 + 8])
        for j, emb in enumerate(embs, g0):
            r0, r1 = starts[j], starts[j + 1]
            feats = None if findex is None else findex[r0:r1]
            mask = None if row_mask is None or not spectra else row_mask[r0:r1]
            if own_forward:
                out = model([batches[j]], feats)
            elif head is None:
                out = _fallback_predict(model, batches[j], feats, mask)
            else:
                if encodings is not None:
                    emb = encodings[r0:r1]
                if emb is None:
                    x = mpn([batches[j]], feats)
                else:
                    x = emb if feats is None else join_features(emb, feats)
                out = head_predict(model, x, head, normalize=True, mask=mask) if spectra else \
                    head_predict(model, x, head)
            yield r0, out
