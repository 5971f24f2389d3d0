"""Latent vectors on the device: ``chemprop_fingerprint`` (train/molecule_fingerprint.py) and the graph embeddings
of ``chemprop_predict --save_graph_embeddings`` (make_predictions.py:156-195).

The reference runs ``MoleculeModel.fingerprint`` batch by batch, copies every batch to the host as a Python list and
fills a numpy ``[N][fp][M]`` array model by model.  Here a model's vectors stay where the kernels wrote them:
``predict.device_predictions(latent=...)`` yields them (the encoder eight batches at a time, ``train.head_latent`` for
``last_FFN``), ``LatentAccumulator.add`` folds a batch into the ensemble's arrays in one ``wdmpnn_latent_add`` launch,
and the result leaves the device once, after the last model.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native
from .ensemble import (_open_model, make_batches, model_atom_descriptors, model_features, model_graphs,
                       set_feature_sizes_of)
from .slots import shares_encoder
from .features import FeatureTable
from .predict import LATENT_TYPES, PredictionSink, device_predictions


class LatentAccumulator(PredictionSink):
    """The latent vectors of an ensemble of ``n_models`` models for a data set of ``n_rows`` rows, ``width`` columns
    each, on ``device``.  ``columns``: hold every model's vectors as float64 ``[n_rows][width][n_models]``, the
    reference's ``all_fingerprints`` (molecule_fingerprint.py:90,117).  ``running_sum``: hold the fp32 running sum of
    the models' vectors in model order (make_predictions.py:163-166).  ``c0``: the first column of a batch that is
    taken; a batch may be wider than ``c0 + width`` (the feature columns behind an encoding are dropped so).  Nothing
    is zeroed: model 0's ``add`` initialises the rows it covers, so every row must get its models in the order 0,
    1, 2, ...; the order is checked on the host (``ValueError``), the kernel trusts it."""
    _noun = 'accumulator'

    def __init__(self, n_rows: int, width: int, device, n_models: int, columns: bool = True,
                 running_sum: bool = False, c0: int = 0):
        if n_rows < 0 or width < 1 or c0 < 0:
            raise ValueError(f'LatentAccumulator: {n_rows} rows of width {width} from column {c0}')
        if not isinstance(n_models, int) or not 1 <= n_models <= _native.ENSEMBLE_MAX_MODELS:
            raise ValueError(f'LatentAccumulator needs n_models in 1 .. {_native.ENSEMBLE_MAX_MODELS} (got {n_models})')
        if not columns and not running_sum:
            raise ValueError('LatentAccumulator holds the columns, the running sum, or both')
        super().__init__(n_rows, width, device)
        self.n_models, self.c0 = n_models, int(c0)
        self._cols = torch.empty((n_rows, width, n_models), dtype=torch.float64, device=self.device) if columns else None
        self._sum = torch.empty((n_rows, width), dtype=torch.float32, device=self.device) if running_sum else None
        self._count = np.zeros(n_rows, dtype=np.int64)  # models folded into each row so far (host bookkeeping)

    def add(self, vectors: torch.Tensor, row0: int, k: int, scaler=None) -> None:
        """Fold model ``k``'s ``vectors`` (float32 on the device, ``[B][ld]`` with ``ld >= c0 + width``) for rows
        ``row0 .. row0 + B`` into the arrays: one launch, no host sync.  (``scaler``: unused; a sink's ``add`` takes
        it.)"""
        if not torch.is_tensor(vectors) or vectors.dtype != torch.float32 or vectors.device != self.device or \
                vectors.dim() != 2:
            raise ValueError('LatentAccumulator.add expects float32 vectors [B][width] on the accumulator\'s device')
        v = vectors.detach().contiguous()
        B, ld = int(v.shape[0]), int(v.shape[1])
        if ld < self.c0 + self.width:
            raise ValueError(f'vectors of width {ld} for the accumulator\'s columns {self.c0} .. {self.c0 + self.width}')
        if row0 < 0 or row0 + B > self.n_rows:
            raise ValueError(f'rows {row0} .. {row0 + B} outside the accumulator\'s {self.n_rows} rows')
        if not 0 <= k < self.n_models:
            raise ValueError(f'model {k} of an ensemble of {self.n_models}')
        seen = self._count[row0:row0 + B]
        if B and not (seen == k).all():
            raise ValueError(f'model {k} for rows {row0} .. {row0 + B}, which hold {int(seen.min())} to '
                             f'{int(seen.max())} models: every row takes its models once each, in order')
        e = _native.WdLatentAdd()
        e.src, e.ld_src, e.B, e.W, e.c0 = v.data_ptr(), ld, B, self.width, self.c0
        e.M, e.k, e.row0 = self.n_models, k, row0
        e.cols, e.sum, e.ld_sum = _native.ptr(self._cols), _native.ptr(self._sum), self.width
        _native.check(_native.lib().wdmpnn_latent_add(ctypes.byref(e), _native.current_stream(self.device)),
                      'latent add')
        self._count[row0:row0 + B] = k + 1

    def _finished(self) -> None:
        if self.n_rows and not (self._count == self.n_models).all():
            raise ValueError(f'the rows hold between {int(self._count.min())} and {int(self._count.max())} of '
                             f'{self.n_models} models: finish every model over every row first')

    def columns(self) -> torch.Tensor:
        """Every model's vectors, float64 ``[n_rows][width][n_models]``."""
        if self._cols is None:
            raise ValueError('LatentAccumulator(columns=True) holds the models\' vectors')
        self._finished()
        return self._cols

    def mean32(self) -> torch.Tensor:
        """``sum / n_models`` as float32: the IEEE quotient of the fp32 running sum and the model count, which is
        numpy's ``float32_array / int`` (make_predictions.py:193).  Divided in double by a device tensor and rounded
        to float32: a float64 quotient of float32 operands rounds to the float32 quotient (53 >= 2 * 24 + 2 bits),
        whereas torch's ``tensor / python_scalar`` multiplies by the rounded reciprocal, which is not that quotient
        for a count that is no power of two."""
        if self._sum is None:
            raise ValueError('LatentAccumulator(running_sum=True) holds the running sum')
        self._finished()
        m = torch.full((), float(self.n_models), dtype=torch.float64, device=self.device)
        return (self._sum.double() / m).float()


def model_fingerprint(model, batches, fingerprint_type: str = 'MPN', features: Optional[FeatureTable] = None,
                      atom_descriptors=None) -> torch.Tensor:
    """``model_fingerprint`` of the reference (molecule_fingerprint.py:151-183) as one float32 device tensor: the
    model's ``fingerprint(..., fingerprint_type)`` of every batch of ``batches`` (``BatchMolGraph`` s; a model of
    several molecules takes lists of them), rows in batch order.  ``MPN``: the FFN's input, ``features`` joined when
    given (they may be left out: the encoders alone run); ``last_FFN``: ``[N][ffn_hidden_size]``.
    ``atom_descriptors``: the rows' ``AtomDescriptorTable`` for a descriptor model."""
    parts = [v for _, v in device_predictions(model, batches, features, latent=fingerprint_type,
                                              atom_descriptors=atom_descriptors)]
    if not parts:
        dev = next(model.parameters()).device
        return torch.empty((0, 0), dtype=torch.float32, device=dev)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def fingerprint_width(model, fingerprint_type: str) -> int:
    """``total_fp_size`` of molecule_fingerprint.py:79-89: ``hidden_size * number_of_molecules`` for ``MPN`` (the
    feature columns are not part of it), ``ffn_hidden_size`` for ``last_FFN``."""
    if fingerprint_type not in LATENT_TYPES:
        raise ValueError(f'Fingerprint type {fingerprint_type} not supported')
    if fingerprint_type == 'MPN':
        if model.encoder.features_only:
            raise ValueError('With features_only models, there is no latent MPN representation. Use last_FFN '
                             'fingerprint type instead.')
        return int(sum(e.hidden_size for e in model.encoder.encoder))
    linears = [m for m in model.ffn if isinstance(m, torch.nn.Linear)]
    if len(linears) < 2:
        from .train import NO_LATENT_LAYER
        raise ValueError(NO_LATENT_LAYER)
    return int(linears[0].out_features)


def molecule_fingerprint(checkpoints_or_models, graphs: Sequence, batch_size: int, fingerprint_type: str = 'MPN',
                         features=None, phase_features=None, features_scaling: bool = True, device=None,
                         atom_descriptors=None, atom_descriptor_scaling: bool = True, atom_features=None,
                         bond_features=None, bond_feature_scaling: bool = True) -> np.ndarray:
    """The fingerprints of ``graphs`` (``MolGraph`` records, one per row) under every model, float64 numpy
    ``[N][fp][M]`` as the reference's ``molecule_fingerprint`` returns them.  ``checkpoints_or_models``: checkpoint
    paths, ``(model, data_scaler, features_scaler)`` tuples or models (a sequence: the array's last axis is its
    length), handled one after the other as ``ensemble.predict_ensemble`` does, each model seeing the raw
    ``features`` through its own features scaler (``features_scaling=False``: as they are) and ``phase_features``
    unscaled.  ``MPN``: fp = ``hidden_size * number_of_molecules``, the feature columns dropped; features are not
    needed, even for a model trained with them (the encoders alone run).  ``last_FFN``: fp = ``ffn_hidden_size``.
    ``atom_descriptors``: one raw ``[n_atoms][d]`` array per row for descriptor models, each model scaling them
    with its own ``atom_descriptor_scaler`` (``ensemble.model_atom_descriptors``).  ``atom_features`` /
    ``bond_features``: the raw extra atom / bond features of models trained with them, appended to the graphs' rows
    through each model's own scalers (``ensemble.model_graphs``).  One host copy, after the last model."""
    device = torch.device('cuda', 0) if device is None else torch.device(device)
    items = list(checkpoints_or_models)
    if not items:
        raise ValueError('molecule_fingerprint: no model given')
    batches = None
    n = len(graphs)
    acc = None
    for k, item in enumerate(items):
        model, _, features_scaler = _open_model(item, device)
        model.eval()
        set_feature_sizes_of(model)
        own = model_graphs(item, model, graphs, atom_features, bond_features, atom_descriptor_scaling,
                           bond_feature_scaling, k)
        if own is not graphs:  # (extra features through this model's scalers: its own batches)
            batches = None
        if batches is None:  # (rows of several molecules: with the merged graphs a shared encoder runs once over)
            batches = make_batches(own, batch_size, shared=shares_encoder(model))
        width = fingerprint_width(model, fingerprint_type)
        if acc is None:
            acc = LatentAccumulator(n, width, device, n_models=len(items))
        elif width != acc.width:
            raise ValueError(f'model {k} has a {fingerprint_type} representation of width {width}; the ensemble\'s '
                             f'first model one of width {acc.width}')
        needs = bool(getattr(model.encoder, 'use_input_features', False))
        table = None
        if fingerprint_type != 'MPN' or (needs and (features is not None or phase_features is not None)):
            rows = model_features(model, features, features_scaler if features_scaling else None, phase_features, k)
            table = None if rows is None else FeatureTable(rows, device)
        desc = model_atom_descriptors(item, model, atom_descriptors, device, atom_descriptor_scaling, k)
        for r0, v in device_predictions(model, batches, table, n_rows=n, latent=fingerprint_type,
                                        atom_descriptors=desc):
            acc.add(v, r0, k)
        del model, table, desc
    if n == 0:
        return np.zeros((0, acc.width, len(items)))
    return acc.columns().cpu().numpy()


def fingerprint_columns(width: int, n_models: int) -> list:
    """The CSV's fingerprint columns (molecule_fingerprint.py:124-132): ``fp_j`` for one model, ``fp_j_model_i``
    with j outer and i inner for several -- the order of a row of ``[N][fp][M]`` taken flat."""
    if n_models == 1:
        return [f'fp_{j}' for j in range(width)]
    return [f'fp_{j}_model_{i}' for j in range(width) for i in range(n_models)]
