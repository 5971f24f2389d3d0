"""Ensembles on the device (make_predictions.py:129-201): the mean, the variance and the individual predictions
of M models, and the pairwise SID of an ensemble of spectra (``roundrobin_sid``, spectra_utils.py:211-241).

The reference sums each model's fp32 predictions into a numpy float64 array on the host, one copy per batch
and model.  Here a model's predictions stay where the head wrote them: ``EnsembleAccumulator.add`` folds a
batch into float64 running statistics in one ``wdmpnn_ensemble_add`` launch (Welford's update, with the model's
own inverse target scaling applied in double as ``scaler.py`` does), and the results leave the device once,
after the last model.  ``predict_ensemble`` is the loop over the models; ``accumulate_model`` hands one model's
batches from ``predict.device_predictions``, the package's one prediction loop, to the accumulator.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native
from .features import FeatureTable
from .featurization import BatchMolGraph
from .predict import PredictionSink, _fallback_predict, device_predictions  # noqa: F401 (_fallback_predict: as before)
from .spectra_utils import phase_row_mask


class EnsembleAccumulator(PredictionSink):
    """Float64 running statistics of an ensemble's predictions for a data set of ``n_rows`` rows and ``width``
    cells per row (tasks, spectrum positions, or tasks x classes taken flat), on ``device``.

    ``variance``: also hold Welford's m2.  ``keep``: also hold every model's own predictions, one ``[n_rows][width]``
    slab per model (``n_models`` slabs: the count is then needed up front); ``individual`` and ``roundrobin_sid``
    read them.  Nothing is zeroed: model 0's ``add`` initialises the rows it covers, so every row must get its
    models in the order 0, 1, 2, ...; the order is checked on the host (``ValueError``), the kernel trusts it."""
    _noun = 'accumulator'

    def __init__(self, n_rows: int, width: int, device, variance: bool = False, keep: bool = False,
                 n_models: Optional[int] = None):
        if n_rows < 0 or width < 1:
            raise ValueError(f'EnsembleAccumulator: {n_rows} rows of width {width}')
        if keep and (n_models is None or not 1 <= n_models <= _native.ENSEMBLE_MAX_MODELS):
            raise ValueError(f'EnsembleAccumulator(keep=True) needs n_models in 1 .. {_native.ENSEMBLE_MAX_MODELS} '
                             f'(got {n_models})')
        super().__init__(n_rows, width, device)
        self.n_models = n_models

        def buf(*shape):
            return torch.empty(shape, dtype=torch.float64, device=self.device)
        self._mean = buf(n_rows, width)
        self._m2 = buf(n_rows, width) if variance else None
        self._slabs = buf(n_models, n_rows, width) if keep else None
        self._count = np.zeros(n_rows, dtype=np.int64)  # models folded into each row so far (host bookkeeping)

    def add(self, pred: torch.Tensor, row0: int, k: int, scaler=None) -> None:
        """Fold model ``k``'s predictions ``pred`` (float32 on the device, ``[B][width]`` or ``[B][tasks][classes]``)
        for rows ``row0 .. row0 + B`` into the statistics: one launch, no host sync.  ``scaler``: the model's
        target scaler (``means`` / ``stds`` of length ``width``); the predictions are inverse-scaled in double."""
        pred, B = self._batch(pred, row0)
        if not 0 <= k < _native.ENSEMBLE_MAX_MODELS or (self._slabs is not None and k >= self.n_models):
            raise ValueError(f'model {k} of an ensemble of at most '
                             f'{self.n_models if self._slabs is not None else _native.ENSEMBLE_MAX_MODELS}')
        seen = self._count[row0:row0 + B]
        if B and not (seen == k).all():
            raise ValueError(f'model {k} for rows {row0} .. {row0 + B}, which hold {int(seen.min())} to '
                             f'{int(seen.max())} models: every row takes its models once each, in order')
        e = _native.WdEnsembleAdd()
        e.pred, e.ld_pred, e.B, e.W, e.k, e.row0 = pred.data_ptr(), self.width, B, self.width, k, row0
        if scaler is not None:
            means, stds = self._scale(scaler, self.width)
            e.scale_mean, e.scale_std = means.data_ptr(), stds.data_ptr()
        e.mean, e.m2, e.ld_acc = self._mean.data_ptr(), _native.ptr(self._m2), self.width
        e.keep = self._slabs[k].data_ptr() if self._slabs is not None else None
        _native.check(_native.lib().wdmpnn_ensemble_add(ctypes.byref(e), _native.current_stream(self.device)),
                      'ensemble add')
        self._count[row0:row0 + B] = k + 1

    def models(self) -> int:
        """The number of models every row holds (``ValueError`` while the rows differ or hold none)."""
        if self.n_rows == 0:
            return int(self.n_models or 0)
        lo, hi = int(self._count.min()), int(self._count.max())
        if lo != hi or lo < 1:
            raise ValueError(f'the rows hold between {lo} and {hi} models: finish every model over every row first')
        return lo

    def mean(self) -> torch.Tensor:
        self.models()
        return self._mean

    def variance(self) -> torch.Tensor:
        """``m2 / M``: the population variance, as ``np.var`` over the models."""
        if self._m2 is None:
            raise ValueError('EnsembleAccumulator(variance=True) holds the variance')
        return self._m2 / max(self.models(), 1)

    def individual(self) -> torch.Tensor:
        """Every model's own predictions, ``[M][n_rows][width]``."""
        if self._slabs is None:
            raise ValueError('EnsembleAccumulator(keep=True) holds the individual predictions')
        return self._slabs[:self.models()] if self.n_rows else self._slabs

    def roundrobin_sid(self, threshold: Optional[float] = None) -> torch.Tensor:
        """The pairwise SID of the kept spectra per row (``wdmpnn_ensemble_sid``), float64 ``[n_rows]``; NaN for
        an ensemble of one model."""
        if self._slabs is None:
            raise ValueError('EnsembleAccumulator(keep=True) holds the spectra the pairwise SID compares')
        M = self.models()
        out = torch.empty(self.n_rows, dtype=torch.float64, device=self.device)
        if self.n_rows == 0:
            return out
        s = _native.WdEnsembleSid()
        s.preds, s.model_stride, s.ld = self._slabs.data_ptr(), self.n_rows * self.width, self.width
        s.M, s.N, s.T = M, self.n_rows, self.width
        s.threshold, s.out = 0.0 if threshold is None else float(threshold), out.data_ptr()
        _native.check(_native.lib().wdmpnn_ensemble_sid(ctypes.byref(s), _native.current_stream(self.device)),
                      'ensemble sid')
        return out


def set_feature_sizes_of(model) -> None:
    """``set_extra_atom_fdim`` / ``set_extra_bond_fdim`` as the model was built (a batch without bonds takes its
    bond row width from them)."""
    from .featurization import set_extra_atom_fdim, set_extra_bond_fdim
    set_extra_atom_fdim(int(getattr(model.encoder, 'atom_features_size', 0) or 0))
    set_extra_bond_fdim(int(getattr(model.encoder, 'bond_features_size', 0) or 0))


def make_batches(graphs: Sequence, batch_size: int, shared: bool = False) -> list:
    """The data set as ``BatchMolGraph`` s of ``batch_size`` molecules, in order.  Rows given as tuples or lists of
    N ``MolGraph`` s (a model of N molecules per input) become ``slots.SlotBatch`` es, with their merged graph
    when ``shared`` (a model with ``mpn_shared``)."""
    if batch_size < 1:
        raise ValueError('batch_size must be at least 1')
    if len(graphs) and isinstance(graphs[0], (tuple, list)):
        from .slots import SlotBatch
        n = len(graphs[0])
        if any(not isinstance(r, (tuple, list)) or len(r) != n for r in graphs):
            raise ValueError(f'make_batches: every row needs {n} molecules, as the first has')
        return [SlotBatch([[r[k] for r in graphs[s:s + batch_size]] for k in range(n)], shared=shared)
                for s in range(0, len(graphs), batch_size)]
    return [BatchMolGraph(list(graphs[s:s + batch_size])) for s in range(0, len(graphs), batch_size)]


def accumulate_model(acc: PredictionSink, k: int, model, batches, scaler=None, table: Optional[FeatureTable] = None,
                     row_mask: Optional[torch.Tensor] = None, encodings: Optional[torch.Tensor] = None,
                     embeddings: Optional[PredictionSink] = None, atom_descriptors=None) -> None:
    """Model ``k``'s predictions of ``batches`` into ``acc``, an ``EnsembleAccumulator`` or an ``Evaluator``: every
    batch of ``predict.device_predictions`` (which explains the other arguments) through ``acc.add``.
    ``embeddings``: a ``fingerprint.LatentAccumulator`` that takes, in the same pass, the FFN input of every batch
    (``with_encodings``).  ``atom_descriptors``: the rows' ``AtomDescriptorTable`` for a descriptor model.  No host
    sync."""
    if embeddings is None:
        for r0, out in device_predictions(model, batches, table, row_mask, encodings, n_rows=acc.n_rows,
                                          atom_descriptors=atom_descriptors):
            acc.add(out, r0, k, scaler)
        return
    for r0, out, x in device_predictions(model, batches, table, row_mask, encodings, n_rows=acc.n_rows,
                                         with_encodings=True, atom_descriptors=atom_descriptors):
        acc.add(out, r0, k, scaler)
        embeddings.add(x, r0, k)


def _open_model(item, device):
    """(model, data scaler, features scaler) of an ensemble member: a checkpoint path, a
    ``(model, data_scaler, features_scaler)`` tuple, or a model alone (no scalers)."""
    from . import cli
    if isinstance(item, (str, bytes)) or hasattr(item, '__fspath__'):
        path = str(item)
        scalers = cli.load_scalers(path)
        return cli.load_checkpoint(path, device), scalers[0], scalers[1]
    if isinstance(item, (tuple, list)):
        model, data_scaler, features_scaler = item[:3]  # (a fourth entry: the atom descriptor scaler)
        return model, data_scaler, features_scaler
    return item, None, None


def model_atom_descriptors(item, model, atom_descriptors, device, scaling: bool = True, k: int = 0):
    """The ``AtomDescriptorTable`` of the rows as model ``k`` sees them (make_predictions.py:143-153): the raw
    per-molecule arrays ``atom_descriptors`` through that model's own ``atom_descriptor_scaler`` -- the one stored in
    its checkpoint when ``item`` is a path, ``item[3]`` of a ``(model, data scaler, features scaler, atom descriptor
    scaler)`` tuple, none for a model alone or with ``scaling=False``.  NaN becomes 0 (data.py:133-135).
    ``ValueError`` when the model needs descriptors and gets none, gets descriptors it does not take, or another
    width than it was trained on."""
    from .atom_descriptors import AtomDescriptorTable
    needs = getattr(model.encoder, 'atom_descriptors', None) == 'descriptor'
    if atom_descriptors is None:
        if needs:
            raise ValueError(f'model {k} was trained with atom descriptors: give --atom_descriptors_path to predict')
        return None
    if not needs:
        raise ValueError(f'model {k} was trained without atom descriptors, but atom descriptors were given')
    scaler = None
    if scaling:
        if isinstance(item, (str, bytes)) or hasattr(item, '__fspath__'):
            from . import cli
            scaler = cli.load_scalers(str(item))[2]
        elif isinstance(item, (tuple, list)) and len(item) > 3:
            scaler = item[3]
    arrays = [np.where(np.isnan(a), 0.0, a) for a in (np.asarray(a, dtype=np.float64) for a in atom_descriptors)]
    width = model.encoder.encoder[0].atom_descriptors_size
    if arrays and arrays[0].ndim == 2 and arrays[0].shape[1] != width:
        raise ValueError(f'model {k} was trained with {width} descriptors per atom and {arrays[0].shape[1]} were given')
    return AtomDescriptorTable(arrays, device, scaler)


def model_graphs(item, model, graphs, atom_features=None, bond_features=None, atom_scaling: bool = True,
                 bond_scaling: bool = True, k: int = 0):
    """The rows' graphs as model ``k`` sees them (make_predictions.py:143-153): the raw extra atom features
    (``[n_atoms][da]`` per row) and extra bond features (``[n_bonds / 2][db]`` per row) through that model's own
    ``atom_descriptor_scaler`` / ``bond_feature_scaler`` (found as ``model_atom_descriptors`` finds its scaler:
    the checkpoint at ``item``, or ``item[3]`` / ``item[4]`` of a tuple), appended to the graphs' rows
    (``featurization.widen_mol_graph``).  ``graphs`` itself for a model trained without either.  ``ValueError`` when
    the model needs features and gets none, gets features it does not take, or another width than it was trained
    on."""
    from .featurization import widen_mol_graph
    mpn = model.encoder
    sizes = (int(getattr(mpn, 'atom_features_size', 0) or 0), int(getattr(mpn, 'bond_features_size', 0) or 0))
    given = (atom_features, bond_features)
    names = (('extra atom features', '--atom_descriptors_path'), ('extra bond features', '--bond_features_path'))
    for size, x, (what, flag) in zip(sizes, given, names):
        if size and x is None:
            raise ValueError(f'model {k} was trained with {what}: give {flag} to predict')
        if not size and x is not None:
            raise ValueError(f'model {k} was trained without {what}, but they were given')
    if not any(sizes):
        return graphs
    scalers = [None, None]
    if isinstance(item, (str, bytes)) or hasattr(item, '__fspath__'):
        from . import cli
        scalers = list(cli.load_scalers(str(item))[2:4])
    elif isinstance(item, (tuple, list)):
        scalers = [item[3] if len(item) > 3 else None, item[4] if len(item) > 4 else None]
    out = []
    for size, x, scaler, scaling, (what, _) in zip(sizes, given, scalers, (atom_scaling, bond_scaling), names):
        if x is None:
            out.append(None)
            continue
        arrays = [np.where(np.isnan(a), 0.0, a) for a in (np.asarray(a, dtype=np.float64) for a in x)]
        if arrays and arrays[0].ndim == 2 and arrays[0].shape[1] != size:
            raise ValueError(f'model {k} was trained with {size} {what} per row and {arrays[0].shape[1]} were given')
        out.append([scaler.transform(a) for a in arrays] if scaler is not None and scaling else arrays)
    return [widen_mol_graph(g, None if out[0] is None else out[0][i], None if out[1] is None else out[1][i])
            for i, g in enumerate(graphs)]


def model_features(model, features, features_scaler, phase_features, k: int = 0) -> Optional[np.ndarray]:
    """The input feature rows as model ``k`` sees them: the raw ``features`` through that model's own
    ``features_scaler`` (NaN -> 0; as they are without one), then the phase features, unscaled, as
    ``cli.run_training`` feeds them.  ``ValueError`` when the model needs features and gets none, gets features it
    does not take, or gets another width than it was trained on."""
    parts = []
    if features is not None:
        f = np.asarray(features, dtype=np.float64)
        parts.append(features_scaler.transform(f) if features_scaler is not None else f)
    if phase_features is not None:
        parts.append(np.asarray(phase_features, dtype=np.float64))
    needs = bool(getattr(model.encoder, 'use_input_features', False))
    if not parts:
        if needs:
            raise ValueError(f'model {k} was trained with input features: give the same feature files to predict')
        return None
    if not needs:
        raise ValueError(f'model {k} was trained without input features, but features were given')
    rows = np.concatenate(parts, axis=1)
    lin = next(m for m in model.ffn if isinstance(m, torch.nn.Linear))
    width = lin.in_features - sum(e.hidden_size + getattr(e, 'atom_descriptors_size', 0)
                                  for e in getattr(model.encoder, 'encoder', ()))
    if rows.shape[1] != width:
        raise ValueError(f'model {k} was trained with {width} input features and {rows.shape[1]} were given')
    return rows


def predict_ensemble(checkpoints_or_models, graphs: Sequence, batch_size: int, features=None, phase_features=None,
                     phase_mask=None, variance: bool = False, individual: bool = False, device=None,
                     n_models: Optional[int] = None, features_scaling: bool = True, embeddings: bool = False,
                     atom_descriptors=None, atom_descriptor_scaling: bool = True, atom_features=None,
                     bond_features=None, bond_feature_scaling: bool = True):
    """The ensemble's predictions of ``graphs`` (``MolGraph`` records, one per row): ``(mean, variance,
    individual)`` as float64 numpy arrays, ``[N][W]``, ``[N][W]`` (for spectra models the per-row pairwise SID
    ``[N]``; None without ``variance``) and ``[M][N][W]`` (None without ``individual``).  W is the flat output width:
    tasks, spectrum positions, or tasks x classes.

    ``checkpoints_or_models``: checkpoint paths, ``(model, data_scaler, features_scaler)`` tuples or models, handled
    one after the other (a generator works; ``n_models`` is then needed when per-model slabs are kept).  Every
    model is put in eval mode and sees its own feature table: the raw ``features`` ``[N][Ff]`` through its own
    ``features_scaler`` (``features_scaling=False``: as they are), ``phase_features`` ``[N][phases]`` appended
    unscaled.  Spectra predictions are normalised per row under the row's phase mask (``phase_mask``
    ``[phases][T]``); excluded positions are NaN.  The predictions leave the device once, after the last model.

    ``embeddings``: return a fourth value as well, the ensemble-mean graph embeddings (make_predictions.py:156-195
    with ``--save_graph_embeddings``): float32 ``[N][F]``, the fp32 sum over the models, in order, of the FFN input
    of every row (the encoding, features joined), divided by the model count; gathered in the same pass as the
    predictions (``n_models`` is then needed with a generator of models).

    ``atom_descriptors``: one raw ``[n_atoms][d]`` array per row for models trained with ``--atom_descriptors
    descriptor``; every model builds its own device table with its own ``atom_descriptor_scaler``
    (``model_atom_descriptors``; ``atom_descriptor_scaling=False``: as they are).

    ``atom_features`` / ``bond_features``: one raw ``[n_atoms][da]`` / ``[n_bonds / 2][db]`` array per row for models
    trained with ``--atom_features_path`` / ``--bond_features_path``; every model sees the graphs widened by
    them through its own scalers (``model_graphs``), batched once per model."""
    device = torch.device('cuda', 0) if device is None else torch.device(device)
    if n_models is None and hasattr(checkpoints_or_models, '__len__'):
        n_models = len(checkpoints_or_models)
    batches = None
    n = len(graphs)
    acc = spectra = emb_acc = None
    row_mask = None
    k = -1
    for k, item in enumerate(checkpoints_or_models):
        model, data_scaler, features_scaler = _open_model(item, device)
        model.eval()
        set_feature_sizes_of(model)
        own = model_graphs(item, model, graphs, atom_features, bond_features, atom_descriptor_scaling,
                           bond_feature_scaling, k)
        if own is not graphs:  # (extra features through this model's scalers: its own batches)
            batches = None
        if batches is None:  # (rows of several molecules: with the merged graphs a shared encoder runs once over)
            from .slots import shares_encoder
            batches = make_batches(own, batch_size, shared=shares_encoder(model))
        is_spectra = bool(getattr(model, 'spectra', False))
        width = int([m for m in model.ffn if isinstance(m, torch.nn.Linear)][-1].out_features)
        if acc is None:
            spectra = is_spectra
            keep = individual or (variance and spectra)
            if keep and n_models is None:
                raise ValueError('predict_ensemble: pass n_models with a generator of models when the individual '
                                 'predictions (or a spectra ensemble\'s spread) are wanted')
            acc = EnsembleAccumulator(n, width, device, variance=variance and not spectra, keep=keep,
                                      n_models=n_models)
            if embeddings:
                from .fingerprint import LatentAccumulator
                if n_models is None:
                    raise ValueError('predict_ensemble: pass n_models with a generator of models when the graph '
                                     'embeddings are wanted')
                first = next(m for m in model.ffn if isinstance(m, torch.nn.Linear))
                emb_acc = LatentAccumulator(n, int(first.in_features), device, n_models=n_models, columns=False,
                                            running_sum=True)
            if spectra and phase_features is not None and phase_mask is not None:
                row_mask = torch.from_numpy(np.ascontiguousarray(phase_row_mask(phase_features, phase_mask))).to(device)
                if tuple(row_mask.shape) != (n, width):
                    raise ValueError(f'a phase mask of shape {tuple(row_mask.shape)} for {n} rows of {width} '
                                     'spectrum positions')
        elif is_spectra != spectra or width != acc.width:
            raise ValueError(f'model {k} predicts {"spectra" if is_spectra else "values"} of width {width}; the '
                             f'ensemble\'s first model {"spectra" if spectra else "values"} of width {acc.width}')
        rows = model_features(model, features, features_scaler if features_scaling else None, phase_features, k)
        table = None if rows is None else FeatureTable(rows, device)
        desc = model_atom_descriptors(item, model, atom_descriptors, device, atom_descriptor_scaling, k)
        accumulate_model(acc, k, model, batches, data_scaler, table, row_mask, embeddings=emb_acc,
                         atom_descriptors=desc)
        del model, table, desc
    if acc is None:
        raise ValueError('predict_ensemble: no model given')
    if n == 0:
        empty = (np.zeros((0, acc.width)), None, None)
        return empty + (np.zeros((0, emb_acc.width), dtype=np.float32),) if embeddings else empty
    mean = acc.mean().cpu().numpy()
    spread = None
    if variance:
        spread = (acc.roundrobin_sid() if spectra else acc.variance()).cpu().numpy()
    out = (mean, spread, acc.individual().cpu().numpy() if individual else None)
    return out + (emb_acc.mean32().cpu().numpy(),) if embeddings else out
