"""``chemprop_train`` counterpart for the wD-MPNN on MI355X (BASELINE.json configs[0]: ``chemprop_train
--polymer`` regression on a small polymer CSV, depth 3, hidden 300).

    python -m chemprop_amd.cli --data_path polymers.csv --graphs_path polymers.npz --dataset_type regression \
        --polymer --save_dir out [--epochs 30 --batch_size 50 --depth 3 --hidden_size 300 ...]

The run follows the reference's ``cross_validate`` -> ``run_training`` -> ``train`` chain for one fold
(cross_validate.py:22-115, run_training.py:28-499, train.py:17-113), with the pieces outside the hot path
restated here:

* data: CSV with a header; the first column holds the (polymer) SMILES, the others the targets, empty
  cells = missing (utils.py get_data); graphs come pre-featurised from ``--graphs_path`` (one MolGraph
  record per row, ``chemprop_amd.graph_io``) since RDKit featurisation is out of scope here;
  ``--polymer`` checks every SMILES cell as a polymer string (``chemprop_amd.polymer``);
* split: ``split_type random`` with ``split_sizes`` and ``seed`` (data/utils.py:536-547), the default
  branch the fork lost in run_training.py:58-89 and that run_training_V0.py:74-81 still has;
* targets scaled by a StandardScaler fit on the training set (scaler.py:6-63) for regression;
  ``--dataset_type multiclass``: every target cell is a class index in ``[0, --multiclass_num_classes)``
  (checked before training, the CSV row named on failure), no scaler, ``cross_entropy`` as the default
  metric (args.py:557-558), ``test_preds.csv`` with one ``<task>_class_<k>`` column per class
  (make_predictions.py:213);
  ``--dataset_type spectra``: one target column per spectrum position; the targets of every split are
  normalised once (``spectra_utils.normalize_spectra`` with ``--spectra_target_floor``, per row, under the
  row's phase mask: ``--phase_features_path`` one-hot rows x ``--spectra_phase_mask_path``), no scaler, the
  SID loss (``--alternative_loss_function wasserstein`` for the other one), ``sid`` as the default metric,
  scored over all positions together (evaluate.py:48-50); the phase features are input features of the model
  (data/utils.py:250-258); predictions are normalised on the device and ``test_preds.csv`` leaves the
  positions a row's phase excludes empty (make_predictions.py:175-181);
* ``--features_path F [F ...]``: molecule features, the files' columns side by side (data/utils.py:242-246),
  standardised by a StandardScaler(replace_nan_token=0) fit on the training split unless
  ``--no_features_scaling`` (run_training.py:111-114; stored as the checkpoint's ``features_scaler``), phase
  features appended after them unscaled; each split's rows live in one ``features.FeatureTable`` on the
  device, an epoch's shuffled order is one index upload and a step takes a slice of it, so these models
  train on the direct step and from cached encodings;
* ``--number_of_molecules N [--mpn_shared] --extra_graphs_path G2 [.. GN]``: N molecules per row, the first N CSV
  columns being their SMILES (the reference's default ``smiles_columns``) and ``--graphs_path`` / the extra files
  their graphs in column order; a step's batch is a ``slots.SlotBatch``, so these models train on the direct step
  too; the checkpoint's args hold both settings, and the prediction tools read them there;
* MoleculeModel + initialize_weights after ``torch.manual_seed(pytorch_seed)`` (run_training.py:36,
  model.py:39), Adam (utils.py:295-310), NoamLR stepped per batch (utils.py:490-541, nn_utils.py:115-194),
  training batches reshuffled every epoch by one ``Random(seed)`` (data.py:537-587);
* each epoch: train, evaluate validation and training sets (evaluate.py), ``train_val_loss_log.csv``,
  ``model.pt``; the best validation score (``--metric``, rmse by default) keeps ``best_model.pt``;
* test: best weights, predictions inverse-scaled, ``test_scores.json`` / ``test_scores.csv``
  (run_training.py:440-491, cross_validate.py:149-172) and ``test_preds.csv``;
* ``--ensemble_size M`` (run_training.py:208-499): M models, one after the other, each into ``save_dir/model_<k>/``
  with its own ``test_scores.json``; the seeds are set once, so model 0 is the model of a run without the flag and
  the later ones continue the random streams; every model's test predictions are folded into one
  ``ensemble.EnsembleAccumulator`` on the device, and the top-level scores and ``test_preds.csv`` are the ensemble's;
* ``--device_metrics``: the per-epoch validation and training scores and a single model's test scores come from
  ``evaluate.evaluate`` (resident targets, partial sums on the device) instead of ``predict`` +
  ``evaluate_predictions``; the same files are written;
* ``--resident_graphs``: the training split's graphs are encoded once into a ``graph_table.GraphTable`` on the
  device; each epoch's order is one index upload next to the feature and descriptor indices, each step's graphs a
  slice of it (one gather launch assembles the batch's compact image, the usual build launch expands it), and
  every split's scoring batches are built once per run; a split the table refuses (extra features, a molecule
  larger than a block) is reported in one line and trains on the list path; every output is bitwise unchanged;
* ``--atom_messages`` (args.py:323): messages between atoms; the batches' graphs come from the same compact codes
  (``wdmpnn_build_graph_atom``), with ``--resident_graphs`` too, and the step skips autograd as for bond messages;
  the flag is stored in the checkpoint, where ``chemprop_predict`` and ``chemprop_fingerprint`` find it; with
  ``--undirected`` it is an argument error;
* every prediction above walks its split with ``predict.device_predictions``: ``predict`` copies the batches to the
  host, the ensemble's accumulator and ``evaluate``'s evaluator take them where the head wrote them.

``chemprop_predict`` (``python -m chemprop_amd.cli predict --test_path CSV --graphs_path NPZ --preds_path OUT
--checkpoint_dir D | --checkpoint_path P | --checkpoint_paths P ...``) is make_predictions.py's counterpart: the
predictions of one checkpoint or the mean of an ensemble (``ensemble.predict_ensemble``), with
``--ensemble_variance`` (spectra: the round-robin SID) and ``--individual_ensemble_predictions``;
``--save_graph_embeddings --graph_embeddings_path P`` also saves the ensemble-mean FFN inputs as a float32 ``.npy``.

``chemprop_fingerprint`` (``python -m chemprop_amd.cli fingerprint ... --fingerprint_type MPN | last_FFN``, the same
checkpoint and feature arguments) is molecule_fingerprint.py's counterpart: every checkpoint's latent vectors of
every row (``fingerprint.molecule_fingerprint``) as ``fp_j`` / ``fp_j_model_i`` columns.

The encoder runs on the HIP path (a GPU is required, like every ``chemprop_amd`` forward).  Checkpoints
(``model.pt``, ``best_model.pt``) have the layout of the reference's ``save_checkpoint`` (utils.py:47-73):
``args`` (a plain dict), ``state_dict`` (the reference's parameter names), ``data_scaler`` /
``features_scaler`` / ``atom_descriptor_scaler`` / ``bond_feature_scaler`` as ``{'means', 'stds'}`` lists
or None -- only plain types, so ``torch.load(..., weights_only=True)`` reads them; ``load_checkpoint`` and
``load_scalers`` read them back (utils.py:80-131, 263-293).
"""
from __future__ import annotations

import argparse
import csv
import json
import math
import os
import re
import sys
from random import Random
from typing import Dict, List, Optional

import numpy as np
import torch

from ._native import ENSEMBLE_MAX_MODELS, MAX_SLOTS
from .args import TrainArgs
from .featurization import BatchMolGraph
from .ensemble import EnsembleAccumulator, accumulate_model, make_batches, predict_ensemble
from .evaluate import Evaluator, TargetTable, evaluate
from .features import FeatureTable
from .graph_table import GraphTable
from .graph_io import load_graphs
from .model import MoleculeModel
from .nn_utils import initialize_weights
from .polymer import split_polymer_string, parse_polymer_rules
from .spectra_utils import load_phase_mask, normalize_spectra, phase_row_mask, sid_metric, wasserstein_metric
from .atom_descriptors import AtomDescriptorTable
from .predict import LATENT_TYPES, device_predictions
from .slots import SlotBatch, shares_encoder
from .train import NoamLR, _predict_head, build_optimizer, frozen_encodings, get_loss_func, train_step


class StandardScaler:
    """scaler.py:6-63 (means / stds over axis 0 ignoring missing values; nan -> 0 / 1, zero std -> 1)."""

    def __init__(self, means=None, stds=None, replace_nan_token=None):
        self.means, self.stds, self.replace_nan_token = means, stds, replace_nan_token

    def fit(self, X):
        X = np.array(X).astype(float)
        self.means = np.nanmean(X, axis=0)
        self.stds = np.nanstd(X, axis=0)
        self.means = np.where(np.isnan(self.means), np.zeros(self.means.shape), self.means)
        self.stds = np.where(np.isnan(self.stds), np.ones(self.stds.shape), self.stds)
        self.stds = np.where(self.stds == 0, np.ones(self.stds.shape), self.stds)
        return self

    def transform(self, X):
        X = np.array(X).astype(float)
        t = (X - self.means) / self.stds
        return np.where(np.isnan(t), self.replace_nan_token, t)

    def inverse_transform(self, X):
        X = np.array(X).astype(float)
        t = X * self.stds + self.means
        return np.where(np.isnan(t), self.replace_nan_token, t)


def _scaler_to_dict(sc: Optional[StandardScaler]):
    """utils.py:58-62: means / stds as plain lists (None without a scaler)."""
    if sc is None:
        return None
    conv = (lambda v: np.asarray(v, dtype=float).tolist() if v is not None else None)
    return {'means': conv(sc.means), 'stds': conv(sc.stds)}


def _plain(v):
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return str(v)  # e.g. torch.device


def save_checkpoint(path: str, model, scaler: Optional[StandardScaler] = None,
                    features_scaler: Optional[StandardScaler] = None, args=None,
                    atom_descriptor_scaler: Optional[StandardScaler] = None,
                    bond_feature_scaler: Optional[StandardScaler] = None) -> None:
    """utils.py:47-73: {'args', 'state_dict', 'data_scaler', 'features_scaler', 'atom_descriptor_scaler',
    'bond_feature_scaler'}; every value a plain type (weights_only-loadable)."""
    a = {} if args is None else {k: _plain(v) for k, v in (vars(args) if not isinstance(args, dict) else args).items()}
    torch.save({'args': a, 'state_dict': model.state_dict(), 'data_scaler': _scaler_to_dict(scaler),
                'features_scaler': _scaler_to_dict(features_scaler),
                'atom_descriptor_scaler': _scaler_to_dict(atom_descriptor_scaler),
                'bond_feature_scaler': _scaler_to_dict(bond_feature_scaler)}, path)


def load_checkpoint(path: str, device=None):
    """utils.py:80-131 for this module's checkpoints: a MoleculeModel rebuilt from the stored args with the
    stored weights (``encoder.encoder.W*`` names of older checkpoints remapped to ``encoder.encoder.0.W*``,
    utils.py:114-115).  Loaded with weights_only=True: nothing in the file is executed."""
    state = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(state, dict) or 'state_dict' not in state:
        raise ValueError(f'{path} is not a checkpoint (no state_dict)')
    sd = {re.sub(r'^encoder\.encoder\.([Wc])', r'encoder.encoder.0.\1', k): v for k, v in state['state_dict'].items()}
    if 'args' not in state:
        return sd
    fields = set(TrainArgs.__dataclass_fields__)
    kw = {k: v for k, v in state['args'].items() if k in fields and k != 'device'}
    args = TrainArgs(**kw, device=torch.device(device) if device is not None else torch.device('cpu'))
    set_feature_sizes(args)  # (the encoder's row widths: the extra atom / bond features the model was trained with)
    model = MoleculeModel(args)
    model.load_state_dict(sd)
    return model.to(args.device)


def load_frzn_checkpoint(model, path: str, log=None) -> tuple:
    """``--checkpoint_frzn`` (run_training.py:271-285): copy into ``model`` every tensor of the checkpoint at
    ``path`` whose name and shape match one of the model's (``strict=False`` semantics); returns (names loaded,
    names skipped) and reports both through ``log``.  The file is read with ``weights_only=True``; its weights
    are under ``state_dict`` (this package's and the reference's ``save_checkpoint``, utils.py:47-73) or
    ``model_state_dict`` (the fork's pretraining files, run_training.py:275); ``encoder.encoder.W*`` names of
    older checkpoints are remapped as in ``load_checkpoint``.  ``ValueError`` when nothing matches.  Loading
    freezes nothing: that is ``apply_freezing``."""
    log = log or (lambda msg: print(msg, file=sys.stderr))
    state = torch.load(path, map_location='cpu', weights_only=True)
    sd = None
    if isinstance(state, dict):
        sd = state.get('state_dict', state.get('model_state_dict'))
    if not isinstance(sd, dict):
        raise ValueError(f'{path} is not a checkpoint (no state_dict or model_state_dict)')
    sd = {re.sub(r'^encoder\.encoder\.([Wc])', r'encoder.encoder.0.\1', k): v for k, v in sd.items()}
    own = model.state_dict()
    loaded, skipped = [], []
    for name, t in sd.items():
        if not isinstance(t, torch.Tensor) or name not in own:
            skipped.append(name)
            log(f'checkpoint_frzn: skipped {name} (no such parameter in the model)')
        elif tuple(own[name].shape) != tuple(t.shape):
            skipped.append(name)
            log(f'checkpoint_frzn: skipped {name} (shape {tuple(t.shape)}, the model has {tuple(own[name].shape)})')
        else:
            loaded.append(name)
    if not loaded:
        raise ValueError(f'{path}: no tensor matches the model by name and shape')
    model.load_state_dict({k: sd[k] for k in loaded}, strict=False)
    log(f'checkpoint_frzn: loaded {len(loaded)} tensors from {path}: {", ".join(loaded)}')
    return loaded, skipped


def apply_freezing(model, frzn_encoder: bool = False, frzn_ffn_layers: int = 0) -> None:
    """``--frzn_encoder`` / ``--frzn_ffn_layers N``.  ``frzn_encoder`` freezes every encoder parameter
    (run_training.py:287-291).  ``frzn_ffn_layers = N > 0`` freezes the FIRST N ``Linear`` layers of the FFN,
    weight and bias, and implies a frozen encoder: the documented meaning (args.py:430-435) and what
    model.py:118-121 aims at.  It is not run_training.py:302-305, whose loop freezes the LAST 2N tensors of the
    FFN against its own help text; and unlike model.py's ``parameters()[0:2N]`` slice it counts Linear layers,
    so a PReLU slope or a bias-free layer does not shift the cut.  ``N >= `` the FFN's Linear layers is a
    ``ValueError`` (nothing would train).  With neither flag every parameter trains (run_training.py:277-285)."""
    if frzn_ffn_layers < 0:
        raise ValueError('--frzn_ffn_layers must not be negative')
    linears = [m for m in model.ffn if isinstance(m, torch.nn.Linear)]
    if frzn_ffn_layers >= len(linears) and frzn_ffn_layers > 0:
        raise ValueError(f'--frzn_ffn_layers {frzn_ffn_layers}: the FFN has {len(linears)} Linear layers, and at '
                         'least one must stay trainable')
    if frzn_encoder or frzn_ffn_layers > 0:
        for p in model.encoder.parameters():
            p.requires_grad = False
    for lin in linears[:frzn_ffn_layers]:
        for p in lin.parameters():
            p.requires_grad = False


def subsample_train(n_train: int, frac: float, seed: int) -> List[int]:
    """``--train_frac`` (run_training.py:132-137): the positions kept of a training split of ``n_train`` rows,
    ``default_rng(seed).choice(n_train, int(n_train * frac), replace=False)``."""
    if not 0 < frac <= 1:
        raise ValueError('--train_frac must be in (0, 1]')
    return np.random.default_rng(seed).choice(n_train, int(n_train * frac), replace=False).tolist()


def load_scalers(path: str):
    """utils.py:263-293: (data scaler, features scaler, atom descriptor scaler, bond feature scaler)."""
    state = torch.load(path, map_location='cpu', weights_only=True)

    def mk(d, nan_token=None):
        if d is None:
            return None
        return StandardScaler(np.asarray(d['means'], dtype=float), np.asarray(d['stds'], dtype=float),
                              replace_nan_token=nan_token)
    return (mk(state.get('data_scaler')), mk(state.get('features_scaler'), 0),
            mk(state.get('atom_descriptor_scaler'), 0), mk(state.get('bond_feature_scaler'), 0))


def random_split(n: int, sizes, seed: int):
    """data/utils.py:536-547 (split_type 'random') on row indices."""
    if not (len(sizes) == 3 and sum(sizes) == 1):
        raise ValueError('Valid split sizes must sum to 1 and must have three sizes: train, validation, and test.')
    indices = list(range(n))
    Random(seed).shuffle(indices)
    train_size = int(sizes[0] * n)
    train_val_size = int((sizes[0] + sizes[1]) * n)
    return indices[:train_size], indices[train_size:train_val_size], indices[train_val_size:]


def metric_value(metric: str, targets: List[float], preds: List[float]) -> float:
    """utils.py get_metric_func for the scalar metrics.  ``cross_entropy`` (multiclass: preds are per-class
    probability lists) is ``log_loss`` over the labels ``0 .. C-1`` as evaluate.py:72-74 calls it, so a class
    absent from ``targets`` keeps its column; ``accuracy`` (utils.py:416-432) takes the argmax of list
    predictions and thresholds scalar ones at 0.5."""
    from sklearn.metrics import accuracy_score, log_loss, mean_absolute_error, mean_squared_error, r2_score, \
        roc_auc_score
    if metric == 'sid':
        return sid_metric(preds, targets)
    if metric == 'wasserstein':
        return wasserstein_metric(preds, targets)
    if metric == 'rmse':
        return math.sqrt(mean_squared_error(targets, preds))
    if metric == 'mse':
        return mean_squared_error(targets, preds)
    if metric == 'mae':
        return mean_absolute_error(targets, preds)
    if metric == 'r2':
        return r2_score(targets, preds)
    if metric == 'auc':
        return roc_auc_score(targets, preds)
    if metric == 'cross_entropy':
        if isinstance(preds[0], (list, tuple)):
            return log_loss(targets, preds, labels=list(range(len(preds[0]))))
        return log_loss(targets, preds)
    if metric == 'accuracy':
        if isinstance(preds[0], (list, tuple)):  # multiclass
            hard = [list(p).index(max(p)) for p in preds]
        else:
            hard = [1 if p > 0.5 else 0 for p in preds]
        return accuracy_score(targets, hard)
    raise ValueError(f'Metric "{metric}" not supported.')


def evaluate_predictions(preds, targets, num_tasks: int, metrics: List[str], dataset_type: str) -> Dict[str, list]:
    """evaluate.py:11-77: per task over the rows with a target; spectra (evaluate.py:48-50): one score per
    metric over all positions together (``sid_metric`` / ``wasserstein_metric`` on the rows as they are, None
    = missing or excluded)."""
    if dataset_type == 'spectra':
        if len(preds) == 0:
            return {m: [float('nan')] for m in metrics}
        return {m: [metric_value(m, targets, preds)] for m in metrics}
    if len(preds) == 0:
        return {m: [float('nan')] * num_tasks for m in metrics}
    out = {m: [] for m in metrics}
    for i in range(num_tasks):
        vp = [preds[j][i] for j in range(len(preds)) if targets[j][i] is not None]
        vt = [targets[j][i] for j in range(len(preds)) if targets[j][i] is not None]
        if dataset_type == 'classification' and (all(t == 0 for t in vt) or all(t == 1 for t in vt) or
                                                 all(p == 0 for p in vp) or all(p == 1 for p in vp)):
            for m in metrics:
                out[m].append(float('nan'))
            continue
        if not vt:
            continue
        for m in metrics:
            out[m].append(metric_value(m, vt, vp))
    return out


def predict(model, graphs, idx, batch_size: int, scaler: Optional[StandardScaler],
            encodings: Optional[torch.Tensor] = None, features=None, spectra_mask=None,
            atom_descriptors=None, batches=None) -> List[List[float]]:
    """predict.py:10-68: eval, no_grad, batches in order, inverse scaling: the batches of
    ``predict.device_predictions`` copied to the host.  ``encodings``: the rows of ``idx`` from ``frozen_encodings``
    (a frozen encoder's outputs, computed once per run): the native prediction head on them in place of the
    model's forward (``NotImplementedError`` for an FFN the native heads refuse; the same for a spectra model).
    ``features``: the input feature rows of the whole data set (numpy rows, indexed by ``idx``), or the split's
    own ``features.FeatureTable`` (row k = ``idx[k]``'s features).  A spectra model's predictions are normalised
    per row on the device (make_predictions.py:175-181): ``spectra_mask`` is the bool ``[len(idx)][T]`` array of
    the positions each row's phase includes (None: all), uploaded once; excluded positions come back as None.
    ``atom_descriptors``: the split's ``AtomDescriptorTable`` (molecule k = ``idx[k]``'s rows, already scaled), or
    the scaled arrays of the whole data set (a list indexed by ``idx``), for a descriptor model.
    ``batches``: the ``make_batches`` of ``idx``'s graphs built earlier (``graphs`` is then not read), for a caller
    that scores the same split many times.  The ``BatchMolGraph`` s of the whole split are held at once."""
    model.eval()
    if not len(idx):
        return []
    device = next(model.parameters()).device
    spectra = bool(getattr(model, 'spectra', False))
    if features is not None and not isinstance(features, FeatureTable):
        features = FeatureTable(np.stack([features[i] for i in idx]), device)
    if features is not None and len(features) != len(idx):
        raise ValueError(f'a feature table of {len(features)} rows for {len(idx)} molecules')
    if atom_descriptors is not None and not isinstance(atom_descriptors, AtomDescriptorTable):
        atom_descriptors = AtomDescriptorTable([atom_descriptors[i] for i in idx], device)
    native = spectra or encodings is not None or atom_descriptors is not None
    if native and _predict_head(model) is None and atom_descriptors is None:
        raise NotImplementedError('predict: the model\'s FFN is not one the native prediction heads run')
    if encodings is not None:
        batches = batch_size
    elif batches is None:
        batches = make_batches([graphs[i] for i in idx], batch_size, shared=shares_encoder(model))
    outs = device_predictions(model, batches, features, device_mask(spectra_mask, device) if spectra else None,
                              encodings, own_forward=not native, n_rows=len(idx), atom_descriptors=atom_descriptors)
    preds = torch.cat([out for _, out in outs]).cpu().numpy().tolist()
    if spectra:
        preds = [[None if math.isnan(v) else v for v in row] for row in preds]
    if scaler is not None:
        preds = scaler.inverse_transform(preds).tolist()
    return preds


def device_mask(mask, device, idx=None) -> Optional[torch.Tensor]:
    """The rows ``idx`` (None: all) of a spectra phase mask ``[N][T]`` on the device; None for no mask or no rows."""
    if mask is None or (idx is not None and not len(idx)):
        return None
    return torch.from_numpy(np.ascontiguousarray(mask if idx is None else mask[idx])).to(device)


def read_csv(path: str):
    with open(path) as f:
        rows = list(csv.reader(f))
    header, body = rows[0], [r for r in rows[1:] if r]
    smiles = [r[0] for r in body]
    targets = [[float(x) if x.strip() != '' else None for x in r[1:]] for r in body]
    return header, smiles, targets


def read_csv_molecules(path: str, number_of_molecules: int):
    """``read_csv`` for ``number_of_molecules`` molecules per row: the first N columns are the SMILES columns (the
    reference's default ``smiles_columns``), the rest the targets.  Returns (header, one list of N SMILES per row,
    targets).  ``ValueError`` for a CSV of fewer than N + 1 columns."""
    n = int(number_of_molecules)
    with open(path) as f:
        rows = list(csv.reader(f))
    header, body = rows[0], [r for r in rows[1:] if r]
    if len(header) < n + 1:
        raise ValueError(f'{path} has {len(header)} columns: {n} SMILES columns and at least one target column are '
                         f'needed for --number_of_molecules {n}')
    smiles = [list(r[:n]) for r in body]
    targets = [[float(x) if x.strip() != '' else None for x in r[n:]] for r in body]
    return header, smiles, targets


def set_feature_sizes(args) -> None:
    """The widths ``MPN`` takes from ``get_atom_fdim`` / ``get_bond_fdim`` for a model of these args (train /
    make_predictions call ``set_extra_atom_fdim(args.atom_features_size)`` and ``set_extra_bond_fdim`` the same
    way): the extra atom / bond feature columns, 0 without them."""
    from .featurization import set_extra_atom_fdim, set_extra_bond_fdim
    feature = getattr(args, 'atom_descriptors', None) == 'feature'
    set_extra_atom_fdim(int(getattr(args, 'atom_features_size', 0) or 0) if feature else 0)
    set_extra_bond_fdim(int(getattr(args, 'bond_features_size', 0) or 0))


def check_number_of_molecules(n: int, extra_graphs_path, atom_descriptors=None, bond_features_path=None) -> None:
    """``--number_of_molecules`` in 1 .. 8 with one graph file per molecule (``--graphs_path`` for the first,
    ``--extra_graphs_path`` for the others), and no atom descriptors with several molecules (the reference's own
    refusal, mpn.py:249-251)."""
    if not 1 <= n <= MAX_SLOTS:
        raise ValueError(f'--number_of_molecules must be in 1 .. {MAX_SLOTS} (got {n})')
    extra = list(extra_graphs_path or [])
    if len(extra) != n - 1:
        raise ValueError(f'--number_of_molecules {n} needs {n - 1} --extra_graphs_path file(s), the graphs of molecules '
                         f'2 .. {n} ({len(extra)} given)')
    if n > 1 and atom_descriptors is not None:
        raise ValueError('Atom descriptors are currently only supported with one molecule per input (i.e., '
                         'number_of_molecules = 1).')
    if n > 1 and bond_features_path is not None:
        raise ValueError('Bond descriptors are currently only supported with one molecule per input (i.e., '
                         'number_of_molecules = 1): --bond_features_path with --number_of_molecules > 1')


def load_molecule_graphs(graphs_path: str, extra_graphs_path, n_rows: int, smiles_rows=None, polymer: bool = False):
    """The graphs of every row: a list of ``MolGraph`` for one molecule per row, a list of per-row tuples of N for
    several (slot k from ``graphs_path`` for k = 0, ``extra_graphs_path[k - 1]`` otherwise).  ``ValueError`` when a
    table does not hold one graph per CSV row.  ``polymer``: ``check_polymer_rows`` on every SMILES column against
    its own slot's graphs (``smiles_rows``: one list of N strings per row)."""
    paths = [graphs_path] + list(extra_graphs_path or [])
    tables = []
    for k, path in enumerate(paths):
        graphs = load_graphs(path)
        if len(graphs) != n_rows:
            raise ValueError(f'{path} holds {len(graphs)} graphs for {n_rows} CSV rows')
        if polymer and smiles_rows is not None:
            check_polymer_rows([r[k] for r in smiles_rows], graphs)
        tables.append(graphs)
    return tables[0] if len(tables) == 1 else list(zip(*tables))


def read_class_targets(path: str, num_classes: int, number_of_molecules: int = 1) -> List[List[Optional[int]]]:
    """The target cells of a multiclass CSV as class indices (empty = missing): every other cell must be an
    integer in [0, num_classes), else ValueError naming the CSV row (1-based, the header being row 1).  The first
    ``number_of_molecules`` columns hold the SMILES."""
    with open(path) as f:
        rows = list(csv.reader(f))
    out = []
    for n, r in enumerate(rows[1:], start=2):
        if not r:
            continue
        row = []
        for col, x in enumerate(r[number_of_molecules:], start=number_of_molecules + 1):
            if x.strip() == '':
                row.append(None)
                continue
            try:
                v = float(x)
            except ValueError:
                v = float('nan')
            if not (v.is_integer() and 0 <= v < num_classes):  # (False for nan and inf)
                raise ValueError(f'{path}, row {n}, column {col}: {x!r} is not an integer class index in '
                                 f'[0, {num_classes})')
            row.append(int(v))
        out.append(row)
    return out


def load_features(path: str) -> np.ndarray:
    """features/utils.py load_features for ``.csv`` (a header row, then one row of numbers per molecule) and
    ``.npy``: float64 ``[N][features]``."""
    if path.endswith('.npy'):
        return np.asarray(np.load(path), dtype=np.float64)
    with open(path) as f:
        reader = csv.reader(f)
        next(reader)
        return np.array([[float(v) for v in row] for row in reader if row], dtype=np.float64)


def load_phase_features(path: str, n_rows: int) -> np.ndarray:
    """data/utils.py:250-254: the one-hot phase rows, one per CSV row."""
    feats = load_features(path)
    if feats.ndim != 2 or len(feats) != n_rows:
        raise ValueError(f'{path} holds {len(feats)} phase rows for {n_rows} CSV rows')
    for row in feats:
        if not (row.sum() == 1 and np.count_nonzero(row) == 1):
            raise ValueError('Phase features must be one-hot encoded.')
    return feats


def load_input_features(paths: List[str], n_rows: int) -> np.ndarray:
    """``--features_path`` (data/utils.py:242-246): the files' columns side by side, one row per CSV row,
    float64 ``[n_rows][features]``."""
    parts = []
    for path in paths:
        f = load_features(path)
        if f.ndim != 2 or len(f) != n_rows or f.shape[1] < 1:
            raise ValueError(f'{path} holds features of shape {f.shape} for {n_rows} CSV rows')
        parts.append(f)
    if not parts:
        raise ValueError('--features_path needs at least one file')
    return np.concatenate(parts, axis=1)


def scale_features(features: np.ndarray, train_idx: List[int], no_features_scaling: bool = False):
    """run_training.py:111-114: ``(features of every row as the model sees them, the scaler or None)``.  Unless
    ``no_features_scaling``, a ``StandardScaler(replace_nan_token=0)`` is fitted on the training rows and applied
    to every row: NaN cells become 0, a column without variance keeps std 1."""
    if no_features_scaling:
        return features, None
    sc = StandardScaler(replace_nan_token=0).fit(features[train_idx])
    return sc.transform(features), sc


def check_atom_descriptor_args(mode: Optional[str], path: Optional[str]) -> None:
    """args.py:97-103, 596-607 for what this package reads: ``--atom_descriptors descriptor`` (rows joined to the
    atom hidden states) or ``feature`` (columns appended to the atom features) with an ``.npz`` file.
    ``ValueError`` with the reason for everything else."""
    if mode is None and path is None:
        return
    if mode is None:
        raise ValueError('--atom_descriptors_path is given without --atom_descriptors: say how the descriptors are '
                         'used (--atom_descriptors descriptor, or feature)')
    if mode not in ('descriptor', 'feature'):
        raise ValueError(f'--atom_descriptors {mode}: "descriptor" and "feature" are the supported modes')
    if path is None:
        raise ValueError(f'--atom_descriptors {mode} needs --atom_descriptors_path')
    check_atom_descriptors_path(path)


def check_bond_features_args(path: Optional[str], no_scaling: bool = False) -> None:
    """``--bond_features_path`` (args.py:105, 609-612): an ``.npz`` file; ``--no_bond_features_scaling`` only with it."""
    if path is None:
        if no_scaling:
            raise ValueError('--no_bond_features_scaling is given without --bond_features_path')
        return
    check_atom_descriptors_path(path)


def load_bond_features(path: str, graphs) -> List[np.ndarray]:
    """``--bond_features_path`` (features/utils.py:76-78, data.py:131-142): the arrays of an ``.npz`` file in file
    order, one float64 ``[n_bonds / 2][db]`` array per graph -- one row per undirected bond, in the order the
    graph's bond pairs were created (``bond_features_extra[bond.GetIdx()]``, featurization.py:460-468), both
    directed bonds of a pair taking the row -- NaN replaced by 0.  ``ValueError`` naming the first offender."""
    check_atom_descriptors_path(path)
    with np.load(path, allow_pickle=False) as container:
        arrays = [np.asarray(container[key]) for key in container]
    if len(arrays) != len(graphs):
        raise ValueError(f'{path} holds {len(arrays)} bond feature arrays for {len(graphs)} molecules')
    out = []
    for k, (a, g) in enumerate(zip(arrays, graphs)):
        if a.ndim != 2 or a.shape[1] < 1 or a.dtype.kind not in 'fiu':
            raise ValueError(f'{path}: array {k} has shape {a.shape} ({a.dtype}); a numeric [n_bonds / 2][d] array is '
                             'expected')
        if a.shape[1] != arrays[0].shape[1]:
            raise ValueError(f'{path}: array {k} has {a.shape[1]} features per bond, array 0 has '
                             f'{arrays[0].shape[1]}')
        if a.shape[0] != g.n_bonds // 2:
            raise ValueError(f'{path}: array {k} has {a.shape[0]} rows, molecule {k} has {g.n_bonds // 2} bonds (the '
                             'number of bonds is different from the length of the extra bond features)')
        a = a.astype(np.float64)
        out.append(np.where(np.isnan(a), 0.0, a))
    return out


def join_extra_features(graphs, atom_features=None, bond_features=None) -> list:
    """The graphs with their (scaled) extra atom / bond features appended to the rows, once per run
    (``featurization.widen_mol_graph``, the reference's concatenating mode): batches of the result are ordinary
    ``BatchMolGraph`` s whose extras travel beside the compact codes."""
    from .featurization import widen_mol_graph
    if atom_features is None and bond_features is None:
        return list(graphs)
    return [widen_mol_graph(g, None if atom_features is None else atom_features[k],
                            None if bond_features is None else bond_features[k]) for k, g in enumerate(graphs)]


def check_atom_descriptors_path(path: str) -> None:
    ext = os.path.splitext(path)[1].lower()
    if ext in ('.pkl', '.pckl', '.pickle'):
        raise ValueError(f'{path}: pickled descriptor tables are read with pandas, which this package does not '
                         'depend on; save the arrays with numpy.savez, one array per molecule in data order')
    if ext == '.sdf':
        raise ValueError(f'{path}: descriptors in an .sdf file are read with RDKit, which this package does not '
                         'depend on; save the arrays with numpy.savez, one array per molecule in data order')
    if ext != '.npz':
        raise ValueError(f'{path}: atom descriptors are read from an .npz file (numpy.savez: one [n_atoms][d] array '
                         'per molecule, in data order)')


def load_atom_descriptors(path: str, graphs) -> List[np.ndarray]:
    """``--atom_descriptors_path`` (features/utils.py:76-78, data/utils.py:310-339): the arrays of an ``.npz`` file
    in file order, one float64 ``[n_atoms][d]`` array per graph, NaN replaced by 0 (data.py:133-135).
    ``ValueError`` naming the first offender: another number of arrays than graphs, an array that is not 2-D, of
    another width than the first, or with another number of rows than its graph has atoms."""
    check_atom_descriptors_path(path)
    with np.load(path, allow_pickle=False) as container:
        arrays = [np.asarray(container[key]) for key in container]
    if len(arrays) != len(graphs):
        raise ValueError(f'{path} holds {len(arrays)} descriptor arrays for {len(graphs)} molecules')
    out = []
    for k, (a, g) in enumerate(zip(arrays, graphs)):
        if a.ndim != 2 or a.shape[1] < 1 or a.dtype.kind not in 'fiu':
            raise ValueError(f'{path}: array {k} has shape {a.shape} ({a.dtype}); a numeric [n_atoms][d] array is '
                             'expected')
        if a.shape[1] != arrays[0].shape[1]:
            raise ValueError(f'{path}: array {k} has {a.shape[1]} descriptors per atom, array 0 has '
                             f'{arrays[0].shape[1]}')
        if a.shape[0] != g.n_atoms:
            raise ValueError(f'{path}: array {k} has {a.shape[0]} rows, molecule {k} has {g.n_atoms} atoms (the '
                             'number of atoms is different from the length of the extra atom features)')
        a = a.astype(np.float64)
        out.append(np.where(np.isnan(a), 0.0, a))
    return out


def scale_atom_descriptors(descriptors: List[np.ndarray], train_idx: List[int],
                           no_atom_descriptor_scaling: bool = False):
    """data.py:432-478 with run_training.py:118-123: ``(every molecule's descriptors as the model sees them, the
    scaler or None)``.  Unless ``no_atom_descriptor_scaling``, a ``StandardScaler(replace_nan_token=0)`` is fitted on
    the stacked rows of the training molecules and applied to every molecule."""
    if no_atom_descriptor_scaling:
        return list(descriptors), None
    sc = StandardScaler(replace_nan_token=0).fit(np.vstack([descriptors[i] for i in train_idx]))
    return [sc.transform(a) for a in descriptors], sc


METRICS_OF = {'spectra': ('sid', 'wasserstein')}  # (args.py:568-573, for the metrics only spectra has)


def check_metrics(dataset_type: str, metrics: List[str]) -> None:
    """args.py:564-573 for the spectra metrics: ``sid`` and ``wasserstein`` are the metrics of spectra, and its
    only ones (``ValueError`` otherwise, with the reference's message)."""
    for m in metrics:
        if (dataset_type == 'spectra') != (m in METRICS_OF['spectra']):
            raise ValueError(f'Metric "{m}" invalid for dataset type "{dataset_type}".')


def parse_args(argv=None, spectra: bool = False) -> argparse.Namespace:
    """The arguments of ``chemprop_train``.  ``spectra``: also accept ``--dataset_type spectra`` (``chemprop_train``
    and ``python -m chemprop_amd.cli`` pass True).  Without it the parser keeps its earlier contract, which the
    suite pins: the dataset types are regression, classification and multiclass, and ``spectra`` is refused like
    any unknown type."""
    ap = argparse.ArgumentParser(prog='chemprop_train', description=__doc__.split('\n')[0])
    ap.add_argument('--data_path', required=True)
    ap.add_argument('--graphs_path', required=True, help='pre-featurised MolGraph records, one per CSV row')
    ap.add_argument('--number_of_molecules', type=int, default=1,
                    help='molecules per data row (1 .. 8): the first N CSV columns hold their SMILES')
    ap.add_argument('--mpn_shared', action='store_true', help='one encoder for every molecule of a row')
    ap.add_argument('--extra_graphs_path', nargs='+', default=None,
                    help='the graph files of molecules 2 .. N (--graphs_path holds molecule 1)')
    ap.add_argument('--dataset_type', default='regression',
                    choices=['regression', 'classification', 'multiclass'] + (['spectra'] if spectra else []))
    ap.add_argument('--multiclass_num_classes', type=int, default=3)
    ap.add_argument('--spectra_activation', default='exp', choices=['exp', 'softplus'],
                    help='the output activation that keeps a spectra model positive')
    ap.add_argument('--spectra_target_floor', type=float, default=1e-8,
                    help='spectra targets below this value are raised to it before they are normalised')
    ap.add_argument('--alternative_loss_function', default=None, choices=['wasserstein'],
                    help='spectra only: train on the Wasserstein loss instead of SID')
    ap.add_argument('--spectra_phase_mask_path', default=None,
                    help='CSV (header, label column): one 0/1 row per phase, 0 = position excluded for that phase')
    ap.add_argument('--phase_features_path', default=None,
                    help='CSV (header) or .npy: the one-hot phase of every data row; fed to the model as features')
    ap.add_argument('--features_path', nargs='+', default=None,
                    help='CSV (header) or .npy files of molecule features, one row per data row; their columns are '
                         'concatenated and fed to the FFN next to the encoding')
    ap.add_argument('--no_features_scaling', action='store_true',
                    help='feed the features of --features_path as they are (default: standardised on the training '
                         'split, NaN -> 0)')
    ap.add_argument('--atom_descriptors', default=None, choices=['feature', 'descriptor'],
                    help='descriptor: per-atom descriptors joined to the atom hidden states before the readout '
                         '(feature, extra columns of the atom features, is spelled --atom_features_path here)')
    ap.add_argument('--atom_descriptors_path', default=None,
                    help='.npz file: one [n_atoms][d] array per data row, in data order')
    ap.add_argument('--no_atom_descriptor_scaling', action='store_true',
                    help='feed the atom descriptors as they are (default: standardised on the training split)')
    ap.add_argument('--atom_features_path', default=None,
                    help='.npz file of extra atom features: one [n_atoms][d] array per data row, in data order, '
                         'appended to the atom features of the graphs (the reference\'s --atom_descriptors feature '
                         '--atom_descriptors_path; --no_atom_descriptor_scaling applies)')
    ap.add_argument('--bond_features_path', default=None,
                    help='.npz file of extra bond features: one [n_bonds / 2][d] array per data row, in data order, '
                         'appended to the bond features of the graphs')
    ap.add_argument('--no_bond_features_scaling', action='store_true',
                    help='feed the extra bond features as they are (default: standardised on the training split)')
    ap.add_argument('--save_dir', required=True)
    ap.add_argument('--polymer', action='store_true')
    ap.add_argument('--split_type', default='random', choices=['random'])
    ap.add_argument('--split_sizes', type=float, nargs=3, default=(0.8, 0.1, 0.1))
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--pytorch_seed', type=int, default=0)
    ap.add_argument('--metric', default=None)
    ap.add_argument('--extra_metrics', nargs='*', default=[])
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--batch_size', type=int, default=50)
    ap.add_argument('--warmup_epochs', type=float, default=2.0)
    ap.add_argument('--init_lr', type=float, default=1e-4)
    ap.add_argument('--max_lr', type=float, default=1e-3)
    ap.add_argument('--final_lr', type=float, default=1e-4)
    ap.add_argument('--grad_clip', type=float, default=None)
    for name, default in (('hidden_size', 300), ('depth', 3), ('ffn_num_layers', 2)):
        ap.add_argument(f'--{name}', type=int, default=default)
    ap.add_argument('--ffn_hidden_size', type=int, default=None)
    ap.add_argument('--dropout', type=float, default=0.0)
    ap.add_argument('--activation', default='ReLU')
    ap.add_argument('--aggregation', default='mean', choices=['mean', 'sum', 'norm'])
    ap.add_argument('--aggregation_norm', type=int, default=100)
    ap.add_argument('--bias', action='store_true')
    ap.add_argument('--undirected', action='store_true')
    ap.add_argument('--atom_messages', action='store_true',
                    help='pass messages between atoms instead of directed bonds (args.py:323); stored in the '
                         'checkpoint, which chemprop_predict and chemprop_fingerprint read it from')
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--weight_decay', type=float, default=0.0)
    ap.add_argument('--optimizer', default='adam', choices=['adam', 'adamw'])
    ap.add_argument('--checkpoint_frzn', default=None,
                    help='pretrained checkpoint: every tensor that matches by name and shape is loaded')
    ap.add_argument('--frzn_encoder', action='store_true', help='freeze every encoder parameter')
    ap.add_argument('--frzn_ffn_layers', type=int, default=0,
                    help='freeze the first N Linear layers of the FFN (implies --frzn_encoder)')
    ap.add_argument('--train_frac', type=float, default=1.0,
                    help='train on this fraction of the training split (drawn by --seed)')
    ap.add_argument('--no_encoding_cache', action='store_true',
                    help='run the frozen encoder every step instead of computing its encodings once')
    ap.add_argument('--ensemble_size', type=int, default=1,
                    help='train this many models, one after the other, into save_dir/model_<k>/; the test '
                         'predictions and scores are the ensemble\'s')
    ap.add_argument('--device_metrics', action='store_true',
                    help='score the validation, training and test splits on the device (evaluate.evaluate): the '
                         'targets stay resident, the predictions are not copied to the host per batch')
    ap.add_argument('--resident_graphs', action='store_true',
                    help='keep the training split\'s graphs on the device as compact codes (graph_table.GraphTable): '
                         'a step gathers its batch there instead of packing it on the host, and every split\'s '
                         'scoring batches are built once per run; results are bitwise unchanged')
    a = ap.parse_args(argv)
    if a.atom_messages and a.undirected:  # (the reference indexes atom messages with b2revb there, mpn.py:101-102)
        ap.error('--atom_messages cannot be combined with --undirected')
    if not 1 <= a.ensemble_size <= ENSEMBLE_MAX_MODELS:
        raise ValueError(f'--ensemble_size must be in 1 .. {ENSEMBLE_MAX_MODELS}')
    if a.alternative_loss_function is not None and a.dataset_type != 'spectra':
        raise ValueError(f'Alternative loss function "{a.alternative_loss_function}" not supported with dataset type '
                         f'"{a.dataset_type}".')
    if a.dataset_type == 'spectra' and not a.spectra_target_floor > 0:
        raise ValueError('--spectra_target_floor must be greater than 0')
    check_metrics(a.dataset_type, ([a.metric] if a.metric else []) + list(a.extra_metrics))
    if a.atom_descriptors == 'feature':  # (the command line keeps the refusal it always had for this spelling)
        raise ValueError('--atom_descriptors feature is not taken on the command line: in the reference such descriptors '
                         'become columns of the atom features when a molecule is featurised, and this tool reads graphs '
                         'that are featurised already (--graphs_path); give the file as --atom_features_path F.npz and '
                         'its scaled columns are joined to the graphs\' atom features, or use --atom_descriptors '
                         'descriptor')
    if a.atom_features_path is not None:  # the same run as the reference's --atom_descriptors feature
        if a.atom_descriptors is not None or a.atom_descriptors_path is not None:
            raise ValueError('--atom_features_path cannot be combined with --atom_descriptors / --atom_descriptors_path: '
                             'a run has one kind of atom descriptors, as in the reference')
        a.atom_descriptors, a.atom_descriptors_path = 'feature', a.atom_features_path
    check_atom_descriptor_args(a.atom_descriptors, a.atom_descriptors_path)
    check_bond_features_args(a.bond_features_path, a.no_bond_features_scaling)
    check_number_of_molecules(a.number_of_molecules, a.extra_graphs_path, a.atom_descriptors, a.bond_features_path)
    return a


def run_training(a: argparse.Namespace) -> Dict[str, list]:
    os.makedirs(a.save_dir, exist_ok=True)
    n_mols = int(getattr(a, 'number_of_molecules', 1))
    mpn_shared = bool(getattr(a, 'mpn_shared', False))
    extra_graphs = getattr(a, 'extra_graphs_path', None)
    check_number_of_molecules(n_mols, extra_graphs, getattr(a, 'atom_descriptors', None),
                              getattr(a, 'bond_features_path', None))
    if n_mols == 1:
        header, smiles, targets = read_csv(a.data_path)
        smiles_rows = [[s] for s in smiles]
    else:
        header, smiles_rows, targets = read_csv_molecules(a.data_path, n_mols)
        smiles = [r[0] for r in smiles_rows]
    # every row must be a well-formed polymer string (data.py:695-703, featurization.py:335-364)
    graphs = load_molecule_graphs(a.graphs_path, extra_graphs, len(smiles), smiles_rows, bool(a.polymer))
    num_tasks = len(header) - n_mols
    multiclass = a.dataset_type == 'multiclass'
    if multiclass:  # class indices, checked here: a bad one must not reach the loss on the device
        if a.multiclass_num_classes < 2:
            raise ValueError('--multiclass_num_classes must be at least 2')
        targets = read_class_targets(a.data_path, a.multiclass_num_classes, n_mols)
    spectra = a.dataset_type == 'spectra'
    phase_features = phase_mask = row_mask = None
    if spectra:  # run_training.py:146-157: every split's targets normalised once, per row, under its phase mask
        if a.phase_features_path is not None:
            phase_features = load_phase_features(a.phase_features_path, len(smiles))
        if a.spectra_phase_mask_path is not None:
            phase_mask = load_phase_mask(a.spectra_phase_mask_path)
        if phase_features is not None and phase_mask is not None:
            if np.asarray(phase_mask).shape != (phase_features.shape[1], num_tasks):
                raise ValueError(f'{a.spectra_phase_mask_path}: a mask of shape {np.asarray(phase_mask).shape} for '
                                 f'{phase_features.shape[1]} phases and {num_tasks} spectrum positions')
            row_mask = phase_row_mask(phase_features, phase_mask)
        targets = normalize_spectra(targets, phase_features, phase_mask, excluded_sub_value=None,
                                    threshold=a.spectra_target_floor)
    metric = a.metric or {'regression': 'rmse', 'multiclass': 'cross_entropy', 'spectra': 'sid'}.get(a.dataset_type,
                                                                                                     'auc')
    metrics = [metric] + [m for m in a.extra_metrics if m != metric]
    check_metrics(a.dataset_type, metrics)
    minimize = metric in ('rmse', 'mse', 'mae', 'cross_entropy', 'sid', 'wasserstein')
    device = torch.device('cuda', a.gpu)
    train_idx, val_idx, test_idx = random_split(len(smiles), a.split_sizes, a.seed)
    if a.train_frac != 1.0:  # run_training.py:132-137; the scalers below are fitted on the subsample
        train_idx = [train_idx[k] for k in subsample_train(len(train_idx), a.train_frac, a.seed)]
    # the model's input features: the --features_path columns, standardised on the training split
    # (run_training.py:111-114), then the phase features as they are (the reference scales those as well)
    features = features_scaler = None
    if a.features_path:
        features, features_scaler = scale_features(load_input_features(a.features_path, len(smiles)), train_idx,
                                                   a.no_features_scaling)
    if phase_features is not None:
        features = phase_features if features is None else np.concatenate([features, phase_features], axis=1)
    # --atom_descriptors descriptor: every molecule's [n_atoms][d] rows, standardised on the training split's
    # stacked rows (run_training.py:118-123)
    descriptors = atom_descriptor_scaler = atom_features = None
    if getattr(a, 'atom_descriptors', None) is not None:
        check_atom_descriptor_args(a.atom_descriptors, a.atom_descriptors_path)
        descriptors, atom_descriptor_scaler = scale_atom_descriptors(
            load_atom_descriptors(a.atom_descriptors_path, graphs), train_idx, a.no_atom_descriptor_scaling)
        if a.atom_descriptors == 'feature':  # columns of the atom rows, not rows for the descriptor layer
            atom_features, descriptors = descriptors, None
    # --bond_features_path: every molecule's [n_bonds / 2][db] rows, standardised the same way
    # (run_training.py:124-128); the scaled extras are joined to the graphs once, here
    bond_features = bond_feature_scaler = None
    bond_features_path = getattr(a, 'bond_features_path', None)
    if bond_features_path is not None:
        check_bond_features_args(bond_features_path)
        bond_features, bond_feature_scaler = scale_atom_descriptors(
            load_bond_features(bond_features_path, graphs), train_idx,
            bool(getattr(a, 'no_bond_features_scaling', False)))
    if atom_features is not None or bond_features is not None:
        graphs = join_extra_features(graphs, atom_features, bond_features)
    args = TrainArgs(hidden_size=a.hidden_size, depth=a.depth, dropout=a.dropout, activation=a.activation,
                     aggregation=a.aggregation, aggregation_norm=a.aggregation_norm, bias=a.bias,
                     undirected=a.undirected, atom_messages=bool(getattr(a, 'atom_messages', False)),
                     ffn_num_layers=a.ffn_num_layers,
                     ffn_hidden_size=a.ffn_hidden_size or a.hidden_size, dataset_type=a.dataset_type,
                     num_tasks=num_tasks, multiclass_num_classes=a.multiclass_num_classes, device=device,
                     frzn_encoder=bool(a.frzn_encoder or a.frzn_ffn_layers > 0), frzn_ffn_layers=a.frzn_ffn_layers,
                     init_lr=a.init_lr, optimizer=a.optimizer, weight_decay=a.weight_decay,
                     spectra_activation=a.spectra_activation, spectra_target_floor=a.spectra_target_floor,
                     alternative_loss_function=a.alternative_loss_function,
                     spectra_phase_mask_path=a.spectra_phase_mask_path, phase_features_path=a.phase_features_path,
                     features_path=list(a.features_path) if a.features_path else None,
                     no_features_scaling=bool(a.no_features_scaling),
                     use_input_features=features is not None,
                     features_size=0 if features is None else int(features.shape[1]),
                     atom_descriptors='feature' if atom_features is not None else
                     None if descriptors is None else 'descriptor',
                     atom_descriptors_size=0 if descriptors is None else int(descriptors[0].shape[1]),
                     atom_descriptors_path=None if descriptors is None and atom_features is None
                     else a.atom_descriptors_path,
                     no_atom_descriptor_scaling=bool(getattr(a, 'no_atom_descriptor_scaling', False)),
                     atom_features_size=0 if atom_features is None else int(atom_features[0].shape[1]),
                     bond_features_size=0 if bond_features is None else int(bond_features[0].shape[1]),
                     bond_features_path=bond_features_path,
                     no_bond_features_scaling=bool(getattr(a, 'no_bond_features_scaling', False)),
                     polymer=bool(a.polymer), ensemble_size=a.ensemble_size, task_names=list(header[n_mols:]),
                     number_of_molecules=n_mols, mpn_shared=mpn_shared,
                     device_metrics=bool(getattr(a, 'device_metrics', False)))
    set_feature_sizes(args)  # (MPN takes its row widths from get_atom_fdim / get_bond_fdim)
    torch.manual_seed(a.pytorch_seed)
    scaler = None
    train_targets = [targets[i] for i in train_idx]
    if a.dataset_type == 'regression':
        scaler = StandardScaler().fit(train_targets)
        train_targets = scaler.transform(train_targets).tolist()
        train_targets = [[None if (x is None or (isinstance(x, float) and math.isnan(x))) else x for x in r]
                         for r in train_targets]
    if spectra:  # one float array (NaN = missing): a batch's rows are a slice, not 1801 Python objects per row
        train_targets = np.array([[np.nan if x is None else x for x in r] for r in train_targets], dtype=np.float64)
        train_targets = train_targets.reshape(len(train_idx), num_tasks)
    # one resident feature table per split, in split order: a batch is a slice of an index into it
    splits = (('train', train_idx), ('val', val_idx), ('test', test_idx))
    tables = None if features is None else {name: FeatureTable(features[idx], device) if len(idx) else None
                                            for name, idx in splits}
    # and one resident atom descriptor table per split: a batch is a slice of an index of its molecules
    desc_tables = None if descriptors is None else {
        name: AtomDescriptorTable([descriptors[i] for i in idx], device) if len(idx) else None for name, idx in splits}
    loss_func = get_loss_func(a.dataset_type, a.alternative_loss_function)

    def save(path, model):
        save_checkpoint(path, model, scaler, features_scaler, args, atom_descriptor_scaler, bond_feature_scaler)

    def batch_targets(pos):
        return train_targets[pos] if spectra else [train_targets[p] for p in pos]

    # --resident_graphs: the training split's graphs go to the device once per run as compact codes (built on
    # first use: a run on cached encodings never needs them; epochs and ensemble members share the table), and
    # the scoring batches of every split are built once per run instead of once per epoch
    resident = bool(getattr(a, 'resident_graphs', False))
    resident_state = {}
    scoring_batches = {}

    def graph_table():
        """The training split's ``GraphTable``, or None when it refuses the split (logged once; the run then
        continues on the list path)."""
        if 'table' not in resident_state:
            try:
                resident_state['table'] = GraphTable([graphs[i] for i in train_idx], device)
            except ValueError as e:
                resident_state['table'] = None
                print(f'--resident_graphs: the training graphs stay on the list path ({e})', flush=True)
        return resident_state['table']

    def batches_of(name, idx):
        if not resident:
            return None
        if name not in scoring_batches:
            scoring_batches[name] = make_batches([graphs[i] for i in idx], a.batch_size, shared=mpn_shared)
        return scoring_batches[name]

    def run_predict(model, enc_cache, name, idx):
        return predict(model, graphs, idx, a.batch_size, scaler, enc_cache and enc_cache[name],
                       tables and tables[name], None if row_mask is None else row_mask[idx],
                       atom_descriptors=desc_tables and desc_tables[name],
                       batches=None if enc_cache is not None or not len(idx) else batches_of(name, idx))
    # --device_metrics: every split's target table and phase mask go to the device once per run, its
    # BatchMolGraphs are built once (on first use: a run on cached encodings never needs them), and a split is
    # scored by evaluate.evaluate without a host copy per batch
    device_metrics = bool(getattr(a, 'device_metrics', False))
    if device_metrics:
        split_idx = dict(splits)
        split_targets = {name: TargetTable([targets[i] for i in idx], a.dataset_type, device,
                                           a.multiclass_num_classes, num_tasks=num_tasks) for name, idx in splits}
        split_masks = {name: device_mask(row_mask, device, idx) for name, idx in splits}
        split_batches = {}

    def score_on_device(model, enc_cache, name, keep=False):
        """(scores, evaluator) of ``model`` on the split ``name``; ``keep``: the evaluator holds the predictions."""
        table = split_targets[name]
        ev = Evaluator(table, metrics, a.dataset_type, scaler, keep=keep)
        if enc_cache is not None:
            batches = a.batch_size
        else:
            if name not in split_batches:
                split_batches[name] = batches_of(name, split_idx[name]) or \
                    make_batches([graphs[i] for i in split_idx[name]], a.batch_size, shared=mpn_shared)
            batches = split_batches[name]
        return evaluate(model, batches, table, metrics, scaler, tables and tables[name], split_masks[name],
                        enc_cache and enc_cache[name], evaluator=ev,
                        atom_descriptors=desc_tables and desc_tables[name]), ev
    sampler = Random(a.seed)  # (one stream of shuffles for the run: an ensemble's later models continue it)

    def train_model(save_dir):
        """One model, trained into ``save_dir`` (``model.pt``, ``best_model.pt``, ``train_val_loss_log.csv``):
        (the model with its best weights, its cached encodings or None, the best epoch)."""
        model = MoleculeModel(args)
        initialize_weights(model)
        if a.checkpoint_frzn is not None:
            load_frzn_checkpoint(model, a.checkpoint_frzn)
        apply_freezing(model, a.frzn_encoder, a.frzn_ffn_layers)
        model = model.to(device)
        optimizer = build_optimizer(model, args)
        # a frozen encoder without dropout gives every molecule the same encoding at every step: computed once
        # per split, the steps and the per-epoch scores then run the head alone (train.frozen_encodings)
        enc_cache = None
        if args.frzn_encoder and a.dropout == 0 and not a.no_encoding_cache and descriptors is None and \
                n_mols == 1 and \
                _predict_head(model.eval()) is not None:
            enc_cache = {name: frozen_encodings(model, [graphs[i] for i in idx], a.batch_size)
                         for name, idx in splits}
        scheduler = NoamLR(optimizer, warmup_epochs=[a.warmup_epochs], total_epochs=[a.epochs],
                           steps_per_epoch=len(train_idx) // a.batch_size, init_lr=[a.init_lr], max_lr=[a.max_lr],
                           final_lr=[a.final_lr])
        log_path = os.path.join(save_dir, 'train_val_loss_log.csv')
        best = math.inf if minimize else -math.inf
        best_epoch = 0
        with open(log_path, 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(['epoch', 'train_loss'] + [f'train_avg_{m}' for m in metrics] +
                       [f'val_avg_{m}' for m in metrics])
            for epoch in range(a.epochs):
                order = list(range(len(train_idx)))
                sampler.shuffle(order)
                losses = []
                # the epoch's order as one validated index upload; every step takes a slice of it
                findex = tables['train'].index(order) if tables is not None and order else None
                dindex = desc_tables['train'].index(order) if desc_tables is not None and order else None
                gtable = graph_table() if resident and enc_cache is None and order else None
                gindex = None if gtable is None else gtable.index(order)
                for s in range(0, len(order), a.batch_size):
                    pos = order[s:s + a.batch_size]
                    feats = None if findex is None else findex[s:s + a.batch_size]
                    if enc_cache is not None:
                        rows = enc_cache['train'][torch.as_tensor(pos, device=device)]
                        loss = train_step(model, None, batch_targets(pos), loss_func, optimizer, scheduler,
                                          a.dataset_type, features_batch=feats, grad_clip=a.grad_clip,
                                          encodings=rows)
                    else:
                        if gindex is not None:  # (the step's graphs: a slice of the epoch's index)
                            rows = gindex[s:s + a.batch_size]
                            g = [rows.batch()] if n_mols == 1 else rows.slot_batch(shared=mpn_shared)
                        elif n_mols == 1:
                            g = [BatchMolGraph([graphs[train_idx[p]] for p in pos])]
                        else:  # (one BatchMolGraph per slot, and the merged one for a shared encoder)
                            g = SlotBatch([[graphs[train_idx[p]][k] for p in pos] for k in range(n_mols)],
                                          shared=mpn_shared)
                        loss = train_step(model, g, batch_targets(pos), loss_func, optimizer, scheduler,
                                          a.dataset_type, features_batch=feats, grad_clip=a.grad_clip,
                                          atom_descriptors_batch=None if dindex is None else
                                          dindex[s:s + a.batch_size])
                    losses.append(float(loss))
                if device_metrics:
                    val_scores = score_on_device(model, enc_cache, 'val')[0]
                    tr_scores = score_on_device(model, enc_cache, 'train')[0]
                else:
                    val_scores = evaluate_predictions(run_predict(model, enc_cache, 'val', val_idx),
                                                      [targets[i] for i in val_idx], num_tasks, metrics,
                                                      a.dataset_type)
                    tr_scores = evaluate_predictions(run_predict(model, enc_cache, 'train', train_idx),
                                                     [targets[i] for i in train_idx], num_tasks, metrics,
                                                     a.dataset_type)
                w.writerow([epoch, float(np.mean(losses)) if losses else float('nan')] +
                           [float(np.nanmean(tr_scores[m])) if tr_scores[m] else float('nan') for m in metrics] +
                           [float(np.nanmean(val_scores[m])) if val_scores[m] else float('nan') for m in metrics])
                save(os.path.join(save_dir, 'model.pt'), model)
                v = float(np.nanmean(val_scores[metric])) if val_scores[metric] else float('nan')
                if (minimize and v < best) or (not minimize and v > best) or (epoch == 0 and math.isnan(v)):
                    best, best_epoch = v, epoch
                    save(os.path.join(save_dir, 'best_model.pt'), model)
        ckpt = torch.load(os.path.join(save_dir, 'best_model.pt'), map_location=device, weights_only=True)
        model.load_state_dict(ckpt['state_dict'])
        return model, enc_cache, best_epoch

    test_targets = [targets[i] for i in test_idx]
    device_scores = None
    if a.ensemble_size == 1:
        model, enc_cache, best_epoch = train_model(a.save_dir)
        if device_metrics:  # the scores from the device; the written predictions from one copy of the kept ones
            device_scores, ev = score_on_device(model, enc_cache, 'test', keep=True)
            test_preds = prediction_rows(ev.predictions().cpu().numpy(), a.dataset_type,
                                         a.multiclass_num_classes) if len(test_idx) else []
        else:
            test_preds = run_predict(model, enc_cache, 'test', test_idx)
    else:
        # run_training.py:208-499: model k trains into save_dir/model_k; every model's test predictions are folded
        # into one accumulator on the device, and the top-level scores and predictions are the ensemble's
        width = num_tasks * (a.multiclass_num_classes if multiclass else 1)
        acc = EnsembleAccumulator(len(test_idx), width, device, keep=True, n_models=a.ensemble_size)
        test_batches = batches_of('test', test_idx) or \
            make_batches([graphs[i] for i in test_idx], a.batch_size, shared=mpn_shared)
        test_mask = device_mask(row_mask, device, test_idx)
        best_epoch = []
        for k in range(a.ensemble_size):
            model_dir = os.path.join(a.save_dir, f'model_{k}')
            os.makedirs(model_dir, exist_ok=True)
            model, _, epoch = train_model(model_dir)
            best_epoch.append(epoch)
            if len(test_idx):
                accumulate_model(acc, k, model, test_batches, scaler, tables and tables['test'], test_mask,
                                 atom_descriptors=desc_tables and desc_tables['test'])
            del model
        each = acc.individual().cpu().numpy() if len(test_idx) else np.zeros((a.ensemble_size, 0, width))
        mean = acc.mean().cpu().numpy() if len(test_idx) else np.zeros((0, width))
        for k in range(a.ensemble_size):  # each model's own scores (run_training.py:440-469)
            own = evaluate_predictions(prediction_rows(each[k], a.dataset_type, a.multiclass_num_classes),
                                       test_targets, num_tasks, metrics, a.dataset_type)
            with open(os.path.join(a.save_dir, f'model_{k}', 'test_scores.json'), 'w') as f:
                json.dump(own, f, indent=4, sort_keys=True)
        test_preds = prediction_rows(mean, a.dataset_type, a.multiclass_num_classes)
    scores = device_scores if device_scores is not None else \
        evaluate_predictions(test_preds, test_targets, num_tasks, metrics, a.dataset_type)
    with open(os.path.join(a.save_dir, 'test_scores.json'), 'w') as f:
        json.dump(scores, f, indent=4, sort_keys=True)
    with open(os.path.join(a.save_dir, 'test_scores.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['Task'] + [f'Mean {m}' for m in metrics])
        for t, name in enumerate(['spectra'] if spectra else header[n_mols:]):  # (cross_validate.py:158-159)
            w.writerow([name] + [scores[m][t] if t < len(scores[m]) else '' for m in metrics])
    with open(os.path.join(a.save_dir, 'test_preds.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        if multiclass:  # one column per class (make_predictions.py:213)
            w.writerow(header[:n_mols] + [f'{name}_class_{k}' for name in header[n_mols:]
                                          for k in range(a.multiclass_num_classes)])
        else:
            w.writerow(header)
        for i, p in zip(test_idx, test_preds):
            w.writerow(smiles_rows[i] + ([x for task in p for x in task] if multiclass else
                                         ['' if x is None else x for x in p]))
    with open(os.path.join(a.save_dir, 'split_indices.json'), 'w') as f:
        json.dump({'train': train_idx, 'val': val_idx, 'test': test_idx, 'best_epoch': best_epoch}, f)
    return scores


def prediction_rows(preds: np.ndarray, dataset_type: str, num_classes: int = 1) -> list:
    """A float64 ``[N][W]`` array of predictions as the rows ``predict`` returns: lists of floats, multiclass as
    ``[tasks][classes]`` per row, a spectrum's excluded (NaN) positions as None."""
    preds = np.asarray(preds, dtype=np.float64)
    if dataset_type == 'multiclass':
        return preds.reshape(len(preds), -1, num_classes).tolist()
    if dataset_type == 'spectra':
        return [[None if math.isnan(v) else v for v in row] for row in preds.tolist()]
    return preds.tolist()


def chemprop_train(argv=None) -> Dict[str, list]:
    """Entry point (setup.py:39 ``chemprop_train`` in the reference)."""
    return run_training(parse_args(argv, spectra=True))


def _prediction_parser(prog: str, description: str) -> argparse.ArgumentParser:
    """The arguments ``chemprop_predict`` and ``chemprop_fingerprint`` share (args.py PredictArgs)."""
    ap = argparse.ArgumentParser(prog=prog, description=description)
    ap.add_argument('--test_path', required=True, help='CSV with a header; the first column holds the SMILES')
    ap.add_argument('--graphs_path', required=True, help='pre-featurised MolGraph records, one per CSV row')
    ap.add_argument('--extra_graphs_path', nargs='+', default=None,
                    help='the graph files of molecules 2 .. N for checkpoints trained with --number_of_molecules N')
    ap.add_argument('--preds_path', required=True, help='the CSV to write')
    ap.add_argument('--checkpoint_dir', default=None,
                    help='every best_model.pt below this directory if there is one, else every .pt file')
    ap.add_argument('--checkpoint_path', default=None)
    ap.add_argument('--checkpoint_paths', nargs='+', default=None)
    ap.add_argument('--features_path', nargs='+', default=None,
                    help='the molecule features the models were trained with, one row per CSV row')
    ap.add_argument('--phase_features_path', default=None)
    ap.add_argument('--no_features_scaling', action='store_true',
                    help='feed the features as they are instead of through each checkpoint\'s features scaler')
    ap.add_argument('--atom_descriptors_path', default=None,
                    help='.npz file of the atom descriptors the models were trained with (one [n_atoms][d] array '
                         'per CSV row); the mode, the width and the scaler come from each checkpoint')
    ap.add_argument('--bond_features_path', default=None,
                    help='.npz file of the extra bond features the models were trained with (one [n_bonds / 2][d] '
                         'array per CSV row); the width and the scaler come from each checkpoint')
    ap.add_argument('--batch_size', type=int, default=50)
    ap.add_argument('--gpu', type=int, default=0)
    return ap


def _check_prediction_args(a: argparse.Namespace) -> argparse.Namespace:
    given = [x is not None for x in (a.checkpoint_dir, a.checkpoint_path, a.checkpoint_paths)]
    if sum(given) != 1:
        raise ValueError('give exactly one of --checkpoint_dir, --checkpoint_path and --checkpoint_paths')
    if a.batch_size < 1:
        raise ValueError('--batch_size must be at least 1')
    if a.atom_descriptors_path is not None:
        check_atom_descriptors_path(a.atom_descriptors_path)
    if a.bond_features_path is not None:
        check_atom_descriptors_path(a.bond_features_path)
    return a


def parse_predict_args(argv=None) -> argparse.Namespace:
    """The arguments of ``chemprop_predict`` (args.py PredictArgs).  Exactly one of ``--checkpoint_dir``,
    ``--checkpoint_path`` and ``--checkpoint_paths`` names the models, and ``--save_graph_embeddings`` comes with
    ``--graph_embeddings_path`` (``ValueError`` otherwise)."""
    ap = _prediction_parser('chemprop_predict', 'Predictions of a checkpoint, or of an ensemble of checkpoints.')
    ap.add_argument('--ensemble_variance', action='store_true',
                    help='also write the spread of the ensemble: the variance per task, the pairwise SID for spectra')
    ap.add_argument('--individual_ensemble_predictions', action='store_true',
                    help='also write every model\'s own predictions')
    ap.add_argument('--drop_extra_columns', action='store_true',
                    help='keep only the SMILES column of the input next to the predictions')
    ap.add_argument('--save_graph_embeddings', action='store_true',
                    help='also save the ensemble-mean graph embeddings (the FFN input of every row), float32 .npy')
    ap.add_argument('--graph_embeddings_path', default=None, help='the .npy file --save_graph_embeddings writes')
    a = _check_prediction_args(ap.parse_args(argv))
    if a.save_graph_embeddings and not a.graph_embeddings_path:
        raise ValueError('--save_graph_embeddings needs --graph_embeddings_path')
    return a


def parse_fingerprint_args(argv=None) -> argparse.Namespace:
    """The arguments of ``chemprop_fingerprint`` (args.py FingerprintArgs): those the prediction run shares, and
    ``--fingerprint_type``."""
    ap = _prediction_parser('chemprop_fingerprint', 'Latent vectors of a checkpoint, or of every checkpoint of an '
                                                    'ensemble.')
    ap.add_argument('--fingerprint_type', choices=LATENT_TYPES, default='MPN',
                    help='MPN: the encoder\'s output without the molecule features; last_FFN: the input of the '
                         'FFN\'s last layer')
    return _check_prediction_args(ap.parse_args(argv))


def find_checkpoints(checkpoint_dir: str) -> List[str]:
    """``--checkpoint_dir``: every ``best_model.pt`` below the directory if there is one, else every ``*.pt``,
    sorted by path.  (The reference takes every ``.pt``, args.py:34-47; this package writes ``model.pt``, the last
    epoch, next to ``best_model.pt``, and an ensemble is made of the best ones.)  ``ValueError`` without any."""
    found = sorted(os.path.join(root, f) for root, _, files in os.walk(checkpoint_dir) for f in files
                   if f.endswith('.pt'))
    best = [p for p in found if os.path.basename(p) == 'best_model.pt']
    if not found:
        raise ValueError(f'no checkpoint (.pt file) below {checkpoint_dir}')
    return best or found


def checkpoint_paths_of(a: argparse.Namespace) -> List[str]:
    if a.checkpoint_dir is not None:
        return find_checkpoints(a.checkpoint_dir)
    return [a.checkpoint_path] if a.checkpoint_path is not None else list(a.checkpoint_paths)


def update_prediction_args(paths: List[str]) -> Dict[str, object]:
    """What the checkpoints decide about a prediction run (make_predictions.py ``update_prediction_args``): the
    first checkpoint's dataset type, task names (``task_0 ..`` when an older checkpoint holds none), class count,
    spectra phase-mask path and ``polymer``.  ``ValueError`` when a later checkpoint disagrees on the dataset type
    or the output width, or a file holds no ``args``."""
    out = None
    for k, path in enumerate(paths):
        state = torch.load(path, map_location='cpu', weights_only=True)
        if not isinstance(state, dict) or not isinstance(state.get('args'), dict):
            raise ValueError(f'{path} is not a checkpoint with its training args')
        t = state['args']
        dataset_type = t.get('dataset_type', 'regression')
        num_tasks = int(t.get('num_tasks', 1))
        classes = int(t.get('multiclass_num_classes', 3)) if dataset_type == 'multiclass' else 1
        if out is None:
            names = t.get('task_names')
            if not names or len(names) != num_tasks:
                names = [f'task_{i}' for i in range(num_tasks)]
            out = {'dataset_type': dataset_type, 'num_tasks': num_tasks, 'multiclass_num_classes': classes,
                   'task_names': list(names), 'spectra_phase_mask_path': t.get('spectra_phase_mask_path'),
                   'polymer': bool(t.get('polymer', False)), 'width': num_tasks * classes,
                   'number_of_molecules': int(t.get('number_of_molecules', 1)),
                   'mpn_shared': bool(t.get('mpn_shared', False))}
        elif dataset_type != out['dataset_type'] or num_tasks * classes != out['width']:
            raise ValueError(f'{path} ({dataset_type}, {num_tasks * classes} outputs) does not fit the ensemble\'s '
                             f'first checkpoint {paths[0]} ({out["dataset_type"]}, {out["width"]} outputs)')
    if out is None:
        raise ValueError('no checkpoint given')
    return out


def write_predictions(path: str, header: List[str], rows: List[List[str]], task_names: List[str], mean,
                      dataset_type: str = 'regression', num_classes: int = 1, spread=None, individual=None,
                      drop_extra_columns: bool = False, smiles_columns: int = 1) -> List[str]:
    """The predictions CSV (make_predictions.py:211-263); returns its header.  ``header`` / ``rows``: the input
    CSV; ``mean`` ``[N][W]``, ``spread`` ``[N][W]`` (spectra: the pairwise SID ``[N]``) or None, ``individual``
    ``[M][N][W]`` or None.  Columns: the input row's (``drop_extra_columns``: its first ``smiles_columns``, the SMILES), one per task
    (multiclass: ``<task>_class_<i>``), then ``<task>_model_<k>`` task by task, then ``<task>_epi_unc`` per task
    (spectra: one ``epi_unc``); a prediction column named like a kept input column (the target column of a
    training CSV) replaces it where it stands, as the reference's per-row dict does.  NaN cells (a spectrum's excluded positions) are written empty, as
    ``chemprop_train`` writes them in ``test_preds.csv``."""
    mean = np.asarray(mean, dtype=np.float64)
    mean = mean.reshape(len(mean), -1)
    names = [f'{t}_class_{i}' for t in task_names for i in range(num_classes)] if dataset_type == 'multiclass' \
        else list(task_names)
    if len(rows) != len(mean) or mean.shape[1] != len(names):
        raise ValueError(f'predictions of shape {mean.shape} for {len(rows)} rows and {len(names)} columns')
    spectra = dataset_type == 'spectra'
    if individual is not None:
        individual = np.asarray(individual, dtype=np.float64).reshape(-1, len(mean), len(names))
    if spread is not None:
        spread = np.asarray(spread, dtype=np.float64).reshape((len(mean),) if spectra else mean.shape)
    keep = smiles_columns if drop_extra_columns else len(header)
    added = list(names)
    if individual is not None:
        added += [f'{n}_model_{k}' for n in names for k in range(len(individual))]
    if spread is not None:
        added += ['epi_unc'] if spectra else [f'{n}_epi_unc' for n in names]
    # the reference fills a dict per row: a prediction column named like an input column takes its place
    out_header = list(header[:keep])
    slot = []
    for name in added:
        if name not in out_header:
            out_header.append(name)
        slot.append(out_header.index(name))

    def cells(values):
        return ['' if math.isnan(v) else v for v in values]
    parent = os.path.dirname(path)
    if parent:
        os.makedirs(parent, exist_ok=True)
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(out_header)
        for n, row in enumerate(rows):
            values = cells(mean[n].tolist())
            if individual is not None:
                values += cells(individual[:, n, :].T.reshape(-1).tolist())
            if spread is not None:
                values += cells([float(spread[n])] if spectra else spread[n].tolist())
            line = (list(row) + [''] * len(out_header))[:keep] + [''] * (len(out_header) - keep)
            for at, v in zip(slot, values):
                line[at] = v
            w.writerow(line)
    return out_header


def check_polymer_rows(smiles: List[str], graphs) -> None:
    """Every row a well-formed polymer string whose degree of polymerisation is its graph's (data.py:695-703,
    featurization.py:335-364)."""
    for s, g in zip(smiles, graphs):
        _, _, rules = split_polymer_string(s)
        if rules:
            _, deg = parse_polymer_rules(rules)
            if not np.isclose(deg, g.degree_of_polym, rtol=1e-6):
                raise ValueError(f'graph degree_of_polym {g.degree_of_polym} != 1 + log10(Xn) = {deg} for {s}')


def _prediction_graphs(a: argparse.Namespace, info: Dict[str, object], header: List[str], rows: List[List[str]]):
    """The graphs of a prediction run's rows (``load_molecule_graphs``): the checkpoints' ``number_of_molecules``
    decides how many SMILES columns the CSV needs and how many ``--extra_graphs_path`` files."""
    n_mols = int(info['number_of_molecules'])
    check_number_of_molecules(n_mols, getattr(a, 'extra_graphs_path', None))
    if len(header) < n_mols:
        raise ValueError(f'{a.test_path} has {len(header)} columns for checkpoints of {n_mols} molecules per row')
    return load_molecule_graphs(a.graphs_path, getattr(a, 'extra_graphs_path', None), len(rows),
                                [r[:n_mols] for r in rows], bool(info['polymer']))


def _prediction_descriptors(a: argparse.Namespace, paths: List[str], graphs) -> Dict[str, object]:
    """The raw per-atom / per-bond inputs of a prediction run as keyword arguments of ``predict_ensemble`` /
    ``molecule_fingerprint``: ``atom_descriptors`` (checkpoints trained with ``--atom_descriptors descriptor``),
    ``atom_features`` (``feature``) and ``bond_features`` (``--bond_features_path``), each None when the checkpoints
    were trained without.  A file must be given exactly when they were trained with it (their stored args say)."""
    state = torch.load(paths[0], map_location='cpu', weights_only=True)
    mode = state['args'].get('atom_descriptors')
    path = getattr(a, 'atom_descriptors_path', None)
    out = {'atom_descriptors': None, 'atom_features': None, 'bond_features': None}
    if mode is None:
        if path is not None:
            raise ValueError(f'{paths[0]} was trained without atom descriptors, but --atom_descriptors_path is given')
    elif path is None:
        raise ValueError(f'{paths[0]} was trained with --atom_descriptors {mode}: give --atom_descriptors_path')
    else:
        out['atom_features' if mode == 'feature' else 'atom_descriptors'] = load_atom_descriptors(path, graphs)
    trained = state['args'].get('bond_features_path') is not None or int(state['args'].get('bond_features_size') or 0)
    bpath = getattr(a, 'bond_features_path', None)
    if not trained:
        if bpath is not None:
            raise ValueError(f'{paths[0]} was trained without extra bond features, but --bond_features_path is given')
    elif bpath is None:
        raise ValueError(f'{paths[0]} was trained with --bond_features_path: give --bond_features_path')
    else:
        out['bond_features'] = load_bond_features(bpath, graphs)
    out['bond_feature_scaling'] = not bool(state['args'].get('no_bond_features_scaling', False))
    return out


def _descriptor_scaling_of(paths: List[str]) -> bool:
    """Whether the run's checkpoints scale their atom descriptors (the first one's stored flag, as
    make_predictions.py:143-153 reads ``train_args.atom_descriptor_scaling``)."""
    state = torch.load(paths[0], map_location='cpu', weights_only=True)
    return not bool(state['args'].get('no_atom_descriptor_scaling', False))


def make_predictions(a: argparse.Namespace):
    """make_predictions.py:272-372 for this package's checkpoints: the ensemble's predictions of ``--test_path``
    written to ``--preds_path``; returns the mean predictions ``[N][W]`` (float64)."""
    save_embeddings = bool(getattr(a, 'save_graph_embeddings', False))
    if save_embeddings and not getattr(a, 'graph_embeddings_path', None):  # (before anything is loaded)
        raise ValueError('--save_graph_embeddings needs --graph_embeddings_path')
    paths = checkpoint_paths_of(a)
    if len(paths) > ENSEMBLE_MAX_MODELS:
        raise ValueError(f'{len(paths)} checkpoints (an ensemble holds at most {ENSEMBLE_MAX_MODELS})')
    info = update_prediction_args(paths)
    with open(a.test_path) as f:
        table = list(csv.reader(f))
    header, rows = table[0], [r for r in table[1:] if r]
    graphs = _prediction_graphs(a, info, header, rows)
    features = load_input_features(a.features_path, len(rows)) if a.features_path else None
    phase_features = phase_mask = None
    if a.phase_features_path is not None:
        phase_features = load_phase_features(a.phase_features_path, len(rows))
    if info['dataset_type'] == 'spectra' and info['spectra_phase_mask_path'] is not None:
        phase_mask = load_phase_mask(info['spectra_phase_mask_path'])
    mean, spread, individual, *embeddings = predict_ensemble(
        paths, graphs, a.batch_size, features=features, phase_features=phase_features, phase_mask=phase_mask,
        variance=a.ensemble_variance, individual=a.individual_ensemble_predictions,
        device=torch.device('cuda', a.gpu), features_scaling=not a.no_features_scaling, embeddings=save_embeddings,
        atom_descriptor_scaling=_descriptor_scaling_of(paths), **_prediction_descriptors(a, paths, graphs))
    if save_embeddings:  # (make_predictions.py:191-195: averaged across the ensemble, next to the predictions)
        parent = os.path.dirname(a.graph_embeddings_path)
        if parent:
            os.makedirs(parent, exist_ok=True)
        np.save(a.graph_embeddings_path, embeddings[0])
    write_predictions(a.preds_path, header, rows, info['task_names'], mean, info['dataset_type'],
                      info['multiclass_num_classes'], spread, individual, a.drop_extra_columns,
                      smiles_columns=info['number_of_molecules'])
    return mean


def chemprop_predict(argv=None):
    """Entry point (setup.py:40 ``chemprop_predict`` in the reference)."""
    return make_predictions(parse_predict_args(argv))


def write_fingerprints(path: str, smiles_header: str, smiles: List[str], fingerprints: np.ndarray) -> List[str]:
    """The fingerprint CSV (molecule_fingerprint.py:124-147); returns its header: the SMILES column, then ``fp_j``
    for one model, ``fp_j_model_i`` (j outer, i inner) for several.  ``fingerprints``: float64 ``[N][fp][M]``; every
    value is written as ``str()`` of the float64, as ``csv.DictWriter`` writes the reference's."""
    from .fingerprint import fingerprint_columns
    fp = np.asarray(fingerprints, dtype=np.float64)
    if fp.ndim != 3 or len(fp) != len(smiles):
        raise ValueError(f'fingerprints of shape {fp.shape} for {len(smiles)} rows ([N][fp][M] expected)')
    several = isinstance(smiles_header, (list, tuple))  # (rows of several molecules: every SMILES column in front)
    header = (list(smiles_header) if several else [smiles_header]) + fingerprint_columns(fp.shape[1], fp.shape[2])
    parent = os.path.dirname(path)
    if parent:
        os.makedirs(parent, exist_ok=True)
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(header)
        for s, row in zip(smiles, fp.reshape(len(fp), -1)):
            w.writerow((list(s) if several else [s]) + [str(v) for v in row])
    return header


def make_fingerprints(a: argparse.Namespace) -> np.ndarray:
    """molecule_fingerprint.py:16-149 for this package's checkpoints: the latent vectors of ``--test_path`` under
    every checkpoint, written to ``--preds_path``; returns them, float64 ``[N][fp][M]``."""
    from .fingerprint import molecule_fingerprint
    paths = checkpoint_paths_of(a)
    if len(paths) > ENSEMBLE_MAX_MODELS:
        raise ValueError(f'{len(paths)} checkpoints (an ensemble holds at most {ENSEMBLE_MAX_MODELS})')
    info = update_prediction_args(paths)
    with open(a.test_path) as f:
        table = list(csv.reader(f))
    header, rows = table[0], [r for r in table[1:] if r]
    graphs = _prediction_graphs(a, info, header, rows)
    features = load_input_features(a.features_path, len(rows)) if a.features_path else None
    phase_features = None
    if a.phase_features_path is not None:
        phase_features = load_phase_features(a.phase_features_path, len(rows))
    fp = molecule_fingerprint(paths, graphs, a.batch_size, a.fingerprint_type, features=features,
                              phase_features=phase_features, features_scaling=not a.no_features_scaling,
                              device=torch.device('cuda', a.gpu),
                              atom_descriptor_scaling=_descriptor_scaling_of(paths),
                              **_prediction_descriptors(a, paths, graphs))
    n_mols = info['number_of_molecules']
    write_fingerprints(a.preds_path, header[0] if n_mols == 1 else header[:n_mols],
                       [r[0] if n_mols == 1 else list(r[:n_mols]) for r in rows], fp)
    return fp


def chemprop_fingerprint(argv=None) -> np.ndarray:
    """Entry point (setup.py ``chemprop_fingerprint`` in the reference)."""
    return make_fingerprints(parse_fingerprint_args(argv))


if __name__ == '__main__':
    if sys.argv[1:2] == ['predict']:  # python -m chemprop_amd.cli predict --test_path ...
        chemprop_predict(sys.argv[2:])
    elif sys.argv[1:2] == ['fingerprint']:  # python -m chemprop_amd.cli fingerprint --test_path ...
        chemprop_fingerprint(sys.argv[2:])
    else:
        print(json.dumps(chemprop_train(sys.argv[1:])))
