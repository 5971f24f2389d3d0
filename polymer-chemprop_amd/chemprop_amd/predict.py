"""The one loop that walks a split for prediction, and what its sinks share.

``device_predictions`` yields every batch's predictions where the head wrote them: the batches in groups of eight
through ``MPNEncoder.forward_many`` (or the split's cached ``train.frozen_encodings``), ``join_features`` for a
model with input features, the native prediction head; no host sync.  Its callers differ in where a batch goes:
``cli.predict`` copies it to the host, ``ensemble.accumulate_model`` hands it to a ``PredictionSink`` -- the
``EnsembleAccumulator`` of an ensemble, or the ``Evaluator`` of ``evaluate.evaluate``.  The same loop yields a
model's latent vectors instead (``latent``), or the FFN input next to the predictions (``with_encodings``), for the
``fingerprint.LatentAccumulator`` of ``fingerprint.molecule_fingerprint`` and of ``predict_ensemble(embeddings=True)``.
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from .atom_descriptors import AtomDescriptorTable
from ._native import MAX_SLOTS
from .features import FeatureTable, join_features
from .slots import join_slots, merged_graph


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


def _fallback_predict(model, batch, feats, mask, return_embeddings: bool = False, desc=None):
    """A model whose FFN the native prediction heads refuse: its own forward (a spectra model's output
    normalised per row with torch ops, as ``head_predict(normalize=True)`` does it natively).
    ``return_embeddings``: (predictions, the FFN input), as the model's forward returns them."""
    if return_embeddings:
        out, emb = model(_molecules(batch), feats, desc, return_embeddings=True)
    else:
        out, emb = model(_molecules(batch), feats, desc), None
    if getattr(model, 'spectra', False):
        m = torch.ones_like(out, dtype=torch.bool) if mask is None else mask.bool()
        s = torch.where(m, out, torch.zeros_like(out))
        out = torch.where(m, s / s.sum(dim=1, keepdim=True), torch.full_like(out, float('nan')))
    return (out, emb) if return_embeddings else out


def _molecules(batch) -> list:
    """A batch as ``MPN.forward`` takes it: one ``BatchMolGraph`` per molecule of the model's input (a batch given
    as a single ``BatchMolGraph`` is a model of one molecule's)."""
    return list(batch) if isinstance(batch, (list, tuple)) else [batch]


def _encode_alone(mpn, batch) -> torch.Tensor:
    """The encoders' output without the input features the model was trained with (molecule_fingerprint.py:30-34:
    the ``MPN`` fingerprint needs none)."""
    if mpn.features_only or mpn.atom_descriptors is not None:
        raise NotImplementedError('the MPN representation without input features: a features_only model has none, '
                                  'and atom descriptors are not supported here')
    return torch.cat([enc(ba) for enc, ba in zip(mpn.encoder, _molecules(batch))], dim=1)


def _encode_slots(mpn, group) -> list:
    """The encodings of a group of batches of a model of N molecules per input, per batch the list ``join_slots``
    takes.  Distinct encoders: one ``forward_many`` per slot encoder over that slot's graphs of the group.  A
    shared encoder: one ``forward_many`` over the batches' merged graphs (``slots.SlotBatch(shared=True)``: per
    batch one slot-major ``[N B][H]`` tensor), or over the flattened slot graphs of plain lists."""
    n = len(mpn.encoder)
    mols = [_molecules(b) for b in group]
    if any(len(m) != n for m in mols):
        raise ValueError(f'a batch of {[len(m) for m in mols]} molecule graphs for a model of {n} molecules per input')
    enc = mpn.encoder[0]
    if all(e is enc for e in mpn.encoder):
        merged = [merged_graph(b) for b in group]
        if all(g is not None for g in merged):
            return [[o] for o in enc.forward_many(merged)]
        outs = enc.forward_many([g for m in mols for g in m])
        return [[o.contiguous() for o in outs[k * n:(k + 1) * n]] for k in range(len(mols))]
    per_slot = [mpn.encoder[k].forward_many([m[k] for m in mols]) for k in range(n)]
    return [[per_slot[k][j].contiguous() for k in range(n)] for j in range(len(mols))]


LATENT_TYPES = ('MPN', 'last_FFN')


@torch.no_grad()
def device_predictions(model, batches, features: Optional[FeatureTable] = None,
                       row_mask: Optional[torch.Tensor] = None, encodings: Optional[torch.Tensor] = None,
                       own_forward: bool = False, n_rows: Optional[int] = None, latent: Optional[str] = None,
                       with_encodings: bool = False,
                       atom_descriptors: Optional[AtomDescriptorTable] = None) -> Iterator[Tuple]:
    """``(row0, predictions)`` of ``model`` for every ``BatchMolGraph`` of ``batches`` (row order = batch order):
    eval mode, ``no_grad``, float32 on the device, no host sync.  ``features``: the model's input features of
    every row, as the model sees them; ``row_mask``: a spectra model's included positions, bool or uint8
    ``[rows][T]`` on the device (ignored for other models): its predictions are normalised per row, the excluded
    positions NaN.  The batches run in groups of up to eight through ``forward_many``, then per batch
    ``join_features`` and the native prediction head; a model whose FFN the native heads refuse runs its own
    forward (``_fallback_predict``).  A batch of a model of several molecules is the list of its ``BatchMolGraph`` s
    (or a ``slots.SlotBatch``): per group one ``forward_many`` per slot encoder (a shared encoder: one, over the
    batches' merged graphs or the flattened slot graphs), then per batch one ``wdmpnn_slots_join`` launch builds the
    FFN input from every slot's encoding and the feature rows.

    ``encodings``: the rows' cached ``train.frozen_encodings``; the head runs straight from them, in the batch
    sizes of ``batches`` (which may then be a plain batch size as well; ``NotImplementedError`` without a native
    head).  ``own_forward``: every batch through ``model([batch], feats)`` and nothing else.  ``n_rows``: the rows
    the caller expects.  Molecules, feature rows and encodings that do not cover the same rows, or features for a
    model that takes none (or the reverse), are a ``ValueError`` before anything is launched.

    ``latent``: yield ``(row0, vectors)``, the model's representation (model.py:123-150) instead of its
    predictions.  ``'MPN'``: the FFN's input, the encoding with the features joined, and no prediction head runs;
    the features may then be left out for a model trained with them, and the encoders alone run.  ``'last_FFN'``:
    ``train.head_latent`` of that input, ``[B][ffn_hidden_size]`` (``MoleculeModel.fingerprint``'s torch slice for an
    FFN the native stack does not run).  ``with_encodings``: yield ``(row0, predictions, x)``, ``x`` being the FFN
    input the same pass holds, as ``model.encoder(...)`` returns it.

    ``atom_descriptors``: the table of every row's (scaled) atom descriptors, for a model with
    ``atom_descriptors='descriptor'``, molecule k of the table being row k.  The encodings still come from
    ``forward_many`` (the encoder runs as for a model without descriptors); per batch one join and one layer launch
    apply ``atom_descriptors_layer`` after the readout (``MPNEncoder.apply_descriptor_layer``).  A descriptor
    model given no table, or a table given to a model without the layer, is a ``ValueError``; so are cached
    ``encodings`` with descriptors."""
    # (here: importing the package does not import the training code)
    from .train import NO_LATENT_LAYER, _head_linears, _predict_head, head_latent, head_predict
    model.eval()
    mpn = model.encoder
    if latent is not None and latent not in LATENT_TYPES:
        raise ValueError(f'Fingerprint type {latent} not supported')
    if latent is not None and (with_encodings or own_forward):
        raise ValueError('latent vectors come instead of predictions: no with_encodings, no own_forward')
    if with_encodings and own_forward:
        raise ValueError('own_forward yields the model\'s output alone: no with_encodings')
    if isinstance(batches, int):
        if batches < 1 or encodings is None:
            raise ValueError('a plain batch size must be at least 1 and needs encodings')
        sizes = [min(batches, len(encodings) - s) for s in range(0, len(encodings), batches)]
    else:
        sizes = [len(_molecules(b)[0].a_scope) for b in batches]
    starts = np.cumsum([0] + sizes).tolist()
    n = starts[-1] if n_rows is None else n_rows
    if starts[-1] != n or (features is not None and len(features) != n) or \
            (encodings is not None and len(encodings) != n):
        raise ValueError(f'{starts[-1]} molecules, {None if features is None else len(features)} feature rows and '
                         f'{None if encodings is None else len(encodings)} encodings for {n} rows')
    needs = bool(getattr(mpn, 'use_input_features', False))
    alone = latent == 'MPN' and needs and features is None  # (the encoders without the features)
    if needs != (features is not None) and not alone:
        raise ValueError('the model takes input features and none were given' if needs else
                         'the model takes no input features, but features were given')
    if own_forward and encodings is not None:
        raise ValueError('own_forward runs the encoder: it takes no encodings')
    wants_desc = getattr(mpn, 'atom_descriptors', None) == 'descriptor' and not mpn.features_only
    if wants_desc != (atom_descriptors is not None) and not (alone and wants_desc):
        raise ValueError('the model takes atom descriptors and none were given' if wants_desc else
                         'the model takes no atom descriptors, but atom descriptors were given')
    if atom_descriptors is not None:
        if not isinstance(atom_descriptors, AtomDescriptorTable):
            raise ValueError('atom_descriptors: an atom_descriptors.AtomDescriptorTable of the rows is expected')
        if len(atom_descriptors) != n:
            raise ValueError(f'{len(atom_descriptors)} molecules in the atom descriptor table for {n} rows')
        if encodings is not None:
            raise ValueError('cached encodings hold no atom descriptors: a descriptor model runs its encoder')
    head = None if own_forward else _predict_head(model)
    spectra = bool(getattr(model, 'spectra', False))
    if latent == 'last_FFN':
        if spectra:
            raise ValueError('a spectra model has no last_FFN representation of width ffn_hidden_size. Use MPN '
                             'fingerprint type instead.')
        if sum(isinstance(m, torch.nn.Linear) for m in model.ffn) < 2:
            raise ValueError(NO_LATENT_LAYER)
    if latent == 'MPN' and mpn.features_only:
        raise ValueError('With features_only models, there is no latent MPN representation. Use last_FFN '
                         'fingerprint type instead.')
    if encodings is not None and head is None:
        raise NotImplementedError('predictions from encodings: the model\'s FFN is not one the native heads run')
    findex = features.index(range(n)) if features is not None and n else None
    dindex = atom_descriptors.index(range(n)) if atom_descriptors is not None and n else None
    n_enc = 0 if mpn.features_only else len(mpn.encoder)
    one_ok = n_enc == 1 and (mpn.atom_descriptors is None or (dindex is not None and mpn.encoder[0]._after_readout()))
    slots_ok = 1 < n_enc <= MAX_SLOTS and mpn.atom_descriptors is None
    many = encodings is None and (head is not None or latent == 'MPN') and (one_ok or slots_ok)
    for g0 in range(0, len(sizes), 8):
        if many and n_enc > 1:
            embs = _encode_slots(mpn, batches[g0:g0 + 8])
        else:
            embs = mpn.encoder[0].forward_many([_molecules(b)[0] for b in batches[g0:g0 + 8]]) if many else \
                [None] * len(sizes[g0:g0 + 8])
        for j, emb in enumerate(embs, g0):
            r0, r1 = starts[j], starts[j + 1]
            feats = None if findex is None else findex[r0:r1]
            mask = None if row_mask is None or not spectra else row_mask[r0:r1]
            desc = None if dindex is None else dindex[r0:r1]
            if own_forward:
                yield r0, model(_molecules(batches[j]), feats, desc)
                continue
            if head is None and latent is None:
                out = _fallback_predict(model, batches[j], feats, mask, with_encodings, desc)
                yield (r0,) + tuple(out) if with_encodings else (r0, out)
                continue
            if encodings is not None:
                emb = encodings[r0:r1]
            if emb is None:
                x = _encode_alone(mpn, batches[j]) if alone else mpn(_molecules(batches[j]), feats, desc)
            elif n_enc > 1 and encodings is None:  # (one launch: every slot's encoding and the feature rows into the FFN input)
                x = join_slots(emb, r1 - r0, feats)
            else:
                if desc is not None:  # (atom_descriptors_layer after the readout: one join, one layer launch)
                    emb = mpn.encoder[0].apply_descriptor_layer(_molecules(batches[j])[0], emb, desc)
                x = emb if feats is None else join_features(emb, feats)
            if latent == 'MPN':
                yield r0, x
                continue
            native = head is not None and x.dim() == 2 and x.dtype == torch.float32 and \
                x.device == _head_linears(head)[0].weight.device
            if latent == 'last_FFN':
                yield r0, head_latent(model, x, head) if native else model.ffn[:-1](x)
                continue
            out = head_predict(model, x, head, normalize=True, mask=mask) if spectra else \
                head_predict(model, x, head)
            yield (r0, out, x) if with_encodings else (r0, out)
