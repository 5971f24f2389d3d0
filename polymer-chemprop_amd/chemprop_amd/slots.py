"""One batch of a model of several molecules per input (``number_of_molecules > 1``: polymer + solvent, solute +
solvent, ...; mpn.py:270-285 runs one encoder per molecule and concatenates their outputs).

A :class:`SlotBatch` is the list of the per-molecule ``BatchMolGraph`` s that ``MPN.forward`` takes, so every
caller of ``[g0, g1, ...]`` takes it unchanged.  For a shared encoder (``mpn_shared``) it also holds ``merged``:
all N B molecules as one ``BatchMolGraph`` in slot-major order, which the shared encoder runs once; its output
``[N B][H]`` is the slot-major layout ``wdmpnn_slots_join`` reads and ``wdmpnn_slots_split`` writes.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _native
from .features import features_segment, features_width, is_device_features
from .featurization import BatchMolGraph


def _widths(g) -> tuple:
    """(atom feature width, bond feature width) of a ``MolGraph``, None where it has no such row."""
    return (len(g.f_atoms[0]) if g.n_atoms else None), (len(g.f_bonds[0]) if g.n_bonds else None)


class SlotBatch(list):
    """``SlotBatch(mol_lists, shared=False)``: ``mol_lists`` are N lists of B ``MolGraph`` s, list k holding
    molecule k of every row.  The object is the list of the N ``BatchMolGraph`` s; ``shared=True`` adds
    ``merged``, the ``BatchMolGraph`` of slot 0's B molecules, then slot 1's, ... (None otherwise).
    ``ValueError`` for N outside 1 .. 8, lists of unequal lengths, or atom / bond feature widths that differ
    between the slots (one FFN input row holds every slot's encoding of the same row; a merged batch has one width)."""

    def __init__(self, mol_lists: Sequence[Sequence], shared: bool = False, **batch_kwargs):
        mol_lists = [list(m) for m in mol_lists]
        n = len(mol_lists)
        if not 1 <= n <= _native.MAX_SLOTS:
            raise ValueError(f'SlotBatch: {n} molecules per input (1 .. {_native.MAX_SLOTS})')
        sizes = [len(m) for m in mol_lists]
        if len(set(sizes)) != 1:
            raise ValueError(f'SlotBatch: the slots hold {sizes} molecules: every row needs one molecule per slot')
        if sizes[0] == 0:
            raise ValueError('SlotBatch: no rows')
        atom_w, bond_w = set(), set()
        for mols in mol_lists:
            for g in mols:
                fa, fb = _widths(g)
                if fa is not None:
                    atom_w.add(fa)
                if fb is not None:
                    bond_w.add(fb)
        if len(atom_w) > 1 or len(bond_w) > 1:
            raise ValueError(f'SlotBatch: atom feature widths {sorted(atom_w)} and bond feature widths '
                             f'{sorted(bond_w)}: every slot needs the same')
        super().__init__(BatchMolGraph(m, **batch_kwargs) for m in mol_lists)
        if n > 1 and any(b.__dict__.get('_compact_extra') for b in self):
            # (the reference refuses them as well: atom / bond features need number_of_molecules == 1)
            raise ValueError('SlotBatch: extra atom / bond features (--atom_features_path, '
                             '--bond_features_path) are not supported with --number_of_molecules > 1')
        self.n_rows = sizes[0]
        self.merged: Optional[BatchMolGraph] = None
        if shared:
            self.merged = BatchMolGraph([g for m in mol_lists for g in m], **batch_kwargs)

    @classmethod
    def from_batches(cls, batches: Sequence[BatchMolGraph], merged: Optional[BatchMolGraph] = None) -> 'SlotBatch':
        """The ``SlotBatch`` of prebuilt ``BatchMolGraph`` s, one per slot (``graph_table.GraphRows.slot_batch``
        gathers them from a resident table), and of their ``merged`` graph for a shared encoder: slot 0's
        molecules, then slot 1's, and so on.  The same ``ValueError`` s as the constructor's."""
        batches = list(batches)
        n = len(batches)
        if not 1 <= n <= _native.MAX_SLOTS:
            raise ValueError(f'SlotBatch: {n} molecules per input (1 .. {_native.MAX_SLOTS})')
        sizes = [len(b.a_scope) for b in batches]
        if len(set(sizes)) != 1:
            raise ValueError(f'SlotBatch: the slots hold {sizes} molecules: every row needs one molecule per slot')
        if sizes[0] == 0:
            raise ValueError('SlotBatch: no rows')
        widths = {(b.atom_fdim, b.bond_fdim) for b in batches + ([] if merged is None else [merged])}
        if len(widths) > 1:
            raise ValueError(f'SlotBatch: (atom, bond) feature widths {sorted(widths)}: every slot needs the same')
        if merged is not None and len(merged.a_scope) != n * sizes[0]:
            raise ValueError(f'SlotBatch: a merged graph of {len(merged.a_scope)} molecules for {n} slots of '
                             f'{sizes[0]}')
        self = cls.__new__(cls)
        list.__init__(self, batches)
        self.n_rows = sizes[0]
        self.merged = merged
        return self


def shares_encoder(model) -> bool:
    """Whether ``model`` runs one encoder for several molecules per input (``mpn_shared``)."""
    encs = getattr(getattr(model, 'encoder', None), 'encoder', None)
    return encs is not None and len(encs) > 1 and all(e is encs[0] for e in encs)


def merged_graph(batch) -> Optional[BatchMolGraph]:
    """The merged graph of a :class:`SlotBatch` built with ``shared=True``, else None."""
    return getattr(batch, 'merged', None) if isinstance(batch, SlotBatch) else None


def join_slots(embs: Sequence[torch.Tensor], n_rows: int, feats=None) -> torch.Tensor:
    """The FFN input ``[B][N H + Ff]`` in one ``wdmpnn_slots_join`` launch.  ``embs``: the N encodings ``[B][H]``
    (float32, contiguous, on one GPU), or one slot-major tensor ``[N B][H]`` in a list of one with ``n_rows = B``.
    ``feats``: ``features.FeatureRows`` or a float32 device tensor ``[B][Ff]``, or None."""
    ptrs, H, n, dev = _slot_pointers(embs, n_rows)
    seg = keep = None
    Ff = 0
    if feats is not None:
        if not is_device_features(feats):
            raise TypeError('join_slots expects FeatureRows or a float32 [B][Ff] tensor on the GPU')
        rows = len(feats) if not torch.is_tensor(feats) else int(feats.shape[0])
        if rows != n_rows or feats.device != dev:
            raise ValueError(f'join_slots: {rows} feature rows on {feats.device} for {n_rows} encodings on {dev}')
        seg, keep = features_segment(feats)
        Ff = features_width(feats)
    x = torch.empty((n_rows, n * H + Ff), dtype=torch.float32, device=dev)
    _native.slots_join(x, ptrs, H, H, seg, _native.current_stream(dev))
    del keep
    return x


def split_slots(dx: torch.Tensor, n: int, H: int) -> torch.Tensor:
    """``dx[:, k H : (k + 1) H]`` for every k as one slot-major tensor ``[n][B][H]`` (one ``wdmpnn_slots_split``
    launch): slice k is slot k's contiguous gradient, the whole the merged backward's ``dout``."""
    if dx.dim() != 2 or dx.dtype != torch.float32 or not dx.is_contiguous() or dx.device.type != 'cuda' or \
            dx.shape[1] < n * H:
        raise ValueError(f'split_slots: {n} slots of {H} columns from a tensor of shape {tuple(dx.shape)} ({dx.dtype})')
    B = dx.shape[0]
    out = torch.empty((n, B, H), dtype=torch.float32, device=dx.device)
    base = out.data_ptr()
    _native.slots_split(dx, [base + 4 * k * B * H for k in range(n)], H, H, _native.current_stream(dx.device))
    return out


def _slot_pointers(embs, n_rows: int):
    embs = list(embs)
    e0 = embs[0]
    for e in embs:
        if e.dim() != 2 or e.dtype != torch.float32 or e.device.type != 'cuda' or not e.is_contiguous() or \
                e.shape[1] != e0.shape[1] or e.device != e0.device:
            raise ValueError(f'slots: encodings of shape {tuple(e.shape)} ({e.dtype}, {e.device})')
    H = int(e0.shape[1])
    if len(embs) == 1 and e0.shape[0] != n_rows:  # slot-major [N B][H]
        if n_rows < 1 or e0.shape[0] % n_rows:
            raise ValueError(f'slots: {e0.shape[0]} merged rows for batches of {n_rows}')
        n = e0.shape[0] // n_rows
        base = e0.data_ptr()
        return [base + 4 * k * n_rows * H for k in range(n)], H, n, e0.device
    if any(e.shape[0] != n_rows for e in embs):
        raise ValueError(f'slots: encodings of {[int(e.shape[0]) for e in embs]} rows for batches of {n_rows}')
    return [e.data_ptr() for e in embs], H, len(embs), e0.device
