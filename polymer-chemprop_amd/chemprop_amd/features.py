"""Molecule-level input features resident on the device (``--features_path``, data/utils.py:242-258; the rows
``MPN.forward`` appends to the encoding, mpn.py:281-285).

The reference stacks a Python list of numpy rows, copies it to the device and concatenates, every step.  Here
the (already scaled) feature matrix of a split is uploaded once as a :class:`FeatureTable`; a batch is a
:class:`FeatureRows` -- the table plus a device slice of a validated row index -- and ``train.join_features``
builds the FFN input ``[encoding | table[idx]]`` in one ``wdmpnn_join_rows`` launch, with no host copy.

The join kernel reads ``table[idx[b]]`` and clamps nothing, so an index reaches it in one way only:
``FeatureTable.index`` checks every position against the table on the host before it uploads them, and
``FeatureIndex[a:b]`` hands out slices of that upload.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _native


class FeatureTable:
    """The feature rows ``[N][Ff]`` of one data split on ``device``.  ``array`` is any float array, already
    scaled by the caller; it is cast to float32 on the host exactly as ``MPN.forward`` casts a list of rows
    (``torch.from_numpy(...).float()``), so the device values are bitwise those of that path.  One upload.
    (A table on the CPU can be built and indexed -- the index checks are host code -- but nothing launches
    from it: ``to_tensor`` and ``join_features`` need a GPU.)"""

    def __init__(self, array, device):
        a = np.ascontiguousarray(np.asarray(array))
        if a.ndim != 2 or a.shape[1] < 1 or a.dtype.kind not in 'fiu':
            raise ValueError(f'FeatureTable expects a numeric [N][Ff] array with Ff >= 1 (got shape {a.shape}, '
                             f'{a.dtype})')
        self.data = torch.from_numpy(a).float().to(torch.device(device))
        self.n_rows, self.width = int(a.shape[0]), int(a.shape[1])

    @property
    def device(self) -> torch.device:
        return self.data.device

    def __len__(self) -> int:
        return self.n_rows

    def index(self, positions: Sequence[int]) -> 'FeatureIndex':
        """The rows ``positions`` (host ints, each in ``[0, N)``: ``ValueError`` otherwise, before anything is
        uploaded) as one int64 upload; slice the result per batch."""
        pos = np.asarray(positions)
        if pos.ndim != 1 or (pos.size and pos.dtype.kind not in 'iu'):
            raise ValueError('FeatureTable.index expects a flat sequence of ints')
        pos = pos.astype(np.int64)
        bad = (pos < 0) | (pos >= self.n_rows)
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f'feature row {int(pos[k])} at position {k} is outside the table of {self.n_rows} rows')
        return FeatureIndex(self, torch.from_numpy(pos).to(self.data.device), _checked=True)

    def rows(self, positions: Sequence[int]) -> 'FeatureRows':
        """``index(positions)[:]``."""
        return self.index(positions)[:]


class FeatureIndex:
    """A validated row index of a :class:`FeatureTable` on its device (``FeatureTable.index`` builds it).
    ``index[a:b]`` is the :class:`FeatureRows` of those positions: a view, no launch and no copy."""

    def __init__(self, table: FeatureTable, idx: torch.Tensor, _checked: bool = False):
        if not _checked:
            raise TypeError('a FeatureIndex comes from FeatureTable.index (which validates the positions)')
        self.table, self._idx = table, idx

    def __len__(self) -> int:
        return int(self._idx.shape[0])

    def __getitem__(self, s) -> 'FeatureRows':
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError('a FeatureIndex is sliced as index[a:b]')
        return FeatureRows(self.table, self._idx[s], _checked=True)


class FeatureRows:
    """The feature rows of one batch: a table and a device slice of a validated index into it."""

    def __init__(self, table: FeatureTable, idx: torch.Tensor, _checked: bool = False):
        if not _checked:
            raise TypeError('FeatureRows come from FeatureIndex[a:b] or FeatureTable.rows')
        self.table, self._idx = table, idx

    def __len__(self) -> int:
        return int(self._idx.shape[0])

    @property
    def width(self) -> int:
        return self.table.width

    @property
    def device(self) -> torch.device:
        return self.table.data.device

    def segment(self) -> tuple:
        """This batch as a ``_native.join_rows`` segment."""
        t = self.table
        return (t.data.data_ptr(), t.width, 0, t.width, self._idx.data_ptr())

    def to_tensor(self) -> torch.Tensor:
        """``table[idx]`` as a float32 ``[B][Ff]`` tensor: one gather launch."""
        dev = self.device
        if dev.type != 'cuda':
            raise ValueError(f'FeatureRows.to_tensor: the table is on {dev}, the gather kernel needs a GPU')
        out = torch.empty((len(self), self.width), dtype=torch.float32, device=dev)
        _native.join_rows(out, [self.segment()], _native.current_stream(dev))
        return out


def is_device_features(f) -> bool:
    """Whether ``f`` is a features batch the native step takes without a host copy: :class:`FeatureRows`, or a
    float32 ``[B][Ff]`` tensor on a GPU."""
    if isinstance(f, FeatureRows):
        return f.device.type == 'cuda'
    return torch.is_tensor(f) and f.dim() == 2 and f.dtype == torch.float32 and f.device.type == 'cuda' and \
        f.shape[1] >= 1


def features_width(f) -> int:
    return f.width if isinstance(f, FeatureRows) else int(f.shape[1])


def features_segment(f) -> tuple:
    """A device features batch (``is_device_features``) as a ``_native.join_rows`` segment, with whatever must
    stay alive until the launch is enqueued."""
    if isinstance(f, FeatureRows):
        return f.segment(), f
    t = f.detach().contiguous()
    return (t.data_ptr(), t.shape[1], 0, t.shape[1], 0), t


def join_features(emb: torch.Tensor, rows) -> torch.Tensor:
    """``[emb | rows]`` as a float32 ``[B][H + Ff]`` tensor in one ``wdmpnn_join_rows`` launch (the
    ``torch.cat`` of ``MPN.forward`` without autograd: the result carries no graph).  ``emb`` is a float32
    ``[B][H]`` tensor on the GPU, ``rows`` a :class:`FeatureRows` or a float32 ``[B][Ff]`` tensor there."""
    if not is_device_features(rows):
        raise TypeError('join_features expects FeatureRows or a float32 [B][Ff] tensor on the GPU')
    if emb.dim() != 2 or emb.dtype != torch.float32 or emb.device.type != 'cuda':
        raise ValueError(f'join_features: encodings of shape {tuple(emb.shape)} ({emb.dtype}, {emb.device})')
    n = len(rows) if isinstance(rows, FeatureRows) else int(rows.shape[0])
    if n != emb.shape[0] or rows.device != emb.device:
        raise ValueError(f'join_features: {n} feature rows on {rows.device} for {emb.shape[0]} encodings on '
                         f'{emb.device}')
    emb = emb.detach().contiguous()
    seg, keep = features_segment(rows)
    H = emb.shape[1]
    out = torch.empty((n, H + features_width(rows)), dtype=torch.float32, device=emb.device)
    _native.join_rows(out, [(emb.data_ptr(), H, 0, H, 0), seg], _native.current_stream(emb.device))
    del keep
    return out


def split_columns(x: torch.Tensor, c0: int, w: int) -> torch.Tensor:
    """``x[:, c0:c0 + w]`` of a contiguous float32 ``[B][ld]`` GPU tensor as a contiguous tensor: one launch."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.device.type != 'cuda' or \
            c0 < 0 or w < 1 or c0 + w > x.shape[1]:
        raise ValueError(f'split_columns: columns {c0}..{c0 + w} of a tensor of shape {tuple(x.shape)} ({x.dtype})')
    out = torch.empty((x.shape[0], w), dtype=torch.float32, device=x.device)
    _native.join_rows(out, [(x.data_ptr(), x.shape[1], c0, w, 0)], _native.current_stream(x.device))
    return out
