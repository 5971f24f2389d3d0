"""Per-atom descriptors resident on the device (``--atom_descriptors descriptor``, data/utils.py:310-339; the rows
``MPNEncoder.forward`` concatenates to the atom hidden states before ``atom_descriptors_layer``, mpn.py:77-79,
136-143).

The reference stacks a Python list of numpy arrays, pads them and copies them to the device, every step.  Here the
(scaled) descriptor rows of a split are uploaded once as an :class:`AtomDescriptorTable`; a batch is an
:class:`AtomDescriptorRows` -- the table plus a device slice of validated first rows -- and the encoder reads the
table where it lies:

* encoder dropout inactive (eval, or ``dropout == 0``): ``atom_descriptors_layer`` is a Linear without an
  activation and the readout is linear in the atom rows, so the layer runs *after* the readout
  (``wdmpnn_desc_join`` + ``wdmpnn_desc_layer``: B rows instead of n_atoms), and the encoder keeps the fused
  forward of a model without descriptors;
* a training forward with active dropout: ``wdmpnn_desc_rows`` fills the padded per-atom array and the per-atom
  layer runs as for a list.

The kernels read ``table[row0[b] + a]`` for ``a < mol_size[b]`` and clamp nothing, so a ``row0`` reaches them in
one way only: ``AtomDescriptorTable.index`` checks every position on the host before it uploads the rows, and
``AtomDescriptorRows.bind`` checks every molecule's atom count against the graph's ``a_scope``.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np
import torch

from . import _native

ATOM_COUNT_MISMATCH = 'The number of atoms is different from the length of the extra atom features'


class AtomDescriptorTable:
    """The descriptor rows of one data split on ``device``: ``arrays`` holds one numeric ``[n_atoms_i][d]`` array
    per molecule, equal ``d``.  With a ``scaler`` each array goes through ``scaler.transform`` first (data.py:
    432-478); the rows are then cast to float32 on the host exactly as ``MPNEncoder.forward`` casts a list
    (float64 rows into a float32 buffer), so the device values are bitwise those of that path.  One upload.  The
    row offsets and atom counts stay on the host."""

    def __init__(self, arrays, device, scaler=None):
        mats, d = [], None
        for k, a in enumerate(arrays):
            a = np.asarray(a)
            if a.ndim != 2 or a.dtype.kind not in 'fiu':
                raise ValueError(f'AtomDescriptorTable: molecule {k} has descriptors of shape {a.shape} ({a.dtype}); '
                                 'a numeric [n_atoms][d] array is expected')
            if d is None:
                d = int(a.shape[1])
            if a.shape[1] != d or d < 1:
                raise ValueError(f'AtomDescriptorTable: molecule {k} has {a.shape[1]} descriptors per atom, the '
                                 f'first molecule {d} (every molecule needs the same width, at least 1)')
            if scaler is not None:
                a = np.asarray(scaler.transform(a))
            mats.append(a)
        if d is None:
            raise ValueError('AtomDescriptorTable: no molecules')
        self.counts = np.array([m.shape[0] for m in mats], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        host = np.zeros((int(self.offsets[-1]), d), np.float32)
        if host.shape[0]:
            host[:] = np.concatenate(mats, axis=0)
        self.data = torch.from_numpy(host).to(torch.device(device))
        self.n_mols, self.n_rows, self.width = len(mats), int(host.shape[0]), d

    @property
    def device(self) -> torch.device:
        return self.data.device

    def __len__(self) -> int:
        return self.n_mols

    def index(self, positions: Sequence[int]) -> 'AtomDescriptorIndex':
        """The molecules ``positions`` (host ints, each in ``[0, len(table))``: ``ValueError`` otherwise, before
        anything is uploaded) as one int64 upload of their first rows; slice the result per batch."""
        pos = np.asarray(positions if not isinstance(positions, range) else list(positions))
        if pos.ndim != 1 or (pos.size and pos.dtype.kind not in 'iu'):
            raise ValueError('AtomDescriptorTable.index expects a flat sequence of ints')
        pos = pos.astype(np.int64)
        bad = (pos < 0) | (pos >= self.n_mols)
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f'molecule {int(pos[k])} at position {k} is outside the descriptor table of '
                             f'{self.n_mols} molecules')
        row0 = np.ascontiguousarray(self.offsets[pos])
        return AtomDescriptorIndex(self, torch.from_numpy(row0).to(self.data.device), self.counts[pos], _checked=True)

    def rows(self, positions: Sequence[int]) -> 'AtomDescriptorRows':
        """``index(positions)[:]``."""
        return self.index(positions)[:]


class AtomDescriptorIndex:
    """Validated first rows of molecules of an :class:`AtomDescriptorTable` on its device, with their atom counts
    on the host.  ``index[a:b]`` is the :class:`AtomDescriptorRows` of those molecules: a view, no launch."""

    def __init__(self, table: AtomDescriptorTable, row0: torch.Tensor, counts: np.ndarray, _checked: bool = False):
        if not _checked:
            raise TypeError('an AtomDescriptorIndex comes from AtomDescriptorTable.index (which validates the '
                            'positions)')
        self.table, self._row0, self._counts = table, row0, counts

    def __len__(self) -> int:
        return int(self._row0.shape[0])

    def __getitem__(self, s) -> 'AtomDescriptorRows':
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError('an AtomDescriptorIndex is sliced as index[a:b]')
        return AtomDescriptorRows(self.table, self._row0[s], self._counts[s], _checked=True)


class AtomDescriptorRows:
    """The descriptors of one batch: a table, a device slice of validated first rows, the atom counts."""

    def __init__(self, table: AtomDescriptorTable, row0: torch.Tensor, counts: np.ndarray, _checked: bool = False):
        if not _checked:
            raise TypeError('AtomDescriptorRows come from AtomDescriptorIndex[a:b] or AtomDescriptorTable.rows')
        self.table, self._row0, self._counts = table, row0, counts

    def __len__(self) -> int:
        return int(self._row0.shape[0])

    @property
    def width(self) -> int:
        return self.table.width

    @property
    def device(self) -> torch.device:
        return self.table.data.device

    def bind(self, mol_graph) -> None:
        """The host checks that let these rows reach a kernel with ``mol_graph``: one molecule per ``a_scope``
        entry, each with as many descriptor rows as the graph has atoms for it (the reference's ``ValueError``,
        mpn.py:139-141), and no molecule without atoms (the reference's ``torch.stack`` fails on those,
        mpn.py:149 vs 171).  Checked once per graph and rows object."""
        seen = self.__dict__.setdefault('_bound', set())
        if id(mol_graph) in seen:
            return
        sizes = np.fromiter((n for _, n in mol_graph.a_scope), dtype=np.int64, count=len(mol_graph.a_scope))
        if sizes.shape[0] != len(self) or (sizes != self._counts).any():
            raise ValueError(ATOM_COUNT_MISMATCH)
        if (sizes == 0).any():
            raise RuntimeError('stack expects each tensor to be equal size (empty molecule with atom descriptors, '
                               'mpn.py:149 vs 171)')
        seen.add(id(mol_graph))
        # (the graph stays alive with the rows: an id is only unique among live objects)
        self.__dict__.setdefault('_bound_graphs', []).append(mol_graph)

    def to_list(self) -> list:
        """The batch as the list of float32 ``[n_atoms_i][d]`` numpy arrays the list path takes (a device-to-host
        copy: for tests and tools)."""
        host = self.table.data.cpu().numpy()
        r0 = self._row0.cpu().numpy()
        return [host[int(a):int(a) + int(n)] for a, n in zip(r0, self._counts)]


def is_device_descriptors(x) -> bool:
    """Whether ``x`` is a descriptor batch read from a device table (no host copy)."""
    return isinstance(x, AtomDescriptorRows)


def desc_join(rows: AtomDescriptorRows, gs, emb: torch.Tensor, aggregation: int, aggregation_norm: float,
              stream: int) -> torch.Tensor:
    """``wdmpnn_desc_join``: x ``[B][H + d + 1]`` = [emb | readout(desc) | s] for the bound graph struct ``gs``."""
    B, H = int(emb.shape[0]), int(emb.shape[1])
    d = rows.width
    if B != len(rows) or B != gs.n_mols:
        raise ValueError(f'desc_join: {B} encodings, {len(rows)} descriptor molecules, {gs.n_mols} graph molecules')
    x = torch.empty((B, H + d + 1), dtype=torch.float32, device=emb.device)
    j = _native.WdDescJoin()
    j.g = ctypes.pointer(gs)
    j.H, j.d = H, d
    j.emb, j.ld_emb = emb.data_ptr(), emb.stride(0) if B else H
    j.table, j.ld_table, j.table_rows = rows.table.data.data_ptr(), d, rows.table.n_rows
    j.row0 = rows._row0.data_ptr()
    j.aggregation, j.aggregation_norm = aggregation, aggregation_norm
    j.x, j.ld_x = x.data_ptr(), H + d + 1
    _native.check(_native.lib().wdmpnn_desc_join(ctypes.byref(j), stream), 'atom descriptor join')
    return x


def desc_layer(x: torch.Tensor, W: torch.Tensor, b, stream: int) -> torch.Tensor:
    """``wdmpnn_desc_layer``: y ``[B][Hd]`` from x ``[B][Hd + 1]``."""
    B, Hd = int(x.shape[0]), int(x.shape[1]) - 1
    y = torch.empty((B, Hd), dtype=torch.float32, device=x.device)
    l = _native.WdDescLayer()
    l.B, l.Hd = B, Hd
    l.x, l.ld_x = x.data_ptr(), Hd + 1
    l.W_d, l.b_d = W.data_ptr(), _native.ptr(b) or None
    l.y, l.ld_y = y.data_ptr(), Hd
    _native.check(_native.lib().wdmpnn_desc_layer(ctypes.byref(l), stream), 'atom descriptor layer')
    return y


def desc_layer_backward(dy: torch.Tensor, x: torch.Tensor, W: torch.Tensor, H: int, dW, db, demb, stream: int) -> None:
    """``wdmpnn_desc_layer_backward`` into the given tensors (each may be None: skipped)."""
    B, Hd = int(x.shape[0]), int(x.shape[1]) - 1
    l = _native.WdDescLayerBackward()
    l.B, l.H, l.Hd = B, H, Hd
    l.dy, l.ld_dy = dy.data_ptr(), Hd
    l.x, l.ld_x = x.data_ptr(), Hd + 1
    l.W_d = W.data_ptr()
    l.dW_d, l.db_d = _native.ptr(dW) or None, _native.ptr(db) or None
    l.demb, l.ld_demb = _native.ptr(demb) or None, H
    _native.check(_native.lib().wdmpnn_desc_layer_backward(ctypes.byref(l), stream), 'atom descriptor layer backward')


def desc_rows(rows: AtomDescriptorRows, gs, stream: int) -> torch.Tensor:
    """``wdmpnn_desc_rows``: the padded per-atom array ``[rup(n_atoms, 128)][rup(d, 32)]`` of the per-atom path."""
    d = rows.width
    if gs.n_mols != len(rows):
        raise ValueError(ATOM_COUNT_MISMATCH)
    R, ld = -(-gs.n_atoms // 128) * 128, -(-d // 32) * 32
    out = torch.empty((R, ld), dtype=torch.float32, device=rows.device)
    r = _native.WdDescRows()
    r.g = ctypes.pointer(gs)
    r.d = d
    r.table, r.ld_table, r.table_rows = rows.table.data.data_ptr(), d, rows.table.n_rows
    r.row0 = rows._row0.data_ptr()
    r.atom_desc, r.rows, r.ld = out.data_ptr(), R, ld
    _native.check(_native.lib().wdmpnn_desc_rows(ctypes.byref(r), stream), 'atom descriptor rows')
    return out


class _LayerAfterReadout(torch.autograd.Function):
    """``[emb | readout(desc)] W_d^T + s b_d`` under autograd: the join and the layer in two launches, the three
    gradients in one.  ``emb`` carries the encoder's graph, so the encoder backward runs unchanged on ``demb``."""

    @staticmethod
    def forward(ctx, emb, W, b, rows, gs, aggregation, aggregation_norm, keep):
        emb = emb.contiguous()
        sid = _native.current_stream(emb.device)
        x = desc_join(rows, gs, emb, aggregation, aggregation_norm, sid)
        y = desc_layer(x, W, b, sid)
        ctx.save_for_backward(x, W)
        ctx.H, ctx.has_b = int(emb.shape[1]), b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        need_emb, need_W, need_b = ctx.needs_input_grad[:3]
        dy = dy.contiguous()
        dev, Hd = dy.device, int(W.shape[0])
        dW = torch.empty_like(W) if need_W else None
        db = torch.empty(Hd, dtype=torch.float32, device=dev) if need_b and ctx.has_b else None
        demb = torch.empty((dy.shape[0], ctx.H), dtype=torch.float32, device=dev) if need_emb else None
        desc_layer_backward(dy, x, W, ctx.H, dW, db, demb, _native.current_stream(dev))
        return demb, dW, db, None, None, None, None, None
