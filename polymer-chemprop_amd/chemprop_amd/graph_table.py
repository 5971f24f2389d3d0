"""Training graphs resident on the device (``chemprop_train --resident_graphs``).

``BatchMolGraph(list of MolGraph)`` packs fp32 feature rows on the host for every training step, encodes them
back into categorical codes, plans the molecule blocks and uploads the image ``wdmpnn_build_graph`` expands.  A
molecule's compact record does not depend on where it stands in a batch, so here every molecule of a split is
encoded once into a :class:`GraphTable` (its codes on the device, its sizes and entry counts on the host); a
batch is a :class:`GraphRows` -- the table plus a device slice of a validated index -- and its
``BatchMolGraph`` gets its device graph from the host plan of the sizes (``compact_plan``, a few hundred bytes
uploaded), one ``wdmpnn_gather_compact`` launch and the same ``wdmpnn_build_graph_ex``.  The assembled image is
bitwise the one ``compact_stage`` makes for ``BatchMolGraph`` of the same molecules in the same order, so the
graph, the step and the scores are bitwise those of the list path.

The gather kernel reads ``table[ids[m]]`` and clamps nothing, so ids reach it in one way only:
``GraphTable.index`` checks every position on the host before it uploads them, and ``GraphIndex[a:b]`` hands out
slices of that upload (as ``features.FeatureTable`` does).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native
from .featurization import BLK_ATOMS, BLK_BONDS, BLK_TARGET, BatchMolGraph, _packer, build_from_image

_CHUNK = 512  # molecules encoded per native call while the table is built


class GraphTable:
    """The compact codes of ``graphs`` (``MolGraph`` s, or rows of N ``MolGraph`` s for a model of N molecules per
    input: the table then holds every slot, molecule ``row * N + slot``) on ``device``: one encode per molecule, one
    upload.  ``ValueError`` -- the reason ``BatchMolGraph`` gives for not encoding compactly and the index of the
    first offender -- when a molecule is not in the reference's categorical layout or alone exceeds a molecule
    block: the caller then keeps the list path.  ``block_target`` as ``BatchMolGraph``'s.
    (A table on the CPU can be built and indexed -- the checks are host code -- but its batches take the dense
    path from their decoded tables: the gather needs a GPU.)"""

    def __init__(self, graphs: Sequence, device, block_target: Optional[int] = None):
        graphs = list(graphs)
        if not graphs:
            raise ValueError('GraphTable: no molecules')
        self.n_slots = 1
        if isinstance(graphs[0], (tuple, list)):
            self.n_slots = len(graphs[0])
            if not 1 <= self.n_slots <= _native.MAX_SLOTS or \
                    any(not isinstance(r, (tuple, list)) or len(r) != self.n_slots for r in graphs):
                raise ValueError(f'GraphTable: every row needs {self.n_slots} molecules (1 .. {_native.MAX_SLOTS}), '
                                 f'as the first has')
            mols = [g for r in graphs for g in r]
        else:
            mols = graphs
        self.n_rows = len(graphs)
        self.block_target = BLK_TARGET if block_target is None else int(block_target)
        self.device = _device(device)
        sizes, xn, atoms, pairs, max_deg = [], [], [], [], []
        self.dims = None
        for c0 in range(0, len(mols), _CHUNK):
            chunk = mols[c0:c0 + _CHUNK]
            b = BatchMolGraph(chunk)
            if b._compact is None:  # which one?  (a molecule encodes alone exactly as it does in a batch)
                for j, g in enumerate(chunk):
                    why = BatchMolGraph([g])._compact_why
                    if why:
                        raise ValueError(f'GraphTable: {self._name(c0 + j)} does not encode compactly: {why}')
                raise ValueError(f'GraphTable: molecules {c0} .. {c0 + len(chunk)} do not encode compactly: '
                                 f'{b._compact_why}')
            if b._compact_extra is not None:
                raise ValueError('GraphTable: extra atom / bond features (--atom_features_path, '
                                 '--bond_features_path) are not supported with --resident_graphs')
            if self.dims is None:
                self.dims = b._compact_dims
                self._flags = (b.overwrite_default_atom_features, b.overwrite_default_bond_features,
                               b.atom_fdim, b.bond_fdim)
            elif b._compact_dims != self.dims:
                raise ValueError(f'GraphTable: feature widths {b._compact_dims} from {self._name(c0)} on, '
                                 f'{self.dims} before')
            m = np.frombuffer(b._compact[0], np.int32).reshape(-1, 4)
            big = (m[:, 1] > BLK_ATOMS) | (m[:, 3] > BLK_BONDS)
            if big.any():
                j = int(np.argmax(big))
                raise ValueError(f'GraphTable: {self._name(c0 + j)} exceeds a molecule block: {int(m[j, 1])} atoms, '
                                 f'{int(m[j, 3])} directed bonds (at most {BLK_ATOMS} / {BLK_BONDS})')
            ent = _packer().compact_entries(*b._compact, *self.dims)
            if ent is None:
                raise ValueError(f'GraphTable: molecules {c0} .. {c0 + len(chunk)}: a bond leaves its molecule')
            sizes.append(np.concatenate([m[:, [1, 3]], np.frombuffer(ent, np.int32).reshape(-1, 2)], axis=1))
            max_deg.append([int(b._deg[s:s + n].max()) if n else 0 for s, n in b.a_scope])
            xn.append(np.frombuffer(b._compact[1], np.float32))
            atoms.append(np.frombuffer(b._compact[2], np.uint8).reshape(-1, 16)[1:])  # (without the pad row)
            pairs.append(np.frombuffer(b._compact[3], np.uint8).reshape(-1, 16))
        # host side: what a plan and a lazy decode need
        self.sizes = np.ascontiguousarray(np.concatenate(sizes), np.int32)  # [M][4] n_atoms, n_bonds, nnz_msg, nnz_agg
        self.xn = np.ascontiguousarray(np.concatenate(xn), np.float32)
        # [M] largest atom degree: a batch's max_num_bonds (the atom-message graph's pad slots) without a decode
        self.max_deg = np.concatenate([np.asarray(d, np.int32) for d in max_deg])
        self.atoms = np.concatenate(atoms)
        self.pairs = np.concatenate(pairs)
        first = np.zeros((len(mols), 2), np.int64)
        np.cumsum(self.sizes[:-1, 0], out=first[1:, 0])
        np.cumsum(self.sizes[:-1, 1] // 2, out=first[1:, 1])
        self.first = first
        # device side, one upload each (a spare record at the end: a table without bonds still has a pair array)
        spare = np.zeros((1, 16), np.uint8)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        self._d_atoms = up(np.concatenate([self.atoms, spare]))
        self._d_pairs = up(np.concatenate([self.pairs, spare]))
        self._d_xn = up(self.xn)
        self._d_first = up(first)
        # the uploads above are complete on return (pageable copies), so any stream may read the table; a stream
        # other than the one current here only has to keep the allocations alive (_use_on)
        self._streams = set()
        if self.device.type == 'cuda':
            self._streams.add(torch.cuda.current_stream(self.device).cuda_stream)

    def _name(self, mol: int) -> str:
        if self.n_slots == 1:
            return f'molecule {mol}'
        return f'molecule {mol % self.n_slots} of row {mol // self.n_slots}'

    def __len__(self) -> int:
        return self.n_rows

    def _use_on(self, stream) -> None:
        """Keep the table's memory alive for a gather enqueued on ``stream`` (the ``DeviceGraph.use_on``
        convention: ``record_stream`` once per stream other than the home stream)."""
        if stream.cuda_stream in self._streams:
            return
        for t in (self._d_atoms, self._d_pairs, self._d_xn, self._d_first):
            t.record_stream(stream)
        self._streams.add(stream.cuda_stream)

    def index(self, positions: Sequence[int]) -> 'GraphIndex':
        """The rows ``positions`` (host ints, each in ``[0, N)``: ``ValueError`` otherwise, before anything is
        uploaded) as one int64 upload; slice the result per batch."""
        pos = np.asarray(positions)
        if pos.ndim != 1 or (pos.size and pos.dtype.kind not in 'iu'):
            raise ValueError('GraphTable.index expects a flat sequence of ints')
        pos = pos.astype(np.int64)
        bad = (pos < 0) | (pos >= self.n_rows)
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f'graph row {int(pos[k])} at position {k} is outside the table of {self.n_rows} rows')
        return GraphIndex(self, pos, torch.from_numpy(pos).to(self.device), _checked=True)  # (complete on return)

    def rows(self, positions: Sequence[int]) -> 'GraphRows':
        """``index(positions)[:]``."""
        return self.index(positions)[:]


class GraphIndex:
    """A validated row index of a :class:`GraphTable`, on the host and on its device (``GraphTable.index`` builds
    it).  ``index[a:b]`` is the :class:`GraphRows` of those positions: views, no launch and no copy."""

    def __init__(self, table: GraphTable, pos: np.ndarray, idx: torch.Tensor, _checked: bool = False):
        if not _checked:
            raise TypeError('a GraphIndex comes from GraphTable.index (which validates the positions)')
        self.table, self._pos, self._idx = table, pos, idx
        # the stream the index was allocated on: a gather on another one records its use (_TableSource.device_graph)
        self._home = torch.cuda.current_stream(idx.device).cuda_stream if idx.device.type == 'cuda' else None

    def __len__(self) -> int:
        return int(self._pos.shape[0])

    def __getitem__(self, s) -> 'GraphRows':
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError('a GraphIndex is sliced as index[a:b]')
        return GraphRows(self.table, self._pos[s], self._idx[s], self._home, _checked=True)


class GraphRows:
    """The graphs of one batch: a table, and a host and a device slice of a validated index into it."""

    def __init__(self, table: GraphTable, pos: np.ndarray, idx: torch.Tensor, home=None, _checked: bool = False):
        if not _checked:
            raise TypeError('GraphRows come from GraphIndex[a:b] or GraphTable.rows')
        self.table, self._pos, self._idx, self._home = table, pos, idx, home

    def __len__(self) -> int:
        return int(self._pos.shape[0])

    def _batch(self, slot0: int, n: int) -> BatchMolGraph:
        if not len(self):
            raise ValueError('GraphRows: no rows')
        return _TableSource(self, slot0, n).batch()

    def batch(self, slot: int = 0) -> BatchMolGraph:
        """The ``BatchMolGraph`` of these rows (of their molecule ``slot`` in a table of rows of N molecules)."""
        if not 0 <= slot < self.table.n_slots:
            raise ValueError(f'GraphRows.batch: slot {slot} of a table of {self.table.n_slots} molecules per row')
        return self._batch(slot, 1)

    def slot_batch(self, shared: bool = False):
        """The ``slots.SlotBatch`` of these rows: one ``BatchMolGraph`` per slot and, with ``shared`` (a model with
        ``mpn_shared``), the merged one: slot 0's molecules, then slot 1's, and so on."""
        from .slots import SlotBatch
        n = self.table.n_slots
        return SlotBatch.from_batches([self._batch(k, 1) for k in range(n)],
                                      merged=self._batch(0, n) if shared else None)


class _TableSource:
    """What makes a ``BatchMolGraph`` a batch of a :class:`GraphTable` (its ``_source``): scopes and sizes come from
    the host plan, ``device_graph`` (on the table's GPU) gathers the compact image on the device,
    and the reference's tables are decoded, from the table's host copy of the codes, only if a host attribute is
    read."""

    def __init__(self, rows: GraphRows, slot0: int, n: int):
        t = rows.table
        self.rows, self.slot0 = rows, slot0
        # batch molecule m = slot (slot0 + m // B) of row pos[m % B]
        ids = rows._pos * t.n_slots + slot0
        if n > 1:
            ids = np.concatenate([ids + k for k in range(n)])
        self.mol_ids = ids
        self.sizes = np.ascontiguousarray(t.sizes[ids])

    def batch(self) -> BatchMolGraph:
        t, sz = self.rows.table, self.sizes
        g = BatchMolGraph.__new__(BatchMolGraph)
        (g.overwrite_default_atom_features, g.overwrite_default_bond_features, g.atom_fdim, g.bond_fdim) = t._flags
        g._compact_dims = t.dims
        g._compact_why = ''
        g.block_target = t.block_target
        a0 = 1 + np.cumsum(sz[:, 0]) - sz[:, 0]
        b0 = 1 + np.cumsum(sz[:, 1]) - sz[:, 1]
        g.n_atoms = 1 + int(sz[:, 0].sum())
        g.n_bonds = 1 + int(sz[:, 1].sum())
        g.a_scope = list(zip(a0.tolist(), sz[:, 0].tolist()))
        g.b_scope = list(zip(b0.tolist(), sz[:, 1].tolist()))
        g.degree_of_polym = t.xn[self.mol_ids].astype(np.float64).tolist()
        g.max_num_bonds = max(1, int(t.max_deg[self.mol_ids].max()))  # featurization.py:802-803
        g._a2b = None
        g._gathers = None
        g.b2b = None
        g.a2a = None
        g._device_cache = {}
        g._source = self
        return g

    def host_compact(self, g: BatchMolGraph) -> tuple:
        """The batch's (mols, xn, atoms, pairs) as ``BatchMolGraph._compact`` holds them."""
        t = self.rows.table
        mols = np.concatenate([np.array(g.a_scope, np.int32).reshape(-1, 2),
                               np.array(g.b_scope, np.int32).reshape(-1, 2)], axis=1)
        atoms = [np.frombuffer(_pad_atom(), np.uint8).reshape(1, 16)]
        pairs = [np.zeros((0, 16), np.uint8)]
        for i, (na, nb) in zip(self.mol_ids, self.sizes[:, :2]):
            fa, fp = t.first[i]
            atoms.append(t.atoms[fa:fa + na])
            pairs.append(t.pairs[fp:fp + nb // 2])
        return (bytearray(mols.tobytes()), bytearray(t.xn[self.mol_ids].tobytes()),
                bytearray(np.concatenate(atoms).tobytes()), bytearray(np.concatenate(pairs).tobytes()))

    def device_graph(self, g: BatchMolGraph, device, atom_messages: bool = False):
        """The batch's DeviceGraph on the table's GPU: plan -> small pinned image -> H2D -> gather ->
        ``wdmpnn_build_graph_ex``, or for an atom-message encoder ``wdmpnn_build_graph_atom`` (the same image; its
        offsets follow from the block table, and the pad slots' count from the table's per-molecule degrees);
        None on any other device (the batch then takes the paths of a ``from_compact`` batch, from its host
        arrays)."""
        t = self.rows.table
        device = _device(device)
        if device.type != 'cuda' or device != t.device:
            return None
        B = len(self.mol_ids)
        # the host-made sections: mols | blocks | block_nnz (blocks <= molecules), each 256-byte aligned.  The
        # pinned block is torch's: its caching host allocator records the copies' stream event when they are
        # enqueued and recycles the block only after they have run, so no staging buffer is rewritten early.
        host = torch.empty(56 * B + 3 * 256, dtype=torch.uint8, pin_memory=True)
        info = _packer().compact_plan(self.sizes, g.block_target, host.data_ptr(), host.numel())
        if info is None:
            raise ValueError('a molecule of a GraphTable exceeds a molecule block (the table checks that)')
        copied, counts, off, total, (h_mols, h_blocks, h_nnz), blk_max = info
        assert copied, 'planned sections larger than their bound'
        n_blocks = counts[3]
        # gather and build run on the stream current now, like every upload and build of a DeviceGraph; on a
        # stream other than the one the table (the index) was allocated on, their memory is recorded as used by it
        stream = torch.cuda.current_stream(device)
        if stream.cuda_stream != self.rows._home:
            self.rows._idx.record_stream(stream)
        t._use_on(stream)
        buf = torch.empty(total, dtype=torch.uint8, device=device)
        buf[off[0]:off[0] + 16 * B].copy_(host[h_mols:h_mols + 16 * B], non_blocking=True)
        # (blocks and block_nnz lie as far apart in the pinned image as in the device image: one copy)
        buf[off[4]:off[5] + 8 * n_blocks].copy_(host[h_blocks:h_nnz + 8 * n_blocks], non_blocking=True)
        del host
        base = buf.data_ptr()
        c = _native.WdGatherCompact()
        c.n_mols, c.n_rows, c.n_slots, c.slot0 = B, len(self.rows), t.n_slots, self.slot0
        c.t_atoms, c.t_pairs, c.t_xn = t._d_atoms.data_ptr(), t._d_pairs.data_ptr(), t._d_xn.data_ptr()
        c.t_first, c.ids = t._d_first.data_ptr(), self.rows._idx.data_ptr()
        c.mols, c.xn, c.atoms, c.pairs = base + off[0], base + off[1], base + off[2], base + off[3]
        _native.check(_native.lib().wdmpnn_gather_compact(ctypes.byref(c), stream.cuda_stream), 'gather compact')
        dg = build_from_image(device, buf, (True, counts, off, total), blk_max, *g._compact_dims,
                              max_num_bonds=g.max_num_bonds if atom_messages else None)
        dg.h2d_bytes = 16 * B + (off[5] - off[4]) + 8 * n_blocks
        dg.gathered = True
        return dg


def _device(device) -> torch.device:
    """``device`` with its index filled in (``cuda`` is the current GPU), so that two spellings compare equal."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def _pad_atom() -> bytes:
    """``compact::pad_atom()``: no columns (0xFF), last = 0, w = 0."""
    return b'\xff' * 8 + b'\x00' * 8
