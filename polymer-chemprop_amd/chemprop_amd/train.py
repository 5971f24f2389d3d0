"""Training-step counterpart of the reference loop.

* ``train_step`` / ``train`` follow ``chemprop/train/train.py:17-113``: mask / targets from
  ``None`` entries, target and data weights, ``loss_func(preds, targets) * w_t * w_d * mask``,
  ``loss.sum() / mask.sum()``, backward, optional ``clip_grad_norm_``, ``optimizer.step()``,
  per-batch scheduler step; plus the DP all-reduce of :mod:`chemprop_amd.dp` between backward and
  the optimizer step.
* ``NoamLR`` restates ``chemprop/nn_utils.py:115-194``; ``get_loss_func`` ``utils.py:338-364``
  (regression / classification / multiclass / spectra); ``build_optimizer`` ``utils.py:295-310``.
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn
from torch.optim import Adam, Optimizer
from torch.optim.lr_scheduler import _LRScheduler

from . import _native
from .dp import GradBucket
from .features import features_width, is_device_features, join_features, split_columns  # noqa: F401 (join_features: public)


class NoamLR(_LRScheduler):
    """nn_utils.py:115-194: linear warm-up from init_lr to max_lr over warmup_epochs, then
    exponential decay to final_lr at total_epochs."""

    def __init__(self, optimizer: Optimizer, warmup_epochs: List[Union[float, int]], total_epochs: List[int],
                 steps_per_epoch: int, init_lr: List[float], max_lr: List[float], final_lr: List[float]):
        assert len(optimizer.param_groups) == len(warmup_epochs) == len(total_epochs) == len(init_lr) == \
            len(max_lr) == len(final_lr)
        self.num_lrs = len(optimizer.param_groups)
        self.optimizer = optimizer
        self.warmup_epochs = np.array(warmup_epochs)
        self.total_epochs = np.array(total_epochs)
        self.steps_per_epoch = steps_per_epoch
        self.init_lr = np.array(init_lr)
        self.max_lr = np.array(max_lr)
        self.final_lr = np.array(final_lr)
        self.current_step = 0
        self.lr = init_lr
        self.warmup_steps = (self.warmup_epochs * self.steps_per_epoch).astype(int)
        self.total_steps = self.total_epochs * self.steps_per_epoch
        self.linear_increment = (self.max_lr - self.init_lr) / self.warmup_steps
        self.exponential_gamma = (self.final_lr / self.max_lr) ** (1 / (self.total_steps - self.warmup_steps))
        super(NoamLR, self).__init__(optimizer)

    def get_lr(self) -> List[float]:
        return list(self.lr)

    def step(self, current_step: int = None):
        self.current_step = self.current_step + 1 if current_step is None else current_step
        for i in range(self.num_lrs):
            if self.current_step <= self.warmup_steps[i]:
                self.lr[i] = self.init_lr[i] + self.current_step * self.linear_increment[i]
            elif self.current_step <= self.total_steps[i]:
                self.lr[i] = self.max_lr[i] * (self.exponential_gamma[i] ** (self.current_step - self.warmup_steps[i]))
            else:
                self.lr[i] = self.final_lr[i]
            self.optimizer.param_groups[i]['lr'] = self.lr[i]


def get_loss_func(dataset_type: str, alternative_loss_function: Optional[str] = None) -> Callable:
    """utils.py:338-364.  Spectra: ``spectra_utils.sid_loss``, or ``wasserstein_loss`` for
    ``alternative_loss_function='wasserstein'`` (the one alternative loss the reference has), both
    ``(preds, targets, mask)``; the other dataset types have no alternative."""
    if alternative_loss_function is not None and \
            not (dataset_type == 'spectra' and alternative_loss_function == 'wasserstein'):
        raise ValueError(f'Alternative loss function "{alternative_loss_function}" not supported with dataset type '
                         f'"{dataset_type}".')
    if dataset_type == 'spectra':
        from .spectra_utils import sid_loss, wasserstein_loss
        return wasserstein_loss if alternative_loss_function == 'wasserstein' else sid_loss
    if dataset_type == 'classification':
        return nn.BCEWithLogitsLoss(reduction='none')
    if dataset_type == 'regression':
        return nn.MSELoss(reduction='none')
    if dataset_type == 'multiclass':
        return nn.CrossEntropyLoss(reduction='none')
    raise ValueError(f'Dataset type "{dataset_type}" not supported.')


# the direct training step's packed weights rewritten by HipAdam's own pass (wdmpnn_adam_step_repack);
# False: a pack launch before every training forward (the A/B and test switch)
ADAM_REPACK = True


class HipAdam(Optimizer):
    """torch.optim.Adam / AdamW (no amsgrad, no maximize) whose update is ONE HIP launch per 16
    parameters (``wdmpnn_adam_step``): torch's fused Adam kernel took 40 us per training step for the
    355 k parameters of the default model (profiles/round2_train_kernel_trace_v2.txt), this one a few.
    Same per-element arithmetic as torch's fused Adam; lr / weight_decay / betas / eps are read from the
    param groups at every step, so schedulers (NoamLR) work unchanged.  State per parameter:
    ``step`` (int), ``exp_avg``, ``exp_avg_sq`` (as torch's Adam).  Writes its parameters through raw
    pointers (no version-counter bump): the encoders' packed-weight caches are keyed on the optimizer-step
    count instead.  A write of an encoder parameter through ``.data`` between steps needs
    ``MPNEncoder.invalidate_packed_params()``."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 decoupled: bool = False):
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or weight_decay < 0.0:
            raise ValueError('invalid Adam hyperparameter')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.decoupled = bool(decoupled)
        self._tables = {}  # parameter pointers of one launch -> its ctypes tensor table
        self._repack = None  # [(encoder, its training pack)] for the next step (train_step's direct path)

    def repack_next(self, *encoders) -> None:
        """Have the next :meth:`step` also rewrite every given encoder's training pack (the packed weight copies
        its direct training forward reads) from the updated weights, instead of a pack launch before the next
        forward (``wdmpnn_adam_step_repack``).  No effect for an encoder whose six weights are not updated in
        one call of that step.  With several encoders (a model of several molecules per input) the step's tensor
        table is split: one ``wdmpnn_adam_step_repack`` call per encoder over that encoder's weights and one
        ``wdmpnn_adam_step`` call for the rest (Adam is element-wise: the values do not depend on the split).  A
        shared encoder is one encoder."""
        pend = []
        if ADAM_REPACK:
            for enc in encoders:
                tp = enc.__dict__.get('_train_pack')
                if tp is not None and all(tp is not q for _, q in pend):
                    pend.append((enc, tp))
        self._repack = pend or None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _native.lib()
        state = self.state
        rp, self._repack = self._repack, None
        for group in self.param_groups:
            ps = [(p, state[p]) for p in group['params'] if p.grad is not None]
            if not ps:
                continue
            # torch's Adam keeps one step count per parameter: a parameter that had no gradient on some
            # steps lags behind the others, so the launches are grouped by step count (usually one group)
            by_step = {}
            for p, st in ps:
                if 'exp_avg' not in st:
                    if p.device.type != 'cuda' or p.dtype != torch.float32 or not p.is_contiguous():
                        raise TypeError('HipAdam expects contiguous float32 CUDA parameters')
                    st['step'] = 0
                    st['exp_avg'] = torch.zeros_like(p)
                    st['exp_avg_sq'] = torch.zeros_like(p)
                by_step.setdefault(int(st['step']) + 1, []).append((p, st))
            for step, sub in by_step.items():
                key = tuple(p.data_ptr() for p, _ in sub)
                tab = self._tables.get(key)
                if tab is None:
                    tab = (_native.WdAdamTensor * len(sub))()
                    for k, (p, st) in enumerate(sub):
                        tab[k].param, tab[k].exp_avg, tab[k].exp_avg_sq = p.data_ptr(), st['exp_avg'].data_ptr(), \
                            st['exp_avg_sq'].data_ptr()
                        tab[k].numel = p.numel()
                    self._tables[key] = tab
                for k, (p, st) in enumerate(sub):
                    g = p.grad
                    if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous():
                        raise TypeError('HipAdam expects dense contiguous float32 gradients')
                    tab[k].grad = g.data_ptr()
                    st['step'] = step
                h = _native.WdAdamHyper(float(group['lr']), float(group['betas'][0]), float(group['betas'][1]),
                                        float(group['eps']), float(group['weight_decay']), step, int(self.decoupled))
                sid = _native.current_stream(sub[0][0].device)
                if rp:
                    ptrs = frozenset(key)
                    now = [(e, tp) for e, tp in rp if tp['ptrs'] <= ptrs and tp['key'][-1] == sid]
                    if len(now) > 1:
                        rp = [q for q in rp if all(q is not r for r in now)]
                        self._step_split(L, tab, sub, key, h, now, sid)
                        continue
                    if now:
                        enc, tp = now[0]
                        rp = [q for q in rp if q is not now[0]]
                        rc = L.wdmpnn_adam_step_repack(tab, len(sub), ctypes.byref(h), ctypes.byref(tp['gs']),
                                                       ctypes.byref(tp['p']), ctypes.byref(tp['cfg']),
                                                       tp['buf'].data_ptr(), tp['buf'].numel(), sid)
                        if rc != _native.ERR_UNSUPPORTED:
                            _native.check(rc, 'adam step + repack')
                            enc._repacked_by_optimizer(tp)
                            continue
                _native.check(L.wdmpnn_adam_step(tab, len(sub), ctypes.byref(h), sid), 'adam step')
        return loss

    def _step_split(self, L, tab, sub, key, h, now, sid) -> None:
        """One step-count group with several encoders to repack: a sub-table and a ``wdmpnn_adam_step_repack`` call
        per encoder, one ``wdmpnn_adam_step`` call for the remaining tensors.  The sub-tables are cached next to
        the group's table (their gradient pointers are copied from it every step)."""
        skey = (key, tuple(tuple(sorted(tp['ptrs'])) for _, tp in now))
        parts = self._tables.get(skey)
        if parts is None:
            taken, parts = set(), []
            for _, tp in now:
                rows = [k for k, (p, _) in enumerate(sub) if p.data_ptr() in tp['ptrs'] and k not in taken]
                taken.update(rows)
                parts.append(rows)
            parts.append([k for k in range(len(sub)) if k not in taken])
            parts = [(rows, (_native.WdAdamTensor * max(len(rows), 1))()) for rows in parts]
            self._tables[skey] = parts
        for rows, t in parts:
            for j, k in enumerate(rows):
                t[j] = tab[k]
        for (enc, tp), (rows, t) in zip(now, parts):
            rc = L.wdmpnn_adam_step_repack(t, len(rows), ctypes.byref(h), ctypes.byref(tp['gs']), ctypes.byref(tp['p']),
                                           ctypes.byref(tp['cfg']), tp['buf'].data_ptr(), tp['buf'].numel(), sid)
            if rc == _native.ERR_UNSUPPORTED:  # (this encoder packs before its next forward)
                rc = L.wdmpnn_adam_step(t, len(rows), ctypes.byref(h), sid)
                _native.check(rc, 'adam step')
                continue
            _native.check(rc, 'adam step + repack')
            enc._repacked_by_optimizer(tp)
        rows, t = parts[-1]
        if rows:
            _native.check(L.wdmpnn_adam_step(t, len(rows), ctypes.byref(h), sid), 'adam step')

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._tables.clear()  # the moment buffers were replaced: rebuild the pointer tables


def build_optimizer(model: nn.Module, args=1e-4, weight_decay: float = 0.0) -> Optimizer:
    """utils.py:295-310: Adam (or AdamW when ``args.optimizer == 'adamw'``) over all parameters.
    ``args`` is a TrainArgs-like object (``init_lr``, optional ``weight_decay`` / ``optimizer``) as in
    the reference, or a plain learning rate.  On a GPU the update runs as :class:`HipAdam` (same update
    rule, one HIP launch per step)."""
    if isinstance(args, (int, float)):
        lr, wd, kind = float(args), weight_decay, 'adam'
    else:
        lr, wd, kind = args.init_lr, getattr(args, 'weight_decay', 0.0), getattr(args, 'optimizer', 'adam')
    params = list(model.parameters())
    groups = [{'params': params, 'lr': lr, 'weight_decay': wd}]
    if bool(params) and all(p.device.type == 'cuda' and p.dtype == torch.float32 for p in params):
        return HipAdam(groups, lr=lr, weight_decay=wd, decoupled=kind == 'adamw')
    if kind == 'adamw':
        return torch.optim.AdamW(groups)
    return Adam(groups)


# pinned host tables of batch_loss, a ring of _PINNED_RING per (device, shape): allocating pinned memory
# every step costs more than the rest of the loss.  A buffer is refilled after the event of its last copy,
# which with a ring is several steps old (one buffer made every step wait for the previous step's forward:
# the host could not run ahead of the GPU)
_PINNED_TABLES = {}
_PINNED_RING = 4


def _host_table(rows: np.ndarray, dev: torch.device, zero_copy: bool = False):
    """rows (float32 [B][2T]) -> device tensor through a reused pinned buffer (asynchronous copy).
    ``zero_copy``: no copy; returns (device address of the pinned buffer, its event) or None when the
    buffer is not mapped for the device -- the caller's kernel reads the rows over PCIe, and the caller
    records the event after that kernel's launch (the buffer is refilled only after it)."""
    if dev.type != 'cuda':
        return None if zero_copy else torch.from_numpy(rows).to(dev)
    key = (dev, rows.shape, zero_copy)
    ring = _PINNED_TABLES.get(key)
    if ring is None:
        ring = _PINNED_TABLES[key] = [0, [None] * _PINNED_RING]
    i = ring[0]
    ring[0] = (i + 1) % _PINNED_RING
    ent = ring[1][i]
    if ent is None:
        if zero_copy:
            # the kernel reads the rows in place: coherent mapped memory (torch's pinned buffers are
            # non-coherent, and a rewritten slot read again at the same device address would then rely
            # on the dispatch invalidating stale L2 lines)
            cb = _native.CoherentHostBuffer(rows.shape)
            ent = ring[1][i] = (cb, torch.cuda.Event(), cb.device_ptr)
        else:
            buf = torch.empty(rows.shape, dtype=torch.float32, pin_memory=True)
            ent = ring[1][i] = (buf, torch.cuda.Event(), 0)
    else:
        ent[1].synchronize()  # (this buffer's last reader, _PINNED_RING steps ago)
    buf, ev, dptr = ent
    if zero_copy:
        buf.array[...] = rows
        return (dptr, ev) if dptr else None
    buf.numpy()[...] = rows
    table = buf.to(dev, non_blocking=True)
    ev.record(torch.cuda.current_stream(dev))
    return table


def _targets_and_mask(target_batch, nan_missing: bool = False):
    """train.py:46-48 on the host: (targets with 0 for the missing ones, mask), float64 [B][T].
    ``nan_missing`` (spectra): a float ``ndarray`` [B][T] is taken as it is with NaN = missing: no per-element
    Python work (a spectra batch of 64 x 1801 lists with ``None`` entries costs 15 ms here, its array 0.3 ms)."""
    if nan_missing and isinstance(target_batch, np.ndarray) and target_batch.dtype.kind == 'f' and \
            target_batch.ndim == 2:
        present = ~np.isnan(target_batch)
        return np.where(present, target_batch, 0.0).astype(np.float64), present.astype(np.float64)
    n_b = len(target_batch)
    n_t = len(target_batch[0]) if n_b else 0
    # missing targets are None (train.py:47-48); numpy's float conversion would turn them into NaN, so the
    # mask comes from an object array (a NaN target stays a NaN, as in the reference).  Fast path: a batch
    # that converts to floats without any NaN had neither (mask of ones, the same table)
    tgt = None
    try:
        tgt = np.asarray(target_batch, dtype=np.float64)
        if tgt.shape != (n_b, n_t) or np.isnan(tgt).any():
            tgt = None
    except (TypeError, ValueError):
        tgt = None
    if tgt is not None:
        mask = np.ones((n_b, n_t))
    else:
        obj = np.array(target_batch, dtype=object).reshape(n_b, n_t)
        present = obj != None  # noqa: E711 (elementwise)
        tgt = np.where(present, obj, 0.0).astype(np.float64)
        mask = present.astype(np.float64)
    return tgt, mask


def _check_class_indices(tgt: np.ndarray, mask: np.ndarray, num_classes: int) -> None:
    """Every present target must be a class index: an integer in [0, num_classes).  torch's own check
    (nll_loss) is a device-side assert that takes the process's GPU context down; this one runs on the
    host before anything is launched."""
    ok = (tgt == np.floor(tgt)) & (tgt >= 0) & (tgt < num_classes)  # (NaN compares false)
    bad = (mask > 0) & ~ok
    if bad.any():
        r, t = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f'multiclass target {tgt[r, t]!r} in row {r}, task {t} is not an integer class index in '
                         f'[0, {num_classes})')


def check_class_targets(target_batch, num_classes: int) -> None:
    """Raise ValueError unless every target of ``target_batch`` ([B][tasks], None = missing) is an integer
    class index in [0, num_classes); the message names the first offending row and task."""
    if len(target_batch):
        _check_class_indices(*_targets_and_mask(target_batch), num_classes)


def _spectra_targets_ok(tgt: np.ndarray, mask: np.ndarray) -> bool:
    """Every present target is finite and > 0 (one pass: a finite positive value times a mask of 0 / 1 is > 0
    exactly where the mask is 1; NaN and inf fail the comparisons)."""
    with np.errstate(invalid='ignore'):
        return bool(((tgt > 0) & (tgt < np.inf)).sum() == int(mask.sum()) and not ((mask == 0) & (tgt != 0)).any())


def _check_spectra_targets(tgt: np.ndarray, mask: np.ndarray) -> None:
    """Every present spectra target must be finite and greater than 0 (``normalize_spectra`` with the target
    floor leaves them so): the table marks a missing target with 0, and the losses take its logarithm."""
    with np.errstate(invalid='ignore'):
        bad = (mask > 0) & ~(np.isfinite(tgt) & (tgt > 0))
    if bad.any():
        r, t = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f'spectra target {tgt[r, t]!r} in row {r}, column {t} is not finite and greater than 0 '
                         '(normalize the targets with a positive floor first)')


def check_spectra_targets(target_batch) -> None:
    """Raise ValueError unless every present target of ``target_batch`` ([B][T], None = missing) is finite and
    greater than 0; the message names the first offending row and column."""
    if len(target_batch):
        _check_spectra_targets(*_targets_and_mask(target_batch))


def _loss_table(target_batch, target_weights, data_weights, dev, zero_copy: bool = False, num_classes: int = 0,
                spectra: bool = False):
    """train.py:46-74's targets and weights as one device table [B][2T] (targets | w = target weight *
    data weight * mask, rounded once to fp32) and the host count mask.sum().  ``num_classes`` > 0
    (multiclass): the targets are class indices, checked on the host (``_check_class_indices``).
    ``spectra``: a target of 0 in the table means "missing" (the mask of the spectra losses, which is not the
    weight's: a present target with weight 0 still counts in the row's sum); every present target is checked
    to be finite and > 0 (``_check_spectra_targets``) and must still be nonzero once rounded to fp32."""
    n_b = len(target_batch)
    n_t = len(target_batch[0]) if n_b else 0
    tgt, mask = _targets_and_mask(target_batch, spectra)
    if num_classes and n_b:
        _check_class_indices(tgt, mask, num_classes)
    if spectra and n_b:  # (as rounded to fp32: a present target that rounds to 0 would go missing)
        if not _spectra_targets_ok(tgt.astype(np.float32), mask):
            _check_spectra_targets(tgt, mask)
            _check_spectra_targets(tgt.astype(np.float32), mask)
    tw = np.ones(n_t) if target_weights is None else np.asarray(target_weights, dtype=np.float64)
    dw = np.ones(n_b) if data_weights is None else np.asarray(data_weights, dtype=np.float64)
    # targets and W travel as one host table (one pinned, asynchronous copy: pageable copies would each
    # stall the host until the forward has drained)
    rows = np.concatenate([tgt, tw[None, :] * dw[:, None] * mask], axis=1).astype(np.float32)
    if zero_copy:
        return _host_table(rows, dev, True), n_t, int(mask.sum()), rows.shape
    return _host_table(rows, dev), n_t, int(mask.sum())


def batch_loss(preds: torch.Tensor, target_batch: Sequence[Sequence[Optional[float]]], loss_func: Callable,
               dataset_type: str = 'regression', target_weights: Sequence[float] = None,
               data_weights: Sequence[float] = None) -> torch.Tensor:
    """train.py:46-74: ``(loss_func(preds, targets) * target_weights * data_weights * mask).sum() /
    mask.sum()``.  The three weight factors are multiplied on the host into one weight table W, and
    ``mask.sum()`` is a host count: two fewer device ops forward and backward, the same loss (W is
    rounded once to fp32 instead of twice)."""
    table, n_t, n_mask = _loss_table(target_batch, target_weights, data_weights, preds.device,
                                     spectra=dataset_type == 'spectra')
    targets, w = table[:, :n_t], table[:, n_t:]
    if dataset_type == 'spectra':  # train.py:70-71: the loss takes the mask (the table's "0 = missing")
        loss = loss_func(preds, targets, targets != 0) * w
    elif dataset_type == 'multiclass':
        targets = targets.long()
        loss = torch.cat([loss_func(preds[:, j, :], targets[:, j]).unsqueeze(1) for j in range(preds.size(1))],
                         dim=1) * w
    else:
        loss = loss_func(preds, targets) * w
    return loss.sum() / float(n_mask)


# ------------------------------------------------------------------------------------------------
# Fused FFN head + masked MSE loss (wdmpnn_head_mse).  The reference's step evaluates ffn(emb) (model.py:
# 57-121), loss_func(preds, targets) * weights and .sum() / mask.sum() (train.py:55-74) and autograd runs
# their backward: ~25 small torch ops whose host time left the GPU idle for most of the step
# (profiles/round2_train_kernel_trace_v3.txt).  For the default head (two Linear layers, an activation, no
# active dropout; MSELoss for regression, BCEWithLogitsLoss for classification, per-task CrossEntropyLoss for
# multiclass) the loss and every gradient of the head come from two HIP
# launches in the forward; the backward scales them by the loss's incoming gradient (one launch).
# Every other FFN of create_ffn with at most 64 outputs (one or up to six Linear layers, dropout active
# while training, PReLU with its single shared slope) runs the stack head (wdmpnn_head_stack, _StackHead):
# 2 L - 1 launches, dropout masks from the counter hash of nn_utils.dropout_mask under one seed per step.
# ------------------------------------------------------------------------------------------------
def _head_act(m: nn.Module) -> Optional[int]:
    """WdActivation of an FFN activation module the fused head supports (not PReLU), else None."""
    if type(m) is nn.ReLU:
        return 0
    if type(m) is nn.LeakyReLU and m.negative_slope == 0.1:
        return 1
    if type(m) is nn.Tanh:
        return 3
    if type(m) is nn.SELU:
        return 4
    if type(m) is nn.ELU and m.alpha == 1.0:
        return 5
    return None


def _fusable_head(model: nn.Module, loss_func: Callable, dataset_type: str):
    """(Linear 1, Linear 2, activation code, loss kind, classes per task) when the step's head + loss can
    run fused, else None.  Classes per task is 1 but for multiclass (kind 2)."""
    n_classes = 1
    if dataset_type == 'regression' and type(loss_func) is nn.MSELoss and loss_func.reduction == 'none':
        kind = 0
    elif dataset_type == 'classification' and type(loss_func) is nn.BCEWithLogitsLoss and \
            loss_func.reduction == 'none' and loss_func.weight is None and loss_func.pos_weight is None:
        kind = 1  # (the FFN's logits: MoleculeModel applies the sigmoid only outside training, model.py:186-188)
    elif dataset_type == 'multiclass' and type(loss_func) is nn.CrossEntropyLoss and \
            loss_func.reduction == 'none' and loss_func.weight is None and loss_func.ignore_index == -100 and \
            loss_func.label_smoothing == 0:
        kind = 2  # (one softmax cross-entropy per task over its num_classes logits, train.py:67-69)
        n_classes = getattr(model, 'num_classes', 0) if getattr(model, 'multiclass', False) else 0
        if not isinstance(n_classes, int) or n_classes < 2:
            return None
    elif dataset_type == 'spectra':
        from .spectra_utils import sid_loss, wasserstein_loss
        if loss_func is not sid_loss and loss_func is not wasserstein_loss:
            return None
        st = _head_structure(model)  # (always the spectra entry point: no two-layer tuple path)
        if st is None or _head_parts(st)[5] is None:
            return None
        return st.with_kind(1 if loss_func is wasserstein_loss else 0, 1)
    else:
        return None
    st = _head_structure(model)
    if st is None:
        return None
    if type(st) is tuple and kind != 2:  # (the every-step case: nothing of the head to look at)
        return st + (kind, n_classes)
    linears, _, _, _, _, spectra = _head_parts(st)
    if spectra is not None:
        return None
    n_out = linears[-1].out_features
    if kind == 2 and (n_out % n_classes or n_out != getattr(model, 'output_size', -1)):
        return None
    return st + (kind, n_classes) if type(st) is tuple else st.with_kind(kind, n_classes)


class _StackHead:
    """An FFN the native stack head runs (``wdmpnn_head_stack``): its ``Linear`` layers, the activation code,
    the shared PReLU slope (or None), the dropout probability active now, and the loss or output kind with its
    classes per task (set by ``with_kind``).  ``spectra``: None, or the output activation of a spectra FFN
    (0 exp, 1 softplus): such a head runs ``wdmpnn_head_spectra`` and its kind is the spectra loss (0 SID,
    1 Wasserstein)."""
    __slots__ = ('linears', 'act', 'slope', 'p', 'kind', 'n_classes', 'spectra')

    def __init__(self, linears, act, slope, p, kind=None, n_classes=1, spectra=None):
        self.linears, self.act, self.slope, self.p, self.kind, self.n_classes = linears, act, slope, p, kind, n_classes
        self.spectra = spectra

    def with_kind(self, kind: int, n_classes: int) -> '_StackHead':
        return _StackHead(self.linears, self.act, self.slope, self.p, kind, n_classes, self.spectra)

    def params(self) -> list:
        """W_1, b_1, ..., W_L, b_L (None for an absent bias), then the slope (or None)."""
        out = []
        for l in self.linears:
            out += [l.weight, l.bias]
        return out + [self.slope]


def _head_parts(head):
    """(linears, act, slope, kind, n_classes, spectra) of a head in either form: the two-layer tuple of
    ``_head_structure`` (kind None) or of ``_fusable_head`` / ``_predict_head``, or a :class:`_StackHead`.  The
    one place that tells the two apart to read them."""
    if isinstance(head, _StackHead):
        return head.linears, head.act, head.slope, head.kind, head.n_classes, head.spectra
    if len(head) == 5:
        l1, l2, act, kind, n_classes = head
        return (l1, l2), act, None, kind, n_classes, None
    return head[:2], head[2], None, None, 1, None


HEAD_MAX_WIDTH, HEAD_MAX_OUTPUTS = 4096, 64  # (wdmpnn.h: F, Hf <= 4096, T <= 64)


def _spectra_act(m: nn.Module) -> Optional[int]:
    """WdHeadSpectra.spectra_act of a spectra FFN's output activation (create_ffn: ``_Exp`` or ``nn.Softplus``
    with its defaults), else None."""
    from .model import _Exp
    if type(m) is _Exp:
        return 0
    if type(m) is nn.Softplus and m.beta == 1 and m.threshold == 20:
        return 1  # (beyond the threshold torch returns z itself: within 2.1e-9 of log1p(exp(z)))
    return None


def _ffn_structure(ffn: nn.Module, training: bool, spectra: bool = False) -> Optional[_StackHead]:
    """The structure of an FFN built by ``MoleculeModel.create_ffn`` within the native head's limits, else None:
    Dropout, Linear, then (activation, Dropout, Linear) up to ``HEAD_MAX_LAYERS`` Linear layers in all, every
    Dropout with one probability (< 1), one activation (the same module at every site, as create_ffn builds it:
    a PReLU must have a single slope), hidden layers of one width, widths <= 4096 and <= 64 outputs.  Devices
    and dtypes are not looked at (``_head_structure`` does).  ``spectra``: the FFN of a spectra model, the same
    stack followed by its output activation (``_Exp`` or ``nn.Softplus``), with up to ``HEAD_MAX_SPECTRUM``
    outputs; without it a trailing activation is not recognised."""
    if not isinstance(ffn, nn.Sequential):
        return None
    mods = list(ffn)
    s_act = None
    if spectra:
        s_act = _spectra_act(mods[-1]) if mods else None
        if s_act is None:
            return None
        mods = mods[:-1]
    if len(mods) < 2 or len(mods) % 3 != 2 or len(mods) // 3 + 1 > _native.HEAD_MAX_LAYERS:
        return None
    drops, linears, acts = mods[0::3], mods[1::3], mods[2::3]
    if any(type(d) is not nn.Dropout for d in drops) or any(type(l) is not nn.Linear for l in linears):
        return None
    p = drops[0].p
    if any(d.p != p for d in drops) or not 0 <= p < 1:
        return None
    code, slope = _native.ACT_IDENTITY, None  # (a one-layer FFN has no activation site)
    if acts:
        act = acts[0]
        if any(a is not act for a in acts):
            return None
        if type(act) is nn.PReLU:
            if act.num_parameters != 1:
                return None
            code, slope = 2, act.weight
        else:
            code = _head_act(act)
            if code is None:
                return None
    width = linears[0].in_features
    hidden = linears[0].out_features
    for i, l in enumerate(linears):
        if l.in_features != width or l.in_features > HEAD_MAX_WIDTH:
            return None
        if i < len(linears) - 1 and l.out_features != hidden:
            return None
        width = l.out_features
    if linears[-1].out_features > (_native.HEAD_MAX_SPECTRUM if spectra else HEAD_MAX_OUTPUTS):
        return None
    return _StackHead(linears, code, slope, float(p) if training else 0.0, spectra=s_act)


def _head_structure(model: nn.Module):
    """The FFN of a MoleculeModel as the native head kernels run it, else None: (Linear 1, Linear 2,
    activation code) for the two-layer head without active dropout or PReLU (``wdmpnn_head_mse`` /
    ``wdmpnn_head_predict``), a :class:`_StackHead` (kind unset) for every other FFN ``_ffn_structure``
    recognises; float32 contiguous parameters on the GPU."""
    from .model import MoleculeModel
    if not isinstance(model, MoleculeModel) or type(model).forward is not MoleculeModel.forward:
        return None
    spectra = bool(getattr(model, 'spectra', False))
    st = None if spectra else _two_layer_structure(model)
    if st is not None:
        return st
    st = _ffn_structure(model.ffn, model.training, spectra)  # (spectra: a _StackHead with ``spectra`` set)
    if st is None:
        return None
    for t in st.params():
        if t is not None and (t.device.type != 'cuda' or t.dtype != torch.float32 or not t.is_contiguous()):
            return None
    return st


def _two_layer_structure(model: nn.Module):
    """(Linear 1, Linear 2, activation code) of the two-layer head (Dropout / Linear / activation / Dropout /
    Linear on the GPU, no dropout while training, no PReLU, at most 64 outputs), else None."""
    ffn = model.ffn
    if len(ffn) != 5:
        return None
    d0, l1, act, d1, l2 = ffn
    if type(d0) is not nn.Dropout or type(d1) is not nn.Dropout or type(l1) is not nn.Linear \
            or type(l2) is not nn.Linear:
        return None
    if model.training and (d0.p > 0 or d1.p > 0):
        return None
    code = _head_act(act)
    if code is None:
        return None
    for t in (l1.weight, l1.bias, l2.weight, l2.bias):
        if t is not None and (t.device.type != 'cuda' or t.dtype != torch.float32 or not t.is_contiguous()):
            return None
    if l1.in_features > 4096 or l1.out_features > 4096 or l2.out_features > 64:
        return None
    return l1, l2, code


def _run_head_two(x: torch.Tensor, head, tab_ptr: int, ld_table: int, inv_n: float, grad_of: Callable):
    """One ``wdmpnn_head_mse`` call on the encodings x [B][F] (contiguous) for the two-layer 5-tuple:
    (loss, dx, (dW1, db1, dW2, db2)), None for an absent bias.  ``grad_of(parameter)`` gives the buffer each
    gradient is written into (this entry point computes them all)."""
    l1, l2, act, kind, n_classes = head
    W1, b1, W2, b2 = l1.weight, l1.bias, l2.weight, l2.bias
    dev = x.device
    B, F = x.shape
    Hf, T = W1.shape[0], W2.shape[0]
    scratch = torch.empty(B * (2 * Hf + T + 1), dtype=torch.float32, device=dev)
    dx = torch.empty_like(x)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dW1, dW2 = grad_of(W1), grad_of(W2)
    db1 = grad_of(b1) if b1 is not None else None
    db2 = grad_of(b2) if b2 is not None else None
    ptr = _native.ptr
    sp = scratch.data_ptr()
    h = _native.WdHead(ptr(x), F, B, F, Hf, T, ptr(W1), ptr(b1), ptr(W2), ptr(b2), tab_ptr, ld_table,
                       float(inv_n), act, sp, sp + 4 * B * Hf, sp + 8 * B * Hf, sp + 4 * B * (2 * Hf + T),
                       ptr(dx), ptr(dW1), ptr(db1), ptr(dW2), ptr(db2), ptr(loss), kind, n_classes)
    _native.check(_native.lib().wdmpnn_head_mse(ctypes.byref(h), _native.current_stream(dev)), 'FFN head + loss')
    return loss, dx, (dW1, db1, dW2, db2)


class _HeadMSE(torch.autograd.Function):
    """loss = sum(w (W2 act(W1 x + b1) + b2 - y)^2) / n, with every gradient computed in the forward.  ``head``
    is the two-layer 5-tuple; W1, b1, W2, b2 are its parameters: autograd needs them as inputs to hand their
    gradients out."""

    @staticmethod
    def forward(ctx, x, head, table, inv_n, W1, b1, W2, b2):
        loss, dx, grads = _run_head_two(x.contiguous(), head, table.data_ptr(), table.shape[1], inv_n,
                                        torch.empty_like)
        ctx.grads = (dx,) + grads
        return loss

    @staticmethod
    def backward(ctx, gl):
        grads, ctx.grads = ctx.grads, None  # (sole owner: autograd adopts the tensors instead of copying)
        _scale_all(grads, gl)
        return (grads[0], None, None, None) + grads[1:]


def _scale_all(grads, gl: torch.Tensor) -> None:
    """Every gradient times the loss's incoming gradient: wdmpnn_scale, 8 buffers per launch."""
    live = [g for g in grads if g is not None]
    gl = gl.to(torch.float32).contiguous()
    for i in range(0, len(live), 8):
        part = live[i:i + 8]
        ptrs = (ctypes.c_void_p * len(part))(*[g.data_ptr() for g in part])
        ns = (ctypes.c_int64 * len(part))(*[g.numel() for g in part])
        _native.check(_native.lib().wdmpnn_scale(ptrs, ns, len(part), gl.data_ptr(),
                                                 _native.current_stream(gl.device)), 'scale')


def _fill_ffn(h, x: torch.Tensor, linears, slope, act: int):
    """The FFN on the encodings x [B][F] (contiguous) written into the fields the stack and spectra structs
    share (``WdHeadStack``, ``WdHeadStackPredict``, ``WdHeadSpectra``, ``WdHeadSpectraPredict``, ``WdHeadLatent``); returns
    (B, F, Hf, T, L) as written (Hf 0 for one layer)."""
    B, F = x.shape
    L, T = len(linears), linears[-1].out_features
    Hf = linears[0].out_features if L > 1 else 0
    h.x, h.ld_x, h.B, h.F, h.Hf, h.L = x.data_ptr(), F, B, F, Hf, L
    if hasattr(h, 'T'):  # (WdHeadLatent stops below the last Linear: no outputs)
        h.T = T
    for i, l in enumerate(linears):
        h.W[i], h.b[i] = l.weight.data_ptr(), 0 if l.bias is None else l.bias.data_ptr()
    h.slope, h.act = 0 if slope is None else slope.data_ptr(), act
    return B, F, Hf, T, L


def _run_head_stack(x: torch.Tensor, head: _StackHead, tab_ptr: int, ld_table: int, inv_n: float, seed: int,
                    grad_of: Callable, want_dx: bool = True):
    """One ``wdmpnn_head_stack`` call on the encodings x [B][F] (contiguous): (loss, dx, the gradients in the
    order of ``head.params()``, None where the parameter is None).  ``grad_of(parameter)`` gives the buffer
    each gradient is written into, or None for a gradient nobody wants (a frozen parameter); ``want_dx``:
    whether d loss / d x is wanted (else dx is None).  With anything left out the call is
    ``wdmpnn_head_stack_partial``: the same outputs, bitwise, and no launch or workgroup for the rest."""
    dev = x.device
    spectra = head.spectra is not None  # (wdmpnn_head_spectra: the same fields, NULL gradients = not wanted)
    h = _native.WdHeadSpectra() if spectra else _native.WdHeadStack()
    B, F, Hf, T, L = _fill_ffn(h, x, head.linears, head.slope, head.act)
    nbytes = (_native.head_spectra_scratch_bytes if spectra else _native.head_stack_scratch_bytes)(B, F, Hf, T, L)
    scratch = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=dev)
    dx = torch.empty_like(x) if want_dx else None
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ptr = _native.ptr
    params = head.params()  # (W_1, b_1, ..., W_L, b_L, the slope)
    grads = [grad_of(t) if t is not None else None for t in params]
    for i in range(L):
        h.dW[i], h.db[i] = ptr(grads[2 * i]), ptr(grads[2 * i + 1])
    h.dslope = ptr(grads[2 * L])
    partial = not want_dx or any(g is None and t is not None for g, t in zip(grads, params))
    h.table, h.ld_table, h.inv_n = tab_ptr, ld_table, float(inv_n)
    h.p, h.seed, h.loss_kind = head.p, seed, head.kind
    if spectra:
        h.spectra_act = head.spectra
    else:
        h.n_classes = head.n_classes
    h.scratch, h.scratch_bytes = scratch.data_ptr(), scratch.numel() * 4
    h.dx, h.loss = ptr(dx), loss.data_ptr()
    if spectra:
        entry = _native.lib().wdmpnn_head_spectra
    else:
        entry = _native.lib().wdmpnn_head_stack_partial if partial else _native.lib().wdmpnn_head_stack
    _native.check(entry(ctypes.byref(h), _native.current_stream(dev)), 'FFN head stack + loss')
    return loss, dx, grads


class _HeadStack(torch.autograd.Function):
    """The loss of a :class:`_StackHead` on x, with every gradient computed in the forward (as ``_HeadMSE``).
    ``params`` are ``head.params()``: autograd needs them as inputs to hand their gradients out."""

    @staticmethod
    def forward(ctx, x, head, table, inv_n, seed, *params):
        # only the gradients autograd will ask for (a frozen parameter, a frozen encoder's output: none)
        need = ctx.needs_input_grad
        wanted = {id(t) for t, n in zip(params, need[5:]) if t is not None and n}
        loss, dx, grads = _run_head_stack(x.contiguous(), head, table.data_ptr(), table.shape[1], inv_n, seed,
                                          lambda t: torch.empty_like(t) if id(t) in wanted else None, need[0])
        ctx.grads = [dx] + grads
        return loss

    @staticmethod
    def backward(ctx, gl):
        grads, ctx.grads = ctx.grads, None
        _scale_all(grads, gl)
        return (grads[0], None, None, None, None) + tuple(grads[1:])


def _head_seed(head) -> int:
    """The head's dropout seed for this step: one ``_dropout_seed`` draw when its dropout is active (after the
    encoder's draw, on the direct and the autograd path alike), else 0."""
    if isinstance(head, _StackHead) and head.p > 0:
        from .mpn import _dropout_seed
        return _dropout_seed()
    return 0


def head_loss(emb: torch.Tensor, head, target_batch, target_weights=None, data_weights=None) -> torch.Tensor:
    """``batch_loss(model.ffn(emb), ...)`` for a head accepted by ``_fusable_head`` (regression with MSE,
    classification with BCE on logits, multiclass with one cross-entropy per task: the targets are then
    class indices, one per task, checked on the host).  A :class:`_StackHead` (deeper or one-layer FFN, active
    dropout, PReLU) runs ``wdmpnn_head_stack``; its dropout masks follow the counter hash of
    ``nn_utils.dropout_mask`` under one seed drawn here."""
    linears, _, _, kind, n_classes, spectra = _head_parts(head)
    spectra = spectra is not None
    table, n_t, n_mask = _loss_table(target_batch, target_weights, data_weights, emb.device,
                                     num_classes=n_classes if kind == 2 and not spectra else 0, spectra=spectra)
    inv_n = _check_head_batch(linears, n_classes, n_t, n_mask, table.shape[0], emb)
    if isinstance(head, _StackHead):
        return _HeadStack.apply(emb, head, table, inv_n, _head_seed(head), *head.params())
    l1, l2 = linears
    return _HeadMSE.apply(emb, head, table, inv_n, l1.weight, l1.bias, l2.weight, l2.bias)


def _check_head_batch(linears, n_classes: int, n_t: int, n_mask, n_rows: int, x: torch.Tensor) -> float:
    """A loss table (``_loss_table``: n_t targets per row, n_mask present targets, n_rows rows) against the
    head and its input x (``ValueError``); returns 1 / n_mask, the loss's normalisation (inf without targets)."""
    l1, l2 = linears[0], linears[-1]
    if n_t * n_classes != l2.out_features:
        raise ValueError(f'{n_t} targets per row for {l2.out_features} outputs')
    if n_rows != x.shape[0] or x.dim() != 2 or x.shape[1] != l1.in_features:
        raise ValueError(f'{n_rows} target rows for encodings of shape {tuple(x.shape)} '
                         f'(FFN input {l1.in_features})')
    return 1.0 / n_mask if n_mask else float('inf')


def _predict_head(model: nn.Module):
    """(Linear 1, Linear 2, activation code, output kind, classes per task) when ``head_predict`` can run
    the model's FFN and output activation (model.py:186-192), else None."""
    st = _head_structure(model)
    if st is None:
        return None
    n_out = _head_parts(st)[0][-1].out_features
    kind, c = 1 if getattr(model, 'classification', False) else 0, 1
    if getattr(model, 'multiclass', False):
        kind, c = 2, getattr(model, 'num_classes', 0)
        if not isinstance(c, int) or c < 2 or n_out % c:
            return None
    return st + (kind, c) if type(st) is tuple else st.with_kind(kind, c)


def _head_linears(head) -> list:
    """The Linear layers of a head of ``_fusable_head`` / ``_predict_head``, first to last."""
    return list(_head_parts(head)[0])


def _head_input(emb: torch.Tensor, l1: nn.Linear) -> torch.Tensor:
    """The encodings ``emb`` as the eval-mode heads read them (detached, contiguous); ``ValueError`` unless they
    are float32 ``[B][in_features]`` on the device of the FFN's first Linear ``l1``."""
    if emb.dim() != 2 or emb.shape[1] != l1.in_features or emb.device != l1.weight.device or \
            emb.dtype != torch.float32:
        raise ValueError(f'encodings of shape {tuple(emb.shape)} ({emb.dtype}, {emb.device}) for an FFN input of '
                         f'{l1.in_features} on {l1.weight.device}')
    return emb.detach().contiguous()


def head_predict(model: nn.Module, emb: torch.Tensor, head=None, normalize: bool = False,
                 mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The eval-mode predictions of ``model`` from the encodings ``emb`` (model.py:152-194 after the
    encoder: ``ffn``, then nothing for regression, the sigmoid for classification, the softmax over each
    task's classes for multiclass) as L HIP launches (``wdmpnn_head_stack_predict``; two for the two-layer
    head, whose tuple fills the same struct with L = 2).  ``[B][T]`` for
    regression and classification, ``[B][tasks][classes]`` for multiclass.  No autograd graph is built.
    The model must be in eval mode with an FFN the native heads run: any FFN of ``create_ffn`` with at most 64
    outputs; ``NotImplementedError`` otherwise: there is no torch fallback here.
    A spectra model (``wdmpnn_head_spectra_predict``, up to 8192 outputs) returns ``act_s(ffn)`` as its
    ``forward`` does, or with ``normalize`` every row divided by the sum of its included positions
    (``spectra_utils.normalize_spectra`` on the device): ``mask`` is a bool or uint8 ``[B][T]`` tensor on the
    device (nonzero = included; None = every position), and the excluded positions come back as NaN.
    ``normalize`` and ``mask`` are for spectra models only (``ValueError`` otherwise)."""
    if model.training:
        raise ValueError('head_predict is the eval-mode head: call model.eval() first')
    if head is None:
        head = _predict_head(model)
    if head is None:
        raise NotImplementedError('head_predict: the model\'s FFN is not one the native head runs (Dropout / Linear / '
                                  'activation stacks of create_ffn, <= 64 outputs, a single PReLU slope)')
    linears, act, slope, kind, n_classes, spectra = _head_parts(head)
    x = _head_input(emb, linears[0])
    dev = x.device
    if (normalize or mask is not None) and spectra is None:
        raise ValueError('head_predict: normalize / mask are for spectra models')
    h = _native.WdHeadStackPredict() if spectra is None else _native.WdHeadSpectraPredict()
    B, F, Hf, T, L = _fill_ffn(h, x, linears, slope, act)
    if mask is not None:
        if not normalize or tuple(mask.shape) != (B, T) or mask.device != dev or \
                mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'head_predict: mask of shape {tuple(mask.shape)} ({mask.dtype}, {mask.device}) for '
                             f'normalize={normalize} and outputs of shape {(B, T)} on {dev}')
        mask = mask.contiguous().view(torch.uint8)
    # the z_l; a spectrum's z_L - b_L behind them
    scratch = torch.empty(max((L - 1) * B * Hf + (0 if spectra is None else B * T), 4), dtype=torch.float32, device=dev)
    out = torch.empty((B, T), dtype=torch.float32, device=dev)
    h.scratch, h.scratch_bytes, h.out = scratch.data_ptr(), scratch.numel() * 4, out.data_ptr()
    if spectra is None:
        h.out_kind, h.n_classes = kind, n_classes
        entry, what = _native.lib().wdmpnn_head_stack_predict, 'FFN head stack (predict)'
    else:
        h.spectra_act, h.normalize, h.mask = spectra, int(bool(normalize)), _native.ptr(mask)
        entry, what = _native.lib().wdmpnn_head_spectra_predict, 'FFN head spectra (predict)'
    _native.check(entry(ctypes.byref(h), _native.current_stream(dev)), what)
    return out.view(B, T // n_classes, n_classes) if kind == 2 and spectra is None else out


NO_LATENT_LAYER = 'With a ffn_num_layers of 1, there is no latent FFN representation. Use MPN fingerprint type instead.'


def head_latent(model: nn.Module, emb: torch.Tensor, head=None) -> torch.Tensor:
    """The input of the FFN's last Linear in eval mode from the encodings ``emb`` (model.py:123-150,
    ``fingerprint_type='last_FFN'``: ``ffn[:-1](emb)``) as ``[B][ffn_hidden_size]`` float32 on the device: L - 1 HIP
    launches (``wdmpnn_head_stack_latent``), the first L - 2 of them those of ``head_predict``.  ``head``: the
    model's ``_predict_head``, as ``head_predict`` takes it.  No autograd graph is built.
    ``NotImplementedError`` for an FFN the native stack does not run; ``ValueError`` for a model in training mode,
    for ``ffn_num_layers == 1`` (molecule_fingerprint.py:83-87) and for a spectra model: its ``ffn[:-1]`` strips
    only the output activation, so the reference's latent array of width ``ffn_hidden_size`` cannot hold it."""
    if model.training:
        raise ValueError('head_latent is an eval-mode head: call model.eval() first')
    if head is None:
        head = _predict_head(model)
    if head is None:
        raise NotImplementedError('head_latent: the model\'s FFN is not one the native head runs (Dropout / Linear / '
                                  'activation stacks of create_ffn, <= 64 outputs, a single PReLU slope)')
    linears, act, slope, _, _, spectra = _head_parts(head)
    if spectra is not None:
        raise ValueError('head_latent: a spectra model has no last_FFN representation (its ffn[:-1] ends with the '
                         'last Linear, of the spectrum\'s width, not ffn_hidden_size). Use MPN fingerprint type instead.')
    if len(linears) < 2:
        raise ValueError(NO_LATENT_LAYER)
    x = _head_input(emb, linears[0])
    dev = x.device
    h = _native.WdHeadLatent()
    B, _, Hf, _, L = _fill_ffn(h, x, linears, slope, act)
    scratch = torch.empty(max((L - 2) * B * Hf, 4), dtype=torch.float32, device=dev)  # (z_1 .. z_{L-2})
    out = torch.empty((B, Hf), dtype=torch.float32, device=dev)
    h.scratch, h.scratch_bytes, h.out, h.ld_out = scratch.data_ptr(), scratch.numel() * 4, out.data_ptr(), Hf
    _native.check(_native.lib().wdmpnn_head_stack_latent(ctypes.byref(h), _native.current_stream(dev)),
                  'FFN head stack (latent)')
    return out


def _grad_buffer(p: torch.Tensor) -> torch.Tensor:
    """The tensor a direct step writes p's gradient into: p.grad when it can be overwritten in place (a
    GradBucket view, or the last step's gradient), else a fresh one (installed as p.grad)."""
    g = p.grad
    if g is None or g.shape != p.shape or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device:
        g = torch.empty_like(p)
        p.grad = g
    return g


def _features_ok(mpn, features_batch) -> bool:
    """The features side of a direct step: a model without input features gets none; a model with them gets
    rows that are on the device already (``features.FeatureRows`` or a float32 ``[B][Ff]`` tensor there).  A list
    of numpy rows keeps the autograd path."""
    if mpn.use_input_features:
        return is_device_features(features_batch)
    return features_batch is None


def _descriptors_ok(mpn, enc, atom_descriptors_batch) -> bool:
    """The descriptor side of a direct step: a model without ``atom_descriptors_layer`` gets none; a model with
    it gets rows of a device table (``atom_descriptors.AtomDescriptorRows``) and has no encoder dropout, so that the
    layer runs after the readout (``MPNEncoder._after_readout``).  A list of numpy arrays and active dropout keep
    the autograd path, and so does an atom-message encoder with descriptors: the layer after the readout joins
    the bond-message encoder's atom states (a model without descriptors takes the direct step in either mode)."""
    has = hasattr(enc, 'atom_descriptors_layer')
    if not mpn.atom_descriptors and not has:
        return atom_descriptors_batch is None
    from .atom_descriptors import is_device_descriptors
    return mpn.atom_descriptors == 'descriptor' and has and not enc.atom_messages and \
        is_device_descriptors(atom_descriptors_batch) and \
        atom_descriptors_batch.device.type == 'cuda' and enc.dropout == 0 and enc._after_readout()


def _direct_encoder(model: nn.Module, mol_batch, features_batch, head, atom_descriptors_batch=None):
    """The MPNEncoder when the step can skip autograd: one molecule per input, atom descriptors only as rows of
    a device table with the layer after the readout (``_descriptors_ok``), extra features
    only as device rows (``_features_ok``), depth >= 2, every parameter trainable and written by the direct
    step (the encoder's native gradients, the descriptor layer's and the fused head's); else None."""
    from .model import MoleculeModel
    from .mpn import MPNEncoder
    if not isinstance(model, MoleculeModel) or type(model).forward is not MoleculeModel.forward:
        return None
    mpn = model.encoder
    if mpn.features_only or not _features_ok(mpn, features_batch) or \
            len(mpn.encoder) != 1 or not isinstance(mol_batch, (list, tuple)) or len(mol_batch) != 1:
        return None
    enc = mpn.encoder[0]
    if type(enc) is not MPNEncoder or enc.depth < 2 or not _descriptors_ok(mpn, enc, atom_descriptors_batch):
        return None
    if type(mol_batch[0]).__name__ != 'BatchMolGraph':
        return None
    ids = []
    if not _all_trainable(model, enc.cached_zero_vector, ids):
        return None
    # the direct step skips zero_grad and overwrites only the gradients it computes: any other trainable
    # parameter (a future addition to the model) would keep a stale gradient, so it must not exist
    linears, _, slope, _, _, _ = _head_parts(head)
    head_params = [t for l in linears for t in (l.weight, l.bias)] + [slope]
    written = {id(t) for _, t in enc._direct_names()} | {id(t) for t in head_params if t is not None}
    if atom_descriptors_batch is not None:  # (the layer after the readout writes its own two gradients)
        written |= {id(t) for t in enc.atom_descriptors_layer._parameters.values() if t is not None}
    # (a shared activation module sits at several places of the FFN's Sequential: its slope is met once per site)
    if set(ids) != written:
        return None
    return enc


def _all_trainable(mod: nn.Module, skip, ids: list) -> bool:
    """Every parameter of ``mod`` and its submodules (but ``skip``) requires grad (their ids appended to
    ``ids``): ``named_parameters``'s test on the raw module dicts (its generators and memo sets cost tens of
    us per step)."""
    for p in mod._parameters.values():
        if p is not None and p is not skip:
            if not p.requires_grad:
                return False
            ids.append(id(p))
    for m in mod._modules.values():
        if m is not None and not _all_trainable(m, skip, ids):
            return False
    return True


def _collect_parameters(mod: nn.Module, skip, out: dict) -> None:
    """id -> parameter of ``mod`` and its submodules (but ``skip``), from the raw module dicts (``_all_trainable``)."""
    for p in mod._parameters.values():
        if p is not None and p is not skip:
            out[id(p)] = p
    for m in mod._modules.values():
        if m is not None:
            _collect_parameters(m, skip, out)


class _FrozenPlan:
    """A partly frozen model the direct step runs (``_frozen_plan``): the encoder, whether all of it is frozen,
    the FFN as a :class:`_StackHead` (kind set) and the frozen parameters (their ``.grad`` is set to None)."""
    __slots__ = ('enc', 'enc_frozen', 'head', 'frozen')

    def __init__(self, enc, enc_frozen, head, frozen):
        self.enc, self.enc_frozen, self.head, self.frozen = enc, enc_frozen, head, frozen

    def grad_of(self, p: torch.Tensor) -> Optional[torch.Tensor]:
        return _grad_buffer(p) if p.requires_grad else None


def _frozen_plan(model: nn.Module, mol_batch, features_batch, head, cached: bool = False) -> Optional[_FrozenPlan]:
    """The plan of a direct step on a model with frozen parameters, else None.  The conditions of
    ``_direct_encoder`` on the model, the encoder and the batch (``cached``: the step runs from cached encodings
    and has no batch), with these in place of "every parameter trainable": every parameter belongs to the
    encoder or to an FFN ``_ffn_structure`` recognises (the two-layer head runs as a stack head here: the one
    entry point that leaves gradients out), the encoder's parameters are all frozen or all trainable, and at
    least one parameter is frozen (any subset of the FFN's weights, biases and slope may be).  ``head`` is
    ``_fusable_head``'s answer: it gives the loss kind.  A partly frozen encoder (``freeze_first_only``) is not
    a plan: such a model keeps the autograd path."""
    from .model import MoleculeModel
    from .mpn import MPNEncoder
    if head is None or not isinstance(model, MoleculeModel) or type(model).forward is not MoleculeModel.forward:
        return None
    mpn = model.encoder
    if mpn.features_only or not _features_ok(mpn, features_batch) or mpn.atom_descriptors or \
            len(mpn.encoder) != 1:
        return None
    if not cached and (not isinstance(mol_batch, (list, tuple)) or len(mol_batch) != 1 or
                       type(mol_batch[0]).__name__ != 'BatchMolGraph'):
        return None
    enc = mpn.encoder[0]
    if type(enc) is not MPNEncoder or enc.depth < 2 or hasattr(enc, 'atom_descriptors_layer'):
        return None
    st = head
    if not isinstance(head, _StackHead):
        st = _ffn_structure(model.ffn, model.training)
        if st is None:
            return None
        _, _, _, kind, n_classes, _ = _head_parts(head)
        st = st.with_kind(kind, n_classes)
    head_params = [t for t in st.params() if t is not None]  # (devices and dtypes: checked by _fusable_head)
    enc_params = [t for _, t in enc._direct_names()]
    known = {id(t) for t in enc_params} | {id(t) for t in head_params}
    every = {}
    _collect_parameters(model, enc.cached_zero_vector, every)
    if set(every) != known:
        return None
    n_train = sum(t.requires_grad for t in enc_params)
    if n_train not in (0, len(enc_params)):
        return None
    frozen = [t for t in every.values() if not t.requires_grad]
    if not frozen:
        return None
    return _FrozenPlan(enc, n_train == 0, st, frozen)


def frozen_encodings(model: nn.Module, graphs: Sequence, batch_size: int) -> torch.Tensor:
    """The encodings ``[len(graphs)][F]`` of a list of ``MolGraph`` under the frozen encoder of ``model``, in
    batches of ``batch_size`` through ``MPNEncoder.forward_many``: with a frozen encoder and no encoder dropout a
    molecule's encoding is the same at every step, so a fine-tuning run computes it once and passes the rows of
    each batch to ``train_step(encodings=...)`` / ``head_predict``.  ``ValueError`` when any encoder parameter
    requires grad or the encoder's dropout would be active in training mode (``dropout > 0``)."""
    from .featurization import BatchMolGraph
    mpn = model.encoder
    if mpn.features_only or len(mpn.encoder) != 1:
        raise ValueError('frozen_encodings: one message-passing encoder expected')
    enc = mpn.encoder[0]
    if any(p.requires_grad for p in enc.parameters()):
        raise ValueError('frozen_encodings: the encoder has trainable parameters (its encodings change every step)')
    if enc.dropout > 0:
        raise ValueError(f'frozen_encodings: encoder dropout {enc.dropout} would be active while training '
                         '(the encodings differ from step to step)')
    dev = enc.W_i.weight.device
    if not len(graphs):
        return torch.empty((0, enc.hidden_size), dtype=torch.float32, device=dev)
    batches = [BatchMolGraph(list(graphs[s:s + batch_size])) for s in range(0, len(graphs), batch_size)]
    outs = []
    with torch.no_grad():
        for s in range(0, len(batches), 8):  # (forward_many launches once per 8 batches; their workspaces are live together)
            outs += enc.forward_many(batches[s:s + 8])
    return torch.cat(outs, dim=0)


def _direct_head(out, head, target_batch, target_weights, data_weights, grad_of: Callable, want_dx: bool = True):
    """The head's part of a direct step on its input ``out`` ``[B][F]``: the loss table, the fused head (loss, dx
    and the head's gradients into ``grad_of``'s buffers).  Returns (loss, dx)."""
    linears, _, _, kind, n_classes, spectra = _head_parts(head)
    spectra = spectra is not None
    nc = n_classes if kind == 2 and not spectra else 0  # (multiclass: _loss_table checks the class indices on the host)
    # the loss table read by the head kernel straight from its pinned host buffer (no copy launch in the
    # step: the copy kernel and its gap were ~10 us, profiles/round4_train_kernel_trace_v1.txt)
    # (the spectra row kernel reads its table rows in several passes: a device copy, not the pinned buffer)
    zc = None
    if not spectra:
        zc, n_t, n_mask, tshape = _loss_table(target_batch, target_weights, data_weights, out.device, zero_copy=True,
                                              num_classes=nc)
    if zc is None:
        table, n_t, n_mask = _loss_table(target_batch, target_weights, data_weights, out.device, num_classes=nc,
                                         spectra=spectra)
        tab_ptr, tshape = table.data_ptr(), tuple(table.shape)
    else:
        tab_ptr = zc[0]
    inv_n = _check_head_batch(linears, n_classes, n_t, n_mask, tshape[0], out)
    dev = out.device
    if isinstance(head, _StackHead):
        loss, dx, _ = _run_head_stack(out, head, tab_ptr, tshape[1], inv_n, _head_seed(head), grad_of, want_dx)
    else:
        loss, dx, _ = _run_head_two(out, head, tab_ptr, tshape[1], inv_n, _grad_buffer)
    if zc is not None:
        zc[1].record(torch.cuda.current_stream(dev))  # (the pinned buffer's last reader)
    return loss, dx


def _direct_step(model, enc, graph, head, target_batch, target_weights, data_weights, bucket=None,
                 plan: _FrozenPlan = None, encodings: torch.Tensor = None, features=None,
                 descriptors=None) -> torch.Tensor:
    """Forward, loss and every gradient of a fused-head step without the autograd engine: the encoder's
    training forward, wdmpnn_head_mse (loss, d loss / d encoding, the head's gradients) and the encoder's
    backward on that gradient (the incoming gradient of the loss is 1), each written straight into the
    parameters' .grad buffers.  The same launches as the autograd path minus its host gaps (the engine
    hand-off, the gradient-seed fill and the scale by 1; profiles/round3_*).
    With ``plan`` (a partly frozen model, ``_frozen_plan``) the head leaves out the frozen parameters' gradients
    (``wdmpnn_head_stack_partial``) and sets their ``.grad`` to None; a frozen encoder runs its inference
    forward on a pack that outlives optimizer steps (``MPNEncoder._frozen_forward``), the head computes no dx and
    there is no encoder backward.  ``encodings`` (frozen encoder only): this batch's rows of
    ``frozen_encodings`` in place of the forward.
    ``features`` (a model with input features: ``features.FeatureRows`` or a float32 device tensor [B][Ff]):
    one ``wdmpnn_join_rows`` launch builds the head's input x = [encoding | features] after the encoder
    forward, the head runs on x (F = ld_x = H + Ff), and one more launch makes the encoder's slice of dx,
    dx[:, 0:H], contiguous for the encoder backward (a frozen encoder has no dx and no such launch): what
    ``torch.cat`` and its backward do on the autograd path, bitwise.
    ``descriptors`` (``atom_descriptors.AtomDescriptorRows``, encoder dropout 0): the encoder runs as for a model
    without descriptors, then ``wdmpnn_desc_join`` and ``wdmpnn_desc_layer`` give the encoding ``[B][H + d]`` the
    rest of the step sees; after the head, one ``wdmpnn_desc_layer_backward`` launch writes the layer's two
    gradients and the encoder backward's input."""
    enc_frozen = plan is not None and plan.enc_frozen
    if encodings is not None:
        out = encodings
    elif enc_frozen:
        out = enc._frozen_forward(graph)
    else:
        out, state = enc._train_forward(graph)
    desc_x = None
    if descriptors is not None:
        from . import atom_descriptors as ad
        descriptors.bind(graph)
        lin, sid = enc.atom_descriptors_layer, _native.current_stream(out.device)
        desc_x = ad.desc_join(descriptors, state[0], out, _native.AGGREGATIONS[enc.aggregation],
                              float(enc.aggregation_norm), sid)
        out = ad.desc_layer(desc_x, lin.weight, lin.bias, sid)
    n_emb = out.shape[1] if out.dim() == 2 else 0
    if features is not None:
        out = join_features(out, features)  # (x: the head's input from here on)
    loss, dx = _direct_head(out, head, target_batch, target_weights, data_weights,
                            _grad_buffer if plan is None else plan.grad_of, not enc_frozen)
    dev = out.device
    if bucket is not None:  # the head's gradients are enqueued: their all-reduce overlaps the encoder backward
        bucket.start_early()
    if plan is not None:
        for p in plan.frozen:  # (as zero_grad(set_to_none=True) on the autograd path: the optimizer skips them)
            p.grad = None
    if not enc_frozen:
        if features is not None:
            dx = split_columns(dx, 0, n_emb)  # (the encoder's slice of dx, contiguous: torch.cat's backward)
        if desc_x is not None:
            lin, dy = enc.atom_descriptors_layer, dx
            dx = torch.empty((dy.shape[0], enc.hidden_size), dtype=torch.float32, device=dev)
            ad.desc_layer_backward(dy, desc_x, lin.weight, enc.hidden_size, _grad_buffer(lin.weight),
                                   None if lin.bias is None else _grad_buffer(lin.bias), dx,
                                   _native.current_stream(dev))
        enc._train_backward(state, dx, {n: _grad_buffer(p) for n, p in enc._direct_names()})
    return loss


class _SlotPlan:
    """A model of several molecules per input the direct step runs (``_direct_slots``): its distinct encoders (one
    for ``mpn_shared``), the number of slots and whether one encoder serves all of them."""
    __slots__ = ('encoders', 'n', 'shared')

    def __init__(self, encoders, n, shared):
        self.encoders, self.n, self.shared = encoders, n, shared


def _all_trainable_but(mod: nn.Module, skip: set, ids: list) -> bool:
    """``_all_trainable`` with several parameters left out (``skip``: their ids)."""
    for p in mod._parameters.values():
        if p is not None and id(p) not in skip:
            if not p.requires_grad:
                return False
            ids.append(id(p))
    for m in mod._modules.values():
        if m is not None and not _all_trainable_but(m, skip, ids):
            return False
    return True


def _direct_slots(model: nn.Module, mol_batch, features_batch, head, atom_descriptors_batch=None):
    """``_direct_encoder`` for ``number_of_molecules > 1``: the :class:`_SlotPlan` when the step can skip autograd,
    else None.  The same conditions on every encoder (plain ``MPNEncoder``, depth >= 2, no atom messages, features
    only as device rows, every parameter trainable and written by the step), no atom descriptors, one
    ``BatchMolGraph`` per slot.  A shared encoder (``mpn_shared``) also needs the batch's merged graph
    (``slots.SlotBatch(shared=True)``) and no encoder dropout: the one forward over the merged batch would draw
    one seed where the per-slot path draws N."""
    from .model import MoleculeModel
    from .mpn import MPNEncoder
    from .slots import merged_graph
    if not isinstance(model, MoleculeModel) or type(model).forward is not MoleculeModel.forward:
        return None
    mpn = model.encoder
    if mpn.features_only or len(mpn.encoder) < 2 or len(mpn.encoder) > _native.MAX_SLOTS or \
            not _features_ok(mpn, features_batch) or mpn.atom_descriptors or atom_descriptors_batch is not None or \
            not isinstance(mol_batch, (list, tuple)) or len(mol_batch) != len(mpn.encoder):
        return None
    encoders = []
    for enc, g in zip(mpn.encoder, mol_batch):
        if type(enc) is not MPNEncoder or enc.depth < 2 or enc.atom_messages or \
                hasattr(enc, 'atom_descriptors_layer') or type(g).__name__ != 'BatchMolGraph' or \
                enc.hidden_size != mpn.encoder[0].hidden_size:
            return None
        if all(enc is not e for e in encoders):
            encoders.append(enc)
    n = len(mpn.encoder)
    shared = len(encoders) == 1
    if not shared and len(encoders) != n:
        return None
    if shared and (encoders[0].dropout > 0 or merged_graph(mol_batch) is None):
        return None
    ids = []
    if not _all_trainable_but(model, {id(e.cached_zero_vector) for e in encoders}, ids):
        return None
    linears, _, slope, _, _, _ = _head_parts(head)
    head_params = [t for l in linears for t in (l.weight, l.bias)] + [slope]
    written = {id(t) for e in encoders for _, t in e._direct_names()} | {id(t) for t in head_params if t is not None}
    if set(ids) != written:
        return None
    return _SlotPlan(encoders, n, shared)


def _direct_step_slots(plan: _SlotPlan, mol_batch, head, target_batch, target_weights, data_weights,
                       features=None) -> torch.Tensor:
    """``_direct_step`` for a model of N molecules per input.  Not shared: every encoder's training forward in slot
    order (their dropout seeds are drawn in that order, as on the autograd path), one ``wdmpnn_slots_join`` launch
    that builds x = [enc_0 | .. | enc_{N-1} | features], the fused head on x, one ``wdmpnn_slots_split`` launch
    that makes every slot's slice of dx contiguous, every encoder's backward into its own ``.grad`` buffers: two
    launches more than the one-molecule pieces, and the losses and gradients of the autograd path, bitwise (the join
    and the split move what ``torch.cat`` and its backward move).  Shared: one training forward over the merged
    batch, whose output ``[N B][H]`` is the join's slot-major input; the split writes one ``[N B][H]`` buffer, the
    merged backward's ``dout``, and the one backward's split-K GEMMs sum the shared weights' gradients over the
    slots themselves."""
    from .slots import join_slots, split_slots
    n_rows = len(mol_batch[0].a_scope)
    if plan.shared:
        enc = plan.encoders[0]
        out, state = enc._train_forward(mol_batch.merged)
        if out.shape[0] != plan.n * n_rows:
            raise ValueError(f'the merged batch holds {out.shape[0]} molecules for {plan.n} slots of {n_rows} rows')
        embs, states = [out], [state]
    else:
        embs, states = [], []
        for enc, g in zip(plan.encoders, mol_batch):
            out, state = enc._train_forward(g)
            embs.append(out)
            states.append(state)
    H = embs[0].shape[1]
    x = join_slots(embs, n_rows, features)
    loss, dx = _direct_head(x, head, target_batch, target_weights, data_weights, _grad_buffer)
    d = split_slots(dx, plan.n, H)
    if plan.shared:
        enc = plan.encoders[0]
        enc._train_backward(states[0], d.view(plan.n * n_rows, H), {n: _grad_buffer(p) for n, p in enc._direct_names()})
    else:
        for k, enc in enumerate(plan.encoders):
            enc._train_backward(states[k], d[k], {n: _grad_buffer(p) for n, p in enc._direct_names()})
    return loss


def train_step(model: nn.Module, mol_batch, target_batch, loss_func: Callable, optimizer: Optimizer,
               scheduler: _LRScheduler = None, dataset_type: str = 'regression', features_batch=None,
               target_weights=None, data_weights=None, grad_clip: float = None,
               bucket: GradBucket = None, fused_head: bool = True, direct: bool = True,
               encodings: torch.Tensor = None, atom_descriptors_batch=None) -> torch.Tensor:
    """One optimisation step (train.py:55-86).  With ``bucket`` the gradients are averaged over the
    data-parallel ranks (one all-reduce) before clipping and the optimizer step.  ``fused_head``: the
    default regression / classification / multiclass head + loss run as ``wdmpnn_head_mse`` (same loss and gradients within fp32
    summation order; ``False`` = the torch ops of the reference); FFNs with another number of layers, active
    dropout or PReLU run as ``wdmpnn_head_stack`` (their dropout masks follow ``nn_utils.dropout_mask``, not
    torch's generator); a spectra model (``dataset_type='spectra'`` with ``spectra_utils.sid_loss`` or
    ``wasserstein_loss``, up to 8192 outputs) always runs ``wdmpnn_head_spectra``, on every path below.
    Its ``target_batch`` may be a float ``ndarray`` [B][T] with NaN = missing instead of lists with ``None``.
    ``direct``: with the fused head and a
    plain one-molecule encoder, skip the autograd engine (``_direct_step``: the same launches and results,
    bitwise, without the engine's host gaps).  The direct step keeps one packed copy of the encoder weights
    across steps (rewritten by :class:`HipAdam`); after writing an encoder parameter through ``.data`` call
    ``MPNEncoder.invalidate_packed_params()`` (reassigned parameters and ``load_state_dict`` are detected).

    Partly frozen models (fine-tuning: ``requires_grad = False`` on all of the encoder and / or on any of the
    FFN's weights, biases and slope; ``_frozen_plan``) take the direct step too: the head computes only the
    wanted gradients (``wdmpnn_head_stack_partial``, on the autograd path as well), a frozen encoder runs its
    inference forward on a weight pack kept across optimizer steps with no backward, and the frozen
    parameters' ``.grad`` is None after the step.  ``encodings``: this batch's rows of ``frozen_encodings``
    (frozen encoder without dropout): the step is then the head and the optimizer alone, with the same result,
    bitwise; ``mol_batch`` is not read.

    ``features_batch`` (a model with ``use_input_features``): a list of numpy rows as in the reference takes the
    autograd path (``MPN.forward`` stacks, copies and concatenates them); ``features.FeatureRows`` (rows of a
    device-resident ``FeatureTable``) or a float32 device tensor ``[B][Ff]`` take the direct step, frozen plans and
    ``encodings=`` included: two more launches than the same step without features (the join and the split of
    dx), one with a frozen encoder or cached encodings, and the same losses and gradients, bitwise.

    ``atom_descriptors_batch`` (a model with ``atom_descriptors='descriptor'``): ``AtomDescriptorRows`` of a
    device-resident ``atom_descriptors.AtomDescriptorTable`` take the direct step when the encoder has no dropout
    (the descriptor layer runs after the readout: encoder forward, join, layer, features join if any, head,
    layer backward, encoder backward).  A list of numpy arrays as in the reference, active dropout, atom
    messages together with descriptors, depth 1 and partly frozen models take the autograd path.

    A model of several molecules per input (``number_of_molecules > 1``; ``mol_batch`` is the list of one
    ``BatchMolGraph`` per molecule, or a ``slots.SlotBatch``) takes the direct step as well (``_direct_slots``,
    ``_direct_step_slots``): every encoder's forward, one ``wdmpnn_slots_join`` launch, the fused head, one
    ``wdmpnn_slots_split`` launch, every encoder's backward; bitwise the autograd path's losses and gradients, and
    :class:`HipAdam` rewrites every encoder's pack.  A shared encoder (``mpn_shared``) runs once, forward and
    backward, over ``SlotBatch(shared=True).merged`` when it has no dropout (the project's parity bound instead of
    bitwise: the merged batch is cut into other molecule blocks); given a plain list, or with dropout, it keeps the
    autograd path.  So do frozen plans, ``encodings=``, ``bucket`` steps and atom descriptors with several molecules."""
    if encodings is not None and atom_descriptors_batch is not None:
        raise ValueError('train_step(encodings=...) takes no atom descriptors (frozen plans with descriptors keep the '
                         'autograd path)')
    if not model.training:  # (module.train() walks every submodule: the reference sets it once per epoch)
        model.train()
    head = _fusable_head(model, loss_func, dataset_type) if fused_head else None
    enc = _direct_encoder(model, mol_batch, features_batch, head, atom_descriptors_batch) \
        if head is not None and direct and encodings is None else None
    slots = None
    if enc is None and head is not None and direct and encodings is None and bucket is None and \
            len(getattr(model.encoder, 'encoder', ())) > 1:
        slots = _direct_slots(model, mol_batch, features_batch, head, atom_descriptors_batch)
    plan = None
    if enc is None and slots is None and head is not None and bucket is None:
        plan = _frozen_plan(model, mol_batch, features_batch, head, cached=encodings is not None)
        if plan is not None:
            head = plan.head  # (the stack head on either path: the same head arithmetic with and without autograd)
    if encodings is not None:
        if plan is None or not plan.enc_frozen or plan.enc.dropout > 0 or not direct:
            raise ValueError('train_step(encodings=...) needs the direct step of a model with a frozen encoder without '
                             'dropout and an FFN the native head runs')
        l1 = plan.head.linears[0]
        n_feat = features_width(features_batch) if features_batch is not None else 0
        if encodings.dim() != 2 or encodings.shape[1] + n_feat != l1.in_features or \
                encodings.dtype != torch.float32 or encodings.device != l1.weight.device:
            raise ValueError(f'encodings of shape {tuple(encodings.shape)} ({encodings.dtype}, {encodings.device}) '
                             f'and {n_feat} features for an FFN input of {l1.in_features} on {l1.weight.device}')
        encodings = encodings.detach().contiguous()
    if plan is not None and not direct:
        plan = None
    if plan is not None:
        enc = plan.enc if not plan.enc_frozen else None  # (HipAdam rewrites a trainable encoder's pack)
        loss = _direct_step(model, plan.enc, None if encodings is not None else mol_batch[0], head, target_batch,
                            target_weights, data_weights, None, plan, encodings, features_batch)
    elif slots is not None:
        loss = _direct_step_slots(slots, mol_batch, head, target_batch, target_weights, data_weights, features_batch)
    elif enc is not None:
        # every trainable parameter's gradient is overwritten: no zeroing, no autograd
        if bucket is not None:
            bucket.attach()
        loss = _direct_step(model, enc, mol_batch[0], head, target_batch, target_weights, data_weights, bucket,
                            features=features_batch, descriptors=atom_descriptors_batch)
    else:
        if bucket is not None:
            bucket.zero()
        else:
            optimizer.zero_grad(set_to_none=True)  # (the optimizer holds every model parameter: build_optimizer)
        # (any model with a (batch, features) forward trains here: descriptors are passed on only when given)
        desc = () if atom_descriptors_batch is None else (atom_descriptors_batch,)
        if head is not None:  # the default regression head: ffn + loss + their gradients as two HIP launches
            loss = head_loss(model.encoder(mol_batch, features_batch, *desc), head, target_batch,
                             target_weights, data_weights)
        else:
            preds = model(mol_batch, features_batch, *desc)
            loss = batch_loss(preds, target_batch, loss_func, dataset_type, target_weights, data_weights)
        loss.backward()
    if bucket is not None:
        # the rest of the bucket behind the last gradient kernel (the direct step launched the head's
        # segment before the encoder backward, so that one overlaps the backward on the GPU); with RCCL
        # finish_allreduce makes the compute stream, not the host, wait for both before the update
        bucket.start_allreduce()
        bucket.finish_allreduce()
    if grad_clip:
        nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
    if isinstance(optimizer, HipAdam):
        if enc is not None:
            optimizer.repack_next(enc)
        elif slots is not None:
            optimizer.repack_next(*slots.encoders)
    optimizer.step()
    if scheduler is not None and isinstance(scheduler, (NoamLR, torch.optim.lr_scheduler.CosineAnnealingLR,
                                                        torch.optim.lr_scheduler.CyclicLR)):
        scheduler.step()
    return loss.detach()


def train(model: nn.Module, batches, loss_func: Callable, optimizer: Optimizer, scheduler: _LRScheduler = None,
          dataset_type: str = 'regression', grad_clip: float = None, bucket: GradBucket = None) -> List[float]:
    """One epoch over ``batches`` = iterable of (mol_batch, target_batch[, features_batch]) (train.py:17-113
    without logging); returns the per-batch losses (one host sync per batch, like loss.item())."""
    losses = []
    for item in batches:
        mol_batch, target_batch = item[0], item[1]
        features_batch = item[2] if len(item) > 2 else None
        loss = train_step(model, mol_batch, target_batch, loss_func, optimizer, scheduler, dataset_type,
                          features_batch, grad_clip=grad_clip, bucket=bucket)
        losses.append(float(loss))
    return losses
