"""Generate tests/golden/multiclass/model_polymer_multiclass.npz from the REAL reference model.

Run where the reference tree is available (tools/ref_loader.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_multiclass_golden.py

The file lives in a subdirectory on purpose: ``golden_io.golden_names()`` feeds every ``tests/golden/*.npz``
to tests that go through ``oracle/mpn_ref.model_forward``, which has no multiclass branch.
``golden_io.load('multiclass/model_polymer_multiclass')`` reads it (the standard keys of
tools/make_goldens.py: graphs, config, ``output`` = the eval-mode class probabilities [7][3][5], ``R`` and
``grad/*`` of sum(output * R)).  Additional keys, the reference's training loss for the same model:

* ``targets`` [7][3] float64, NaN = missing (about a quarter), else the class index;
* ``target_weights`` [3], ``data_weights`` [7];
* ``train_loss``: the model in train mode, then train.py:67-74 with ``nn.CrossEntropyLoss(reduction='none')``
  (utils.py get_loss_func): per-task losses * target weights * data weights * mask, summed, / mask.sum();
* ``train_grad/<name>``: its gradient for every parameter.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'polymer-chemprop_amd'))

from make_goldens import BASE_ARGS, make_graphs, pack_mols  # noqa: E402
from ref_loader import load_reference  # noqa: E402
from chemprop_amd import synthetic  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'multiclass')
NAME = 'model_polymer_multiclass'
KIND, B, SEED = 'polymer', 7, 41
OVERRIDES = dict(hidden_size=64, ffn_hidden_size=48, dataset_type='multiclass', num_tasks=3, multiclass_num_classes=5)


def main():
    ref = load_reference()
    os.makedirs(OUT, exist_ok=True)
    args = types.SimpleNamespace(**{**BASE_ARGS, **OVERRIDES})
    torch.manual_seed(0)
    mol_lists = make_graphs(KIND, B, SEED)
    batches = [ref.featurization.BatchMolGraph(gs) for gs in mol_lists]
    out = {'config': np.array(json.dumps({k: v for k, v in vars(args).items() if k != 'device'})),
           'level': np.array('model'), 'param_seed': np.array(SEED), 'n_slots': np.array(len(batches))}
    for s, (gs, bmg) in enumerate(zip(mol_lists, batches)):
        pack_mols(f's{s}_mol_', gs, out)
        out[f's{s}_a2b'] = bmg.a2b.numpy()
        out[f's{s}_b2a'] = bmg.b2a.numpy()
        out[f's{s}_b2revb'] = bmg.b2revb.numpy()
        out[f's{s}_a_scope'] = np.array(bmg.a_scope, np.int64).reshape(-1, 2)
        out[f's{s}_b_scope'] = np.array(bmg.b_scope, np.int64).reshape(-1, 2)
        out[f's{s}_max_num_bonds'] = np.array(bmg.max_num_bonds)
    module = ref.model.MoleculeModel(args)
    synthetic.fill_parameters(module, SEED)

    # eval: the class probabilities and the gradients of sum(output * R)
    module.eval()
    y = module(batches, None)
    assert tuple(y.shape) == (B, args.num_tasks, args.multiclass_num_classes)
    out['output'] = y.detach().numpy()
    r = np.random.default_rng(SEED + 99).standard_normal(tuple(y.shape)).astype(np.float32)
    out['R'] = r
    (y * torch.from_numpy(r)).sum().backward()
    for pname, p in module.named_parameters():
        if p.grad is not None:
            out[f'grad/{pname}'] = p.grad.numpy().copy()
    out['param_names'] = np.array(json.dumps([n for n, _ in module.named_parameters()]))

    # train: train.py:46-74 with CrossEntropyLoss(reduction='none')
    rng = np.random.default_rng(SEED + 7)
    target_batch = [[None if rng.random() < 0.25 else int(rng.integers(args.multiclass_num_classes))
                     for _ in range(args.num_tasks)] for _ in range(B)]
    tw = rng.uniform(0.5, 1.5, args.num_tasks)
    dw = rng.uniform(0.5, 1.5, B)
    out['targets'] = np.array([[np.nan if x is None else float(x) for x in tb] for tb in target_batch], np.float64)
    out['target_weights'] = tw
    out['data_weights'] = dw
    module.zero_grad()
    module.train()
    loss_func = torch.nn.CrossEntropyLoss(reduction='none')
    present = np.array([[x is not None for x in tb] for tb in target_batch])
    mask = torch.from_numpy(present)
    classes = torch.from_numpy(np.where(present, np.nan_to_num(out['targets']), 0).astype(np.int64))
    preds = module(batches, None)  # train mode: the logits [B][tasks][classes]
    logits_max = float(preds.detach().abs().max())
    per_task = torch.stack([loss_func(preds[:, j, :], classes[:, j]) for j in range(args.num_tasks)], dim=1)
    # the reference's order of the three factors, each rounded to fp32 as there
    loss = (per_task * torch.Tensor(tw) * torch.Tensor(dw).unsqueeze(1) * mask).sum() / mask.sum()
    loss.backward()
    out['train_loss'] = np.array(loss.item(), np.float64)
    for pname, p in module.named_parameters():
        if p.grad is not None:
            out[f'train_grad/{pname}'] = p.grad.numpy().copy()
    path = os.path.join(OUT, f'{NAME}.npz')
    np.savez_compressed(path, **out)
    rows = y.detach().sum(dim=2)
    print(f'{NAME}: out {tuple(y.shape)} rows sum to 1 +- {float((rows - 1).abs().max()):.2g} '
          f'max|logit|={logits_max:.3g} train_loss={loss.item():.6g} missing={int((~mask).sum())}/{mask.numel()} '
          f'{os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
