"""Generate tests/golden/multi_molecule/*.npz from the REAL reference model with number_of_molecules > 1.

Run where the reference tree is available (tools/ref_loader.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_multi_molecule_golden.py

Two cases, parameters from ``synthetic.synthetic_parameter`` (regenerated from the seed by the tests), dropout 0:

* ``shared_two_regression``: ``mpn_shared=True``, 2 molecules per input (polymer + qm9), B = 5, hidden 32, one
  regression task, no input features.  The reference builds ``[MPNEncoder] * 2``: one set of encoder weights, whose
  gradient is the sum over both slots.
* ``three_mols_features_cls``: three encoders (polymer + qm9 + zinc), B = 3, hidden 30, 4 input features, two
  classification tasks with one missing target.

The files live in a subdirectory for the reason tools/make_multiclass_golden.py gives: ``golden_io.golden_names()``
feeds every ``tests/golden/*.npz`` to tests of their own.  ``golden_io.load('multi_molecule/<name>')`` reads them
(the standard keys of tools/make_goldens.py: per-slot graphs, config, ``output`` = the eval-mode predictions, ``R``
and ``grad/*`` of sum(output * R)).  Additional keys, the reference's training loss:

* ``targets`` [B][T] float64, NaN = missing; ``target_weights`` [T], ``data_weights`` [B];
* ``train_loss``: the model in train mode, then train.py:46-74 with ``MSELoss`` / ``BCEWithLogitsLoss``
  (``reduction='none'``): losses * target weights * data weights * mask, summed, / mask.sum();
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

from make_goldens import BASE_ARGS, pack_mols  # noqa: E402
from ref_loader import load_reference  # noqa: E402
from chemprop_amd import synthetic  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'multi_molecule')

# name -> (slot kinds, B, seed, arg overrides, index of the missing target or None)
CASES = {
    'shared_two_regression': (('polymer', 'qm9'), 5, 61,
                              dict(hidden_size=32, ffn_hidden_size=32, number_of_molecules=2, mpn_shared=True,
                                   dataset_type='regression', num_tasks=1), None),
    'three_mols_features_cls': (('polymer', 'qm9', 'zinc'), 3, 62,
                                dict(hidden_size=30, ffn_hidden_size=30, number_of_molecules=3, mpn_shared=False,
                                     use_input_features=True, features_size=4, dataset_type='classification',
                                     num_tasks=2), (1, 0)),
}


def main():
    ref = load_reference()
    os.makedirs(OUT, exist_ok=True)
    for name, (kinds, B, seed, overrides, missing) in CASES.items():
        args = types.SimpleNamespace(**{**BASE_ARGS, **overrides})
        torch.manual_seed(0)
        mol_lists = [synthetic.make_batch(kind, B, seed + 1000 * s) for s, kind in enumerate(kinds)]
        batches = [ref.featurization.BatchMolGraph(gs) for gs in mol_lists]
        out = {'config': np.array(json.dumps({k: v for k, v in vars(args).items() if k != 'device'})),
               'level': np.array('model'), 'param_seed': np.array(seed), 'n_slots': np.array(len(batches))}
        features = None
        if args.use_input_features:
            frng = np.random.default_rng(seed + 7)
            features = [frng.standard_normal(args.features_size).astype(np.float32) for _ in range(B)]
            out['features'] = np.stack(features)
        for s, (gs, bmg) in enumerate(zip(mol_lists, batches)):
            pack_mols(f's{s}_mol_', gs, out)
            out[f's{s}_a2b'] = bmg.a2b.numpy()
            out[f's{s}_b2a'] = bmg.b2a.numpy()
            out[f's{s}_b2revb'] = bmg.b2revb.numpy()
            out[f's{s}_a_scope'] = np.array(bmg.a_scope, np.int64).reshape(-1, 2)
            out[f's{s}_b_scope'] = np.array(bmg.b_scope, np.int64).reshape(-1, 2)
            out[f's{s}_max_num_bonds'] = np.array(bmg.max_num_bonds)
        module = ref.model.MoleculeModel(args)
        synthetic.fill_parameters(module, seed)
        if args.mpn_shared:
            assert module.encoder.encoder[0] is module.encoder.encoder[1]

        # eval: the predictions and the gradients of sum(output * R)
        module.eval()
        y = module(batches, features)
        assert tuple(y.shape) == (B, args.num_tasks)
        out['output'] = y.detach().numpy()
        r = np.random.default_rng(seed + 99).standard_normal(tuple(y.shape)).astype(np.float32)
        out['R'] = r
        (y * torch.from_numpy(r)).sum().backward()
        for pname, p in module.named_parameters():
            if p.grad is not None:
                out[f'grad/{pname}'] = p.grad.numpy().copy()
        out['param_names'] = np.array(json.dumps([n for n, _ in module.named_parameters()]))

        # train: train.py:46-74
        rng = np.random.default_rng(seed + 7)
        cls = args.dataset_type == 'classification'
        target_batch = [[float(rng.integers(0, 2)) if cls else float(rng.normal()) for _ in range(args.num_tasks)]
                        for _ in range(B)]
        if missing is not None:
            target_batch[missing[0]][missing[1]] = None
        tw = rng.uniform(0.5, 1.5, args.num_tasks)
        dw = rng.uniform(0.5, 1.5, B)
        out['targets'] = np.array([[np.nan if x is None else x for x in tb] for tb in target_batch], np.float64)
        out['target_weights'] = tw
        out['data_weights'] = dw
        module.zero_grad()
        module.train()
        loss_func = torch.nn.BCEWithLogitsLoss(reduction='none') if cls else torch.nn.MSELoss(reduction='none')
        mask = torch.Tensor([[x is not None for x in tb] for tb in target_batch])
        targets = torch.Tensor([[0 if x is None else x for x in tb] for tb in target_batch])
        preds = module(batches, features)
        # the reference's order of the three factors, each rounded to fp32 as there
        loss = (loss_func(preds, targets) * torch.Tensor(tw) * torch.Tensor(dw).unsqueeze(1) * mask).sum() / mask.sum()
        loss.backward()
        out['train_loss'] = np.array(loss.item(), np.float64)
        for pname, p in module.named_parameters():
            if p.grad is not None:
                out[f'train_grad/{pname}'] = p.grad.numpy().copy()
        path = os.path.join(OUT, f'{name}.npz')
        np.savez_compressed(path, **out)
        print(f'{name}: out {tuple(y.shape)} train_loss={loss.item():.6g} '
              f'missing={int((1 - mask).sum())}/{mask.numel()} {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
