"""Generate tests/golden/spectra/model_polymer_spectra.npz from the REAL reference model and spectra_utils.

Run where the reference tree is available (tools/ref_loader.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_spectra_golden.py

The file lives in a subdirectory for the reason tools/make_multiclass_golden.py gives.
``golden_io.load('spectra/model_polymer_spectra')`` reads the standard keys (graphs, config, ``output`` = the
eval-mode model output exp(ffn) [8][65]).  The reference's ``MoleculeModel`` with ``dataset_type='spectra'``,
``ffn_num_layers=2``, hidden 48, 65 outputs, no dropout, on an 8-molecule synthetic polymer batch.  Additional keys:

* ``phase_features`` [8][2] one-hot, ``phase_mask`` [2][65] (phase 1 excludes the last 15 positions);
* ``targets`` [8][65] float64, NaN = missing: raw positive spectra with about a fifth of the entries missing,
  through the reference's ``normalize_spectra(..., threshold=1e-8)`` under the phase mask (run_training.py:146-157);
* ``target_weights`` [65], ``data_weights`` [8];
* per loss L in (``sid``, ``wasserstein``), from the model in train mode and train.py:70-74 with the reference's
  ``sid_loss`` / ``wasserstein_loss``: ``L/train_loss``, ``L/lossrow`` [8] (the weighted loss terms summed per row,
  before the division by mask.sum()), ``L/train_grad/<name>`` for every parameter;
* ``normalized`` [8][65]: ``normalize_spectra(output, phase_features, phase_mask, excluded_sub_value=nan)``
  (make_predictions.py:175-181);
* ``sid_metric``, ``wasserstein_metric``: the reference's metrics of ``output`` against ``targets`` with
  ``batch_size`` = the row count (so that its last-batch mean is the mean over all rows).

Prints the normwise distance between the reference's fp32 losses and FFN gradients and an fp64 re-evaluation of
the same formulas from the fp32 encodings: the bar a correct fp32 implementation can meet must be well above it.
"""
from __future__ import annotations

import importlib.util
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
from ref_loader import REF, load_reference  # noqa: E402
from chemprop_amd import synthetic  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'spectra')
NAME = 'model_polymer_spectra'
KIND, B, SEED, T = 'polymer', 8, 43, 65
OVERRIDES = dict(hidden_size=48, ffn_hidden_size=48, dataset_type='spectra', num_tasks=T, spectra_activation='exp')
FLOOR = 1e-8


def load_spectra_utils():
    spec = importlib.util.spec_from_file_location('chemprop.spectra_utils', os.path.join(REF, 'chemprop/spectra_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['chemprop.spectra_utils'] = mod
    spec.loader.exec_module(mod)
    return mod


def normwise(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def main():
    ref = load_reference()
    su = load_spectra_utils()
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
    out['param_names'] = np.array(json.dumps([n for n, _ in module.named_parameters()]))

    # the data: phases, raw spectra with missing entries, normalised as run_training.py:146-157
    rng = np.random.default_rng(SEED + 7)
    phase = rng.integers(0, 2, B)
    phase[0], phase[1] = 0, 1
    phase_features = np.eye(2)[phase]
    phase_mask = np.ones((2, T), np.int64)
    phase_mask[1, T - 15:] = 0
    raw = [[None if rng.random() < 0.2 else float(rng.gamma(2.0)) for _ in range(T)] for _ in range(B)]
    raw[2] = [v if t in (3, 17, 40) else None for t, v in enumerate(raw[2])]  # a row with few present targets
    raw[2][17] = raw[2][17] or 1.0
    targets = su.normalize_spectra(spectra=raw, phase_features=phase_features.tolist(), phase_mask=phase_mask.tolist(),
                                   excluded_sub_value=None, threshold=FLOOR)
    tw = rng.uniform(0.5, 1.5, T)
    dw = rng.uniform(0.5, 1.5, B)
    out['phase_features'] = phase_features
    out['phase_mask'] = phase_mask
    out['targets'] = np.array([[np.nan if x is None else float(x) for x in r] for r in targets], np.float64)
    out['target_weights'] = tw
    out['data_weights'] = dw

    # eval: the model's output, its normalisation and the metrics
    module.eval()
    with torch.no_grad():
        y = module(batches, None)
    assert tuple(y.shape) == (B, T)
    out['output'] = y.numpy()
    preds = y.numpy().tolist()
    norm = su.normalize_spectra(spectra=preds, phase_features=phase_features.tolist(), phase_mask=phase_mask.tolist(),
                                excluded_sub_value=float('nan'))
    out['normalized'] = np.array(norm, np.float64)
    out['sid_metric'] = np.array(su.sid_metric(preds, targets, batch_size=B), np.float64)
    out['wasserstein_metric'] = np.array(su.wasserstein_metric(preds, targets, batch_size=B), np.float64)

    # train: train.py:46-74 with the spectra losses
    present = np.array([[x is not None for x in r] for r in targets])
    mask = torch.from_numpy(present)
    tgt = torch.Tensor([[0 if x is None else x for x in r] for r in targets])
    module.train()
    worst = 0.0
    for name, loss_func in (('sid', su.sid_loss), ('wasserstein', su.wasserstein_loss)):
        module.zero_grad()
        emb = module.encoder(batches, None)
        z = module.ffn(emb)
        per = loss_func(z, tgt, mask) * torch.Tensor(tw) * torch.Tensor(dw).unsqueeze(1) * mask
        loss = per.sum() / mask.sum()
        loss.backward()
        out[f'{name}/train_loss'] = np.array(loss.item(), np.float64)
        out[f'{name}/lossrow'] = per.detach().sum(dim=1).numpy()
        for pname, p in module.named_parameters():
            if p.grad is not None:
                out[f'{name}/train_grad/{pname}'] = p.grad.numpy().copy()
        # the same formulas in fp64 from the fp32 encodings
        ps = {n: p.detach().double().requires_grad_(True) for n, p in module.ffn.named_parameters()}
        h = torch.relu(emb.detach().double() @ ps['1.weight'].t() + ps['1.bias'])
        z64 = torch.exp(h @ ps['4.weight'].t() + ps['4.bias'])
        per64 = loss_func(z64, tgt.double(), mask) * torch.from_numpy(tw) * torch.from_numpy(dw).unsqueeze(1) * mask
        loss64 = per64.sum() / mask.sum()
        loss64.backward()
        d = {'loss': normwise(loss.item(), loss64.item())}
        for n, p in ps.items():
            d[n] = normwise(out[f'{name}/train_grad/ffn.{n}'], p.grad.numpy())
        worst = max(worst, *d.values())
        print(f'{name}: train_loss={loss.item():.6g} fp32 vs fp64: ' + ' '.join(f'{k}={v:.2e}' for k, v in d.items()))
    logits = float(torch.log(y).abs().max())
    path = os.path.join(OUT, f'{NAME}.npz')
    np.savez_compressed(path, **out)
    print(f'{NAME}: out {tuple(y.shape)} max|logit|={logits:.3g} missing={int((~mask).sum())}/{mask.numel()} '
          f'sid_metric={float(out["sid_metric"]):.6g} wasserstein_metric={float(out["wasserstein_metric"]):.6g} '
          f'worst fp32-vs-fp64 normwise distance {worst:.2e} (must be < 1e-5) {os.path.getsize(path) / 1024:.0f} KiB')
    assert worst < 1e-5, 'the fp32 reference is further than 1e-5 from fp64: choose milder logits'


if __name__ == '__main__':
    main()
