"""Time the training step of a model with molecule-level input features.

    python tools/features_step.py [--model regression|spectra] [--variants list direct cached] [--steps 200] [--out FILE]

Polymer batches of 64, hidden 300, depth 3, a two-layer FFN.  ``--model regression``: one task, 200 features per
molecule (a descriptor file); ``--model spectra``: T = 1801 outputs, SID loss, 2 one-hot phase features.  Variants
(each with its own model and optimizer, same seed, alternated REPEATS times in ONE process; per repeat 20 warm-up
steps, then the timed steps ending in a synchronise):

* ``list``: ``features_batch`` is a list of numpy rows -- ``MPN.forward`` stacks them, copies them to the device
  and concatenates, under autograd.  On a tree without ``chemprop_amd.features`` this is the only step such a
  model has (the parent commit's: run this file there for its figure);
* ``direct``: the rows of a resident ``FeatureTable`` (one index upload per repeat, a slice per step): the direct
  step, where the tree has one for such models;
* ``frozen``: the same with a frozen encoder; ``cached``: the frozen encoder's encodings computed once
  (``train.frozen_encodings``), every step the join, the head and the optimizer alone.

``--no_features`` builds the same model without input features (the launch-count baseline of a traced run).
Reports each repeat, the medians and the spread (max - min) between the repeats of one variant; two medians
differ only when they are further apart than the larger spread.  With ``--variants V --steps 5`` under
``rocprofv3 --kernel-trace --stats`` (a run of its own) it gives the kernel list of the step:
calls / (REPEATS x 25) = launches per step."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'polymer-chemprop_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from chemprop_amd import TrainArgs, synthetic, train  # noqa: E402
from chemprop_amd.featurization import BatchMolGraph, get_bond_fdim  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402

BATCH, WARMUP, REPEATS, N_BATCHES = 64, 20, 3, 4
FF, T, PHASES = 200, 1801, 2


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--model', default='regression', choices=['regression', 'spectra'])
    ap.add_argument('--variants', nargs='+', default=['list', 'direct', 'cached'],
                    choices=['list', 'direct', 'frozen', 'cached'])
    ap.add_argument('--no_features', action='store_true')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--label', default='this tree')
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    spectra = a.model == 'spectra'
    try:
        from chemprop_amd.features import FeatureTable
    except ImportError:
        FeatureTable = None
    rng = np.random.default_rng(0)
    n = N_BATCHES * BATCH
    feats = np.eye(PHASES)[rng.integers(PHASES, size=n)] if spectra else rng.standard_normal((n, FF))
    ff = 0 if a.no_features else feats.shape[1]
    args = TrainArgs(hidden_size=300, depth=3, device=dev, dataset_type=a.model, num_tasks=T if spectra else 1,
                     use_input_features=ff > 0, features_size=ff)
    loss_func = train.get_loss_func(a.model)
    mols = [synthetic.make_batch('polymer', BATCH, 9000 + i) for i in range(N_BATCHES)]
    batches = []
    for i, m in enumerate(mols):
        g = BatchMolGraph(m, device_bond_features=True)
        g.device_graph(dev, False, get_bond_fdim())
        if spectra:
            from chemprop_amd import spectra_utils
            raw = rng.gamma(2.0, size=(BATCH, T)) + 0.01
            raw[rng.random((BATCH, T)) < 0.1] = np.nan
            tg = np.array(spectra_utils.normalize_spectra(raw, threshold=1e-8, excluded_sub_value=np.nan),
                          dtype=np.float64)
        else:
            tg = [[float(rng.normal())] for _ in range(BATCH)]
        batches.append(([g], tg))
    modes = {}
    for name in a.variants:
        if name != 'list' and ff and FeatureTable is None:
            continue
        torch.manual_seed(0)
        m = MoleculeModel(args)
        initialize_weights(m)
        if name in ('frozen', 'cached'):
            for p in m.encoder.parameters():
                p.requires_grad = False
        m = m.to(dev).train()
        rows = train.frozen_encodings(m, [g for b in mols for g in b], BATCH) if name == 'cached' else None
        table = FeatureTable(feats, dev) if ff and name != 'list' else None
        modes[name] = (m, train.build_optimizer(m, 1e-4), rows, table)

    def step(name, i, index):
        m, opt, rows, _ = modes[name]
        k = i % N_BATCHES
        s = slice(BATCH * k, BATCH * (k + 1))
        kw = {}
        if ff:
            kw['features_batch'] = index[s] if index is not None else [feats[r] for r in range(s.start, s.stop)]
        if rows is not None:
            kw['encodings'] = rows[s]
        return train.train_step(m, None if rows is not None else batches[k][0], batches[k][1], loss_func, opt,
                                dataset_type=a.model, **kw)

    ms = {name: [] for name in modes}
    last = {}
    for _ in range(REPEATS):
        for name in modes:
            table = modes[name][3]
            index = table.index(range(n)) if table is not None else None  # (one upload per "epoch")
            for i in range(WARMUP):
                step(name, i, index)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(a.steps):
                loss = step(name, i, index)
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            last[name] = float(loss)
    what = f'T = {T}, SID, {PHASES} phase features' if spectra else f'1 task, {FF} features'
    if a.no_features:
        what += ' LEFT OUT (the model without input features)'
    lines = [f'features step [{a.label}]: {a.model} model, polymer B = {BATCH}, hidden 300, depth 3, 2-layer FFN, {what}; '
             f'{WARMUP} warm-up + {a.steps} timed steps per repeat, variants alternated {REPEATS} times in one process; '
             f'resident feature tables in this tree: {"yes" if FeatureTable is not None else "no"}',
             f'device: {torch.cuda.get_device_name(dev)}']
    for name, v in ms.items():
        lines.append(f'    {name:7s} ms/step: ' + ' '.join(f'{x:.4f}' for x in v) +
                     f'   median {statistics.median(v):.4f}   spread {max(v) - min(v):.4f}   last loss {last[name]:.9g}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
