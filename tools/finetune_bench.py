"""Time the fine-tuning step: encoder and first FFN layer frozen, the rest trained.

    python tools/finetune_bench.py [--variants autograd direct cached] [--steps 200] [--out FILE]

Polymer batches of 64, hidden 300, depth 3, three-layer FFN, one regression task; the encoder's parameters and
ffn.1's weight and bias have ``requires_grad = False``.  Variants (each with its own model and optimizer, same
seed, alternated REPEATS times in ONE process; per repeat 20 warm-up steps, then the timed steps ending in a
synchronise):

* ``autograd``: ``train_step(..., direct=False)`` -- on a tree without the frozen direct step this is what every
  frozen model gets (the step of the parent commit: run this file there for its figure);
* ``direct``: ``train_step``'s default, the direct step of a frozen plan where the tree has one;
* ``cached``: the direct step from ``train.frozen_encodings`` rows (skipped where the tree has none).

Reports each repeat, the medians and the spread (max - min) between the repeats of one variant; two medians
differ only when they are further apart than the larger spread.  With ``--variants direct --steps 5`` under
``rocprofv3 --kernel-trace --stats`` (a run of its own) it gives the kernel list of the step."""
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

BATCH, WARMUP, REPEATS = 64, 20, 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--variants', nargs='+', default=['autograd', 'direct', 'cached'])
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--label', default='this tree')
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    args = TrainArgs(hidden_size=300, depth=3, ffn_num_layers=3, device=dev)
    loss_func = train.get_loss_func('regression')
    rng = np.random.default_rng(0)
    mols = [synthetic.make_batch('polymer', BATCH, 9000 + i) for i in range(4)]
    batches = []
    for m in mols:
        g = BatchMolGraph(m, device_bond_features=True)
        g.device_graph(dev, False, get_bond_fdim())
        batches.append(([g], [[float(rng.normal())] for _ in range(BATCH)]))
    has_plan = hasattr(train, '_frozen_plan')
    modes = {}
    for name in a.variants:
        if name == 'cached' and not hasattr(train, 'frozen_encodings'):
            continue
        torch.manual_seed(0)
        m = MoleculeModel(args)
        initialize_weights(m)
        for p in list(m.encoder.parameters()) + list(m.ffn[1].parameters()):
            p.requires_grad = False
        m = m.to(dev).train()
        kw = [dict(direct=False) if name == 'autograd' else {} for _ in batches]
        if name == 'cached':
            rows = train.frozen_encodings(m, [g for b in mols for g in b], BATCH)
            kw = [dict(encodings=rows[BATCH * i:BATCH * (i + 1)]) for i in range(len(batches))]
        modes[name] = (m, train.build_optimizer(m, 1e-4), kw)
    ms = {name: [] for name in modes}
    last = {}
    for _ in range(REPEATS):
        for name, (m, opt, kw) in modes.items():
            for i in range(WARMUP):
                train.train_step(m, *batches[i % 4], loss_func, opt, **kw[i % 4])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(a.steps):
                loss = train.train_step(m, *batches[i % 4], loss_func, opt, **kw[i % 4])
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            last[name] = float(loss)
    lines = [f'fine-tuning step [{a.label}]: polymer B = {BATCH}, hidden 300, depth 3, 3-layer FFN, encoder and ffn.1 '
             f'frozen; {WARMUP} warm-up + {a.steps} timed steps per repeat, variants alternated {REPEATS} times in one '
             f'process; frozen direct step in this tree: {"yes" if has_plan else "no"}',
             f'device: {torch.cuda.get_device_name(dev)}']
    for name, v in ms.items():
        lines.append(f'    {name:9s} ms/step: ' + ' '.join(f'{x:.4f}' for x in v) +
                     f'   median {statistics.median(v):.4f}   spread {max(v) - min(v):.4f}   last loss {last[name]:.6f}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
