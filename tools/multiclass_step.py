"""Time the multiclass training step with the fused head (train_step's default arguments: wdmpnn_head_mse with
the softmax cross-entropy, the direct step, HipAdam's repack) against ``fused_head=False`` (the torch ops of
the reference's step: ffn, reshape, CrossEntropyLoss per task, weights, mask, autograd backward).

    python tools/multiclass_step.py [--out profiles/multiclass_step.txt]

Polymer batches of 128, hidden 300, depth 3, one task x 3 classes.  Per repeat: 20 warm-up steps, then 200
timed steps ending in a synchronise; the two modes alternate three times in ONE process (each mode keeps its
own model and optimizer, same seed).  Reports each repeat, both medians and the spread (max - min) between the
repeats of the same mode; the fused step counts as faster only when the medians differ by more than that."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'polymer-chemprop_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from chemprop_amd import TrainArgs, synthetic  # noqa: E402
from chemprop_amd.featurization import BatchMolGraph, get_bond_fdim  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402
from chemprop_amd.train import _fusable_head, build_optimizer, get_loss_func, train_step  # noqa: E402

BATCH, CLASSES, WARMUP, STEPS, REPEATS = 128, 3, 20, 200, 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    args = TrainArgs(hidden_size=300, depth=3, device=dev, dataset_type='multiclass', multiclass_num_classes=CLASSES)
    loss_func = get_loss_func('multiclass')
    rng = np.random.default_rng(0)
    batches = []
    for i in range(4):
        g = BatchMolGraph(synthetic.make_batch('polymer', BATCH, 7000 + i), device_bond_features=True)
        g.device_graph(dev, False, get_bond_fdim())
        batches.append(([g], [[float(rng.integers(CLASSES))] for _ in range(BATCH)]))
    modes = {}
    for name, kw in (('fused', {}), ('torch', dict(fused_head=False))):
        torch.manual_seed(0)
        m = MoleculeModel(args)
        initialize_weights(m)
        m = m.to(dev)
        assert _fusable_head(m, loss_func, 'multiclass') is not None
        modes[name] = (m, build_optimizer(m, 1e-4), kw)
    ms = {name: [] for name in modes}
    last = {}
    for _ in range(REPEATS):
        for name, (m, opt, kw) in modes.items():
            for i in range(WARMUP):
                train_step(m, *batches[i % 4], loss_func, opt, dataset_type='multiclass', **kw)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(STEPS):
                loss = train_step(m, *batches[i % 4], loss_func, opt, dataset_type='multiclass', **kw)
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) / STEPS * 1e3)
            last[name] = float(loss)
    med = {n: statistics.median(v) for n, v in ms.items()}
    spread = {n: max(v) - min(v) for n, v in ms.items()}
    lines = [f'multiclass training step: polymer B = {BATCH}, hidden 300, depth 3, 1 task x {CLASSES} classes; '
             f'{WARMUP} warm-up + {STEPS} timed steps per repeat, modes alternated {REPEATS} times in one process',
             f'device: {torch.cuda.get_device_name(dev)}']
    for n in ms:
        lines.append(f'{n:5s} ms/step: ' + ' '.join(f'{v:.4f}' for v in ms[n]) +
                     f'   median {med[n]:.4f}   spread {spread[n]:.4f}   last loss {last[n]:.6f}')
    gain = med['torch'] - med['fused']
    worst = max(spread.values())
    lines.append(f'torch - fused = {gain:.4f} ms/step ({med["torch"] / med["fused"]:.2f}x), largest spread between '
                 f'repeats of one mode {worst:.4f} ms: ' +
                 ('fused is faster' if gain > worst else 'NO difference beyond the spread'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
