"""Time the training step for the FFN heads the stack head (wdmpnn_head_stack) covers, against ``fused_head=False``
(the torch ops of the reference's step under the autograd engine).

    python tools/head_stack_step.py [--out FILE]

Polymer batches of 128, hidden 300, depth 3, one regression task.  Configurations:

    a  dropout 0.1                                  (two-layer head, masks active)
    b  ffn_num_layers 3
    c  dropout 0.1, ffn_num_layers 3, PReLU
    d  the default head                             (control: wdmpnn_head_mse, must not move)

Per repeat: 20 warm-up steps, then 200 timed steps ending in a synchronise; per configuration the two modes
('fused': train_step's defaults, 'torch': fused_head=False) alternate three times in ONE process (each mode keeps
its own model and optimizer, same seed).  Reports each repeat, both medians and the spread (max - min) between the
repeats of one mode.  On a tree without the stack head both modes of a, b and c run the torch ops (the 'head'
column says which head the fused mode found), which is the baseline this tree's 'fused' medians are compared
with: the stack head counts as faster only when the medians differ by more than the largest spread of either
run."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'polymer-chemprop_amd')]
import torch  # noqa: E402

from chemprop_amd import TrainArgs, synthetic  # noqa: E402
from chemprop_amd.featurization import BatchMolGraph, get_bond_fdim  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402
from chemprop_amd.train import _fusable_head, build_optimizer, get_loss_func, train_step  # noqa: E402

BATCH, WARMUP, STEPS, REPEATS = 128, 20, 200, 3
CONFIGS = (('a', dict(dropout=0.1)),
           ('b', dict(ffn_num_layers=3)),
           ('c', dict(dropout=0.1, ffn_num_layers=3, activation='PReLU')),
           ('d', dict()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--label', default='', help='a name for this run in the report (the tree it measures)')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    loss_func = get_loss_func('regression')
    batches = []
    for i in range(4):
        g = BatchMolGraph(synthetic.make_batch('polymer', BATCH, 7000 + i), device_bond_features=True)
        g.device_graph(dev, False, get_bond_fdim())
        batches.append(([g], [[0.01 * ((7 * j + i) % 50) - 0.25] for j in range(BATCH)]))
    lines = [f'head stack training step{" [" + a.label + "]" if a.label else ""}: polymer B = {BATCH}, hidden 300, '
             f'depth 3, 1 regression task; {WARMUP} warm-up + {STEPS} timed steps per repeat, modes alternated '
             f'{REPEATS} times in one process', f'device: {torch.cuda.get_device_name(dev)}']
    for tag, extra in CONFIGS:
        args = TrainArgs(hidden_size=300, depth=3, device=dev, **extra)
        modes = {}
        for name, kw in (('fused', {}), ('torch', dict(fused_head=False))):
            torch.manual_seed(0)
            m = MoleculeModel(args)
            initialize_weights(m)
            m = m.to(dev).train()
            modes[name] = (m, build_optimizer(m, 1e-4), kw)
        head = _fusable_head(modes['fused'][0], loss_func, 'regression')
        kind = 'torch ops' if head is None else 'two-layer' if isinstance(head, tuple) else 'stack'
        ms = {name: [] for name in modes}
        last = {}
        for _ in range(REPEATS):
            for name, (m, opt, kw) in modes.items():
                for i in range(WARMUP):
                    train_step(m, *batches[i % 4], loss_func, opt, **kw)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for i in range(STEPS):
                    loss = train_step(m, *batches[i % 4], loss_func, opt, **kw)
                torch.cuda.synchronize(dev)
                ms[name].append((time.perf_counter() - t0) / STEPS * 1e3)
                last[name] = float(loss)
        lines.append(f'({tag}) {extra or "default"}   head: {kind}')
        for n in ms:
            lines.append(f'    {n:5s} ms/step: ' + ' '.join(f'{v:.4f}' for v in ms[n]) +
                         f'   median {statistics.median(ms[n]):.4f}   spread {max(ms[n]) - min(ms[n]):.4f}   '
                         f'last loss {last[n]:.6f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
