"""Time an epoch of direct training steps with the graphs packed on the host per step and with a resident GraphTable.

    python tools/resident_graphs_epoch.py [--paths list table] [--batch_sizes 50 64] [--repeats 5] [--out FILE]

A synthetic polymer data set of 2048 molecules (``chemprop_amd.synthetic``), hidden 300, depth 3, a two-layer FFN,
regression, HipAdam.  An epoch is what ``chemprop_train`` runs per epoch without its scoring: the order is
shuffled, and every slice of B positions becomes a batch and takes one ``train_step`` (the direct step).

* ``list``: ``BatchMolGraph([graphs[p] for p in pos])`` per step, the loop of ``cli.train_model`` as it is without
  ``--resident_graphs`` (native pack, compact encode, plan, one H2D of the image, one build launch).  This is the
  baseline: it runs no code of ``chemprop_amd.graph_table``.
* ``table``: one ``GraphTable`` per process, one index upload per epoch, per step a slice of it
  (``index[s:s + B].batch()``: host plan, two small H2D copies, one gather launch, the same build launch).

Both paths run in ONE process with their own model and optimizer (same seed), alternating (list, table, table,
list, ...), ``--repeats`` timed epochs each after one warm-up epoch each.  Per path and batch size:

* host milliseconds per step spent preparing the graph: the wall time of building the batch and calling its
  ``device_graph`` (which only enqueues), summed over the epoch and divided by the steps;
* the wall time of the epoch (synchronised at its end), per repeat, with the median and the spread (max - min);
* the losses of the two paths' first timed epochs, compared bitwise.

The table path counts as faster only if its median epoch is lower than the list path's by more than the list
path's own spread.

Launches per step come from a traced run of its own (tracing slows the host): under
``rocprofv3 --kernel-trace --stats`` run ``--paths list --batch_sizes 64 --repeats 1``, the same with ``table``, then
``--kernel_stats list=DIR table=DIR --traced_steps N`` (N = the steps the traced runs printed) adds
calls / N per path to the report."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time
from random import Random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'polymer-chemprop_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from chemprop_amd import TrainArgs, synthetic, train  # noqa: E402
from chemprop_amd.featurization import BatchMolGraph, get_bond_fdim  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402

N_MOLS, HIDDEN, DEPTH = 2048, 300, 3


class Path:
    """One path's model, optimizer and epoch loop."""

    def __init__(self, name, graphs, targets, B, dev):
        self.name, self.graphs, self.targets, self.B, self.dev = name, graphs, targets, B, dev
        torch.manual_seed(0)
        args = TrainArgs(hidden_size=HIDDEN, depth=DEPTH, dataset_type='regression', num_tasks=1, device=dev)
        self.model = MoleculeModel(args)
        initialize_weights(self.model)
        self.model = self.model.to(dev).train()
        self.opt = train.build_optimizer(self.model, 1e-4)
        self.loss_func = train.get_loss_func('regression')
        self.sampler = Random(0)
        self.table = None
        if name == 'table':
            from chemprop_amd.graph_table import GraphTable
            t0 = time.perf_counter()
            self.table = GraphTable(graphs, dev)
            torch.cuda.synchronize()
            self.table_s = time.perf_counter() - t0

    def epoch(self):
        """(wall seconds, host seconds preparing graphs, steps, losses)."""
        order = list(range(len(self.graphs)))
        self.sampler.shuffle(order)
        B, fdim = self.B, get_bond_fdim()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prep, losses = 0.0, []
        index = self.table.index(order) if self.table is not None else None
        for s in range(0, len(order), B):
            pos = order[s:s + B]
            p0 = time.perf_counter()
            g = index[s:s + B].batch() if index is not None else BatchMolGraph([self.graphs[p] for p in pos])
            g.device_graph(self.dev, False, fdim)
            prep += time.perf_counter() - p0
            losses.append(train.train_step(self.model, [g], [self.targets[p] for p in pos], self.loss_func, self.opt))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return wall, prep, len(losses), torch.stack(losses).cpu()


def launches(stats_dir, steps):
    files = glob.glob(os.path.join(stats_dir, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit(f'no *kernel_stats.csv under {stats_dir}')
    rows = list(csv.DictReader(open(files[0])))
    calls = sum(int(r['Calls']) for r in rows)
    gather = sum(int(r['Calls']) for r in rows if 'gather_compact_kernel' in r['Name'])
    build = sum(int(r['Calls']) for r in rows if 'build_graph' in r['Name'] or 'graph_build' in r['Name'])
    return calls / steps, gather / steps, build / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--paths', nargs='+', default=['list', 'table'], choices=['list', 'table'])
    ap.add_argument('--batch_sizes', nargs='+', type=int, default=[50, 64])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernel_stats', nargs='*', default=[], help='PATH=DIR of a traced run\'s rocprofv3 output')
    ap.add_argument('--traced_steps', type=int, default=0)
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    if a.kernel_stats:
        say(f'kernel launches per step (rocprofv3 --kernel-trace --stats, {a.traced_steps} steps incl. the first-use ones):')
        for item in a.kernel_stats:
            name, d = item.split('=', 1)
            total, gather, build = launches(d, a.traced_steps)
            say(f'  {name:5s}: {total:6.2f} launches per step, of them gather_compact {gather:.2f}, graph build '
                f'{build:.2f}')
    else:
        dev = torch.device('cuda:0')
        graphs = synthetic.make_batch('polymer', N_MOLS, 0)
        rng = np.random.default_rng(1)
        targets = [[float(v)] for v in rng.normal(size=N_MOLS)]
        say(f'{N_MOLS} synthetic polymers, hidden {HIDDEN}, depth {DEPTH}, direct steps, {a.repeats} timed epochs per '
            f'path after one warm-up epoch each, paths alternating in one process ({torch.cuda.get_device_name(0)})')
        for B in a.batch_sizes:
            paths = [Path(n, graphs, targets, B, dev) for n in a.paths]
            for p in paths:
                p.epoch()  # warm-up: packs, plans, allocator
            res = {p.name: [] for p in paths}
            for r in range(a.repeats):
                for p in (paths if r % 2 == 0 else paths[::-1]):
                    res[p.name].append(p.epoch())
            say(f'\nB = {B}: {res[paths[0].name][0][2]} steps per epoch, '
                f'{(a.repeats + 1) * res[paths[0].name][0][2]} steps run per path')
            for p in paths:
                walls = [w for w, _, _, _ in res[p.name]]
                preps = [1e3 * h / n for _, h, n, _ in res[p.name]]
                say(f'  {p.name:5s}: epoch ms ' + ' '.join(f'{1e3 * w:7.1f}' for w in walls) +
                    f' | median {1e3 * statistics.median(walls):7.1f} spread {1e3 * (max(walls) - min(walls)):6.1f}'
                    f' | per step {1e3 * statistics.median(walls) / res[p.name][0][2]:.3f} ms'
                    f' | graph preparation on the host {statistics.median(preps):.3f} ms per step')
                if p.table is not None:
                    say(f'         (GraphTable of {N_MOLS} molecules built once in {1e3 * p.table_s:.0f} ms)')
            if len(paths) == 2:
                (l, t) = (res['list'], res['table'])
                same = all(torch.equal(x[3].view(torch.int32), y[3].view(torch.int32)) for x, y in zip(l, t))
                ml, mt = statistics.median(w for w, *_ in l), statistics.median(w for w, *_ in t)
                spread = max(w for w, *_ in l) - min(w for w, *_ in l)
                say(f'  losses of every epoch bitwise equal between the paths: {same}')
                verdict = 'FASTER' if ml - mt > spread else 'NOT faster'
                say(f'  table median is {1e3 * (ml - mt):.1f} ms below the list median (list spread '
                    f'{1e3 * spread:.1f} ms): the table path is {verdict} by the acceptance rule '
                    f'(ratio {ml / mt:.2f}x)')
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
