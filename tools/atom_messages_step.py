"""Time atom-message models (``chemprop_train --atom_messages``) on device-built and on host-packed graphs.

    python tools/atom_messages_step.py [--min_seconds 0.3] [--repeats 5] [--out FILE]

Polymer batches of B = 50 and B = 64, hidden 300, depth 3, a two-layer FFN with one regression task, HipAdam.
Two versions of the same molecules:

* ``device``: ``BatchMolGraph(mols)``: the compact codes on the wire, the atom-message graph built on the device
  (``wdmpnn_build_graph_atom``), ``train_step`` on the direct path;
* ``host``: ``BatchMolGraph(mols, compact=False)``: gather lists, their transposes, the ELL rows and the per-atom
  bond-feature sums packed in Python, dense rows uploaded, and ``train_step(direct=False)``, the autograd path:
  what an atom-message model ran before the device build, reproduced in this process.

Legs, alternated ``--repeats`` times in one process, each a window of at least ``--min_seconds`` that ends in a
device synchronise (after WARMUP calls):

* ``prepare``: host milliseconds per batch to make a fresh ``BatchMolGraph`` and call its ``device_graph`` (which only
  enqueues; the synchronise is outside the clock), and the bytes uploaded per directed bond;
* ``forward``: a fresh batch made and encoded (eval mode, ``no_grad``), synchronised window, ms per batch;
* ``step``: ``train_step`` on resident graphs: ``device`` graphs on the direct path, ``device`` graphs on the autograd
  path (``device/autograd``: the step alone), ``host`` graphs on the autograd path;
* ``epoch``: 2048 polymers, shuffled, one step per slice of B: batches packed per step on the ``host`` version
  (autograd), per step on the ``device`` version (what the command runs without ``--resident_graphs``), and from
  a resident ``GraphTable`` (``--resident_graphs``).

Per leg and version: every repeat, the median and the spread (max - min).  A version counts as faster only where
its median is below the other's by more than the other's spread."""
import argparse
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
from chemprop_amd.graph_table import GraphTable  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402

WARMUP, N_BATCHES, N_MOLS, HIDDEN, DEPTH = 10, 8, 2048, 300, 3
FB = get_bond_fdim(atom_messages=True)


def new_model(dev):
    torch.manual_seed(0)
    m = MoleculeModel(TrainArgs(hidden_size=HIDDEN, depth=DEPTH, atom_messages=True, dataset_type='regression',
                                num_tasks=1, device=dev))
    initialize_weights(m)
    m = m.to(dev)
    return m, train.build_optimizer(m, 1e-4)


def window(fn, dev, min_seconds, host_clock=False):
    """ms per call over a window of >= min_seconds; ``host_clock``: only the time inside the calls (they enqueue)."""
    for i in range(WARMUP):
        fn(i)
    torch.cuda.synchronize(dev)
    n, spent, t0 = 0, 0.0, time.perf_counter()
    while True:
        h0 = time.perf_counter()
        for i in range(10):
            fn(n + i)
        spent += time.perf_counter() - h0
        n += 10
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return (spent if host_clock else dt) / n * 1e3


def report(say, leg, name, x, unit='ms'):
    say(f'    {leg:8s} {name:15s} {unit}: ' + ' '.join(f'{t:.4f}' for t in x) +
        f'   median {statistics.median(x):.4f}   spread {max(x) - min(x):.4f}')


def verdict(say, what, new, old):
    mn, mo = statistics.median(new), statistics.median(old)
    spread = max(max(old) - min(old), max(new) - min(new))
    word = 'FASTER' if mo - mn > spread else 'SLOWER' if mn - mo > spread else 'NOT distinguishable'
    say(f'    -> {what}: {mo / mn:.2f}x, {word} (difference {mo - mn:.4f}, larger spread {spread:.4f})')


def epoch(path, model, opt, graphs, targets, B, dev, sampler, table):
    order = list(range(len(graphs)))
    sampler.shuffle(order)
    loss_func = train.get_loss_func('regression')
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    index = table.index(order) if table is not None else None
    losses = []
    for s in range(0, len(order), B):
        pos = order[s:s + B]
        if index is not None:
            g = index[s:s + B].batch()
        else:
            g = BatchMolGraph([graphs[p] for p in pos], compact=path != 'host')
        losses.append(train.train_step(model, [g], [targets[p] for p in pos], loss_func, opt, direct=path != 'host'))
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, torch.stack(losses).cpu()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--min_seconds', type=float, default=0.3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch_sizes', nargs='+', type=int, default=[50, 64])
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say(f'atom messages: polymer batches, hidden {HIDDEN}, depth {DEPTH}, 2-layer FFN, 1 task, HipAdam; {WARMUP} warm-up '
        f'calls, then windows of >= {a.min_seconds:g} s ending in a synchronise; versions alternated {a.repeats} times in one '
        f'process ({torch.cuda.get_device_name(dev)})')
    loss_func = train.get_loss_func('regression')
    for B in a.batch_sizes:
        mols = [synthetic.make_batch('polymer', B, 7000 + i) for i in range(N_BATCHES)]
        targets = [[[float(v)] for v in torch.randn(B, generator=torch.Generator().manual_seed(i))]
                   for i in range(N_BATCHES)]
        model, opt = new_model(dev)
        enc = model.encoder.encoder[0]
        compact = {'device': True, 'host': False}
        resident = {n: [BatchMolGraph(m, compact=c) for m in mols] for n, c in compact.items()}
        dgs = {n: [g.device_graph(dev, True, FB) for g in gs] for n, gs in resident.items()}
        assert all(d.built_on_device for d in dgs['device']) and not any(d.built_on_device for d in dgs['host'])
        edges = sum(d.n_edges for d in dgs['device']) / N_BATCHES

        def prepare(name, i):
            BatchMolGraph(mols[i % N_BATCHES], compact=compact[name]).device_graph(dev, True, FB)

        def forward(name, i):
            with torch.no_grad():
                enc(BatchMolGraph(mols[i % N_BATCHES], compact=compact[name]))

        def step(name, i):
            k = i % N_BATCHES
            graphs = resident['host' if name == 'host' else 'device']
            train.train_step(model, [graphs[k]], targets[k], loss_func, opt, direct=name == 'device')

        legs = (('prepare', prepare, ('device', 'host'), True), ('forward', forward, ('device', 'host'), False),
                ('step', step, ('device', 'device/autograd', 'host'), False))
        ms = {(leg, n): [] for leg, _, names, _ in legs for n in names}
        for _ in range(a.repeats):
            for leg, fn, names, host_clock in legs:
                for n in names:
                    model.train(leg == 'step')
                    ms[(leg, n)].append(window(lambda i: fn(n, i), dev, a.min_seconds, host_clock))
        say(f'\nB = {B}: {edges:.0f} directed bonds per batch')
        for leg, _, names, _ in legs:
            for n in names:
                report(say, leg, n, ms[(leg, n)])
            verdict(say, f'{leg}: device against host', ms[(leg, 'device')], ms[(leg, 'host')])
        verdict(say, 'step: direct against autograd on the same graphs', ms[('step', 'device')],
                ms[('step', 'device/autograd')])
        for n in compact:
            h2d = sum(d.h2d_bytes for d in dgs[n]) / N_BATCHES
            say(f'    upload   {n:15s} bytes per batch: {h2d:.0f} ({h2d / edges:.1f} per directed bond)')
        del resident, dgs

        # the epoch
        graphs = synthetic.make_batch('polymer', N_MOLS, 0)
        tg = [[float(v)] for v in np.random.default_rng(1).normal(size=N_MOLS)]
        t0 = time.perf_counter()
        table = GraphTable(graphs, dev)
        torch.cuda.synchronize(dev)
        table_ms = 1e3 * (time.perf_counter() - t0)
        paths = {}
        for name in ('host', 'device', 'table'):
            m, o = new_model(dev)
            paths[name] = dict(model=m.train(), opt=o, sampler=Random(0), table=table if name == 'table' else None)
        run = lambda n: epoch(n, paths[n]['model'], paths[n]['opt'], graphs, tg, B, dev, paths[n]['sampler'],  # noqa: E731
                              paths[n]['table'])
        res = {n: [] for n in paths}
        for n in paths:
            run(n)  # warm-up: packs, plans, allocator
        for r in range(a.repeats):
            for n in (list(paths) if r % 2 == 0 else list(paths)[::-1]):
                res[n].append(run(n))
        steps = -(-N_MOLS // B)
        say(f'    epoch over {N_MOLS} polymers, {steps} steps (GraphTable built once in {table_ms:.0f} ms):')
        for n in paths:
            report(say, 'epoch', {'host': 'host', 'device': 'device', 'table': 'device/resident'}[n],
                   [1e3 * w for w, _ in res[n]])
        walls = {n: [1e3 * w for w, _ in res[n]] for n in paths}
        verdict(say, 'epoch: device against host', walls['device'], walls['host'])
        verdict(say, 'epoch: resident table against device', walls['table'], walls['device'])
        same = {n: all(torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))
                       for x, y in zip(res[n], res['device'])) for n in ('host', 'table')}
        say(f'    losses of every epoch bitwise equal to the device path\'s: host {same["host"]}, '
            f'resident table {same["table"]}')
        del paths, table
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
