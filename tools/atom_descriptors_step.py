"""Time inference and the training step of a model with atom descriptors (``--atom_descriptors descriptor``).

    python tools/atom_descriptors_step.py [--variants table list] [--min_seconds 1.0] [--out FILE]

Polymer batches of 64, hidden 300, depth 3, 12 descriptors per atom, a two-layer FFN with one regression task.  Two
legs, each in ms per call:

* ``forward``: the eval-mode, ``no_grad`` encoder forward ``model.encoder([graph], None, descriptors)``;
* ``step``: one training step, HipAdam's update included.

Two versions, each with its own model and optimizer (same seed), alternated REPEATS times in ONE process; per
repeat 20 warm-up calls, then a device-synchronised window of at least ``--min_seconds``:

* ``table``: the batch is ``AtomDescriptorRows`` of a resident ``AtomDescriptorTable``: the descriptor-free fused
  forward, then the join and the layer on B rows; the step is ``train.train_step``'s direct step;
* ``list``: the batch is a list of numpy arrays -- padded on the host, copied to the device, the per-atom layer on
  the unblocked path.  Its step is ``model(batch, None, desc)``, ``batch_loss``, ``backward``, ``optimizer.step()``.
  On a tree without ``chemprop_amd.atom_descriptors`` this is the only version such a model has (the parent
  commit's: run this file there, it then measures ``list`` alone).

``--count_launches``: also report the library entry points called per forward and per step (counted on the
ctypes handle, outside the timed windows).  Reports every repeat, the medians and the spread (max - min) between
the repeats of one version; two medians differ only when they are further apart than the larger spread."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'polymer-chemprop_amd')]
import torch  # noqa: E402

from chemprop_amd import TrainArgs, _native, synthetic, train  # noqa: E402
from chemprop_amd.featurization import BatchMolGraph, get_bond_fdim  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402

BATCH, WARMUP, REPEATS, N_BATCHES, D = 64, 20, 3, 4, 12


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--variants', nargs='+', default=['table', 'list'], choices=['table', 'list'])
    ap.add_argument('--min_seconds', type=float, default=1.0)
    ap.add_argument('--count_launches', action='store_true')
    ap.add_argument('--label', default='this tree')
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    try:
        from chemprop_amd.atom_descriptors import AtomDescriptorTable
    except ImportError:
        AtomDescriptorTable = None
    args = TrainArgs(hidden_size=300, depth=3, device=dev, atom_descriptors='descriptor', atom_descriptors_size=D)
    loss_func = train.get_loss_func('regression')
    mols = [synthetic.make_batch('polymer', BATCH, 9000 + i) for i in range(N_BATCHES)]
    desc = [synthetic.random_descriptors(m, D, 100 + i) for i, m in enumerate(mols)]
    graphs, targets = [], []
    for i, m in enumerate(mols):
        g = BatchMolGraph(m, device_bond_features=True)
        g.device_graph(dev, False, get_bond_fdim())
        graphs.append(g)
        gen = torch.Generator().manual_seed(i)
        targets.append([[float(v)] for v in torch.randn(BATCH, generator=gen)])
    modes = {}
    for name in a.variants:
        if name == 'table' and AtomDescriptorTable is None:
            continue
        torch.manual_seed(0)
        m = MoleculeModel(args)
        initialize_weights(m)
        m = m.to(dev)
        index = None
        if name == 'table':
            index = AtomDescriptorTable([x for d_ in desc for x in d_], dev).index(range(N_BATCHES * BATCH))
        modes[name] = (m, train.build_optimizer(m, 1e-4), index)

    def batch_desc(name, k):
        index = modes[name][2]
        return desc[k] if index is None else index[BATCH * k:BATCH * (k + 1)]

    def forward(name, i):
        m = modes[name][0]
        k = i % N_BATCHES
        with torch.no_grad():
            return m.encoder([graphs[k]], None, batch_desc(name, k))

    def step(name, i):
        m, opt, _ = modes[name]
        k = i % N_BATCHES
        if name == 'table':
            return train.train_step(m, [graphs[k]], targets[k], loss_func, opt,
                                    atom_descriptors_batch=batch_desc(name, k))
        opt.zero_grad(set_to_none=True)
        preds = m([graphs[k]], None, desc[k])
        loss = train.batch_loss(preds, targets[k], loss_func, 'regression')
        loss.backward()
        opt.step()
        return loss.detach()

    legs = {'forward': forward, 'step': step}
    ms = {(leg, name): [] for leg in legs for name in modes}
    for _ in range(REPEATS):
        for leg, fn in legs.items():
            for name in modes:
                modes[name][0].train(leg == 'step')
                for i in range(WARMUP):
                    fn(name, i)
                torch.cuda.synchronize(dev)
                n, t0 = 0, time.perf_counter()
                while True:
                    for i in range(50):
                        fn(name, n + i)
                    n += 50
                    torch.cuda.synchronize(dev)
                    dt = time.perf_counter() - t0
                    if dt >= a.min_seconds:
                        break
                ms[(leg, name)].append(dt / n * 1e3)
    lines = [f'atom descriptors [{a.label}]: polymer B = {BATCH}, hidden 300, depth 3, d = {D}, 2-layer FFN, 1 task; '
             f'{WARMUP} warm-up calls, then windows of >= {a.min_seconds:g} s ending in a synchronise, versions '
             f'alternated {REPEATS} times in one process; device tables in this tree: '
             f'{"yes" if AtomDescriptorTable is not None else "no"}',
             f'device: {torch.cuda.get_device_name(dev)}']
    for (leg, name), v in ms.items():
        lines.append(f'    {leg:7s} {name:5s} ms: ' + ' '.join(f'{x:.4f}' for x in v) +
                     f'   median {statistics.median(v):.4f}   spread {max(v) - min(v):.4f}')
    if a.count_launches:
        real = _native.lib()
        seen = {}

        class Counting:
            def __getattr__(self, fn_name):
                fn = getattr(real, fn_name)
                if not fn_name.startswith('wdmpnn_') or fn_name.endswith('_bytes') or \
                        fn_name in ('wdmpnn_last_error', 'wdmpnn_saved_layout'):
                    return fn

                def call(*args_):
                    seen[fn_name] = seen.get(fn_name, 0) + 1
                    return fn(*args_)
                return call
        _native.lib = lambda: Counting()
        for leg, fn in legs.items():
            for name in modes:
                modes[name][0].train(leg == 'step')
                seen.clear()
                fn(name, 0)
                torch.cuda.synchronize(dev)
                lines.append(f'    {leg:7s} {name:5s} library calls: ' +
                             ', '.join(f'{k[len("wdmpnn_"):]} x{v}' for k, v in sorted(seen.items())))
        _native.lib = lambda: real
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
