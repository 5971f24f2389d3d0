"""Time inference and the training step on batches with extra atom / bond features (``--atom_features_path``,
``--bond_features_path``).

    python tools/extra_features_step.py [--min_seconds 0.5] [--out FILE]

Polymer batches of B = 50 and B = 64, hidden 300, depth 3, a two-layer FFN with one regression task, with
``(da, db)`` = (4, 3) -- bond_fdim 154: the code embed with its dense tail -- and (40, 10) -- bond_fdim 197: the
plane-GEMM input layer on device-built rows.  Per case two versions of the same widened molecules:

* ``compact``: ``BatchMolGraph(mols)``: codes + the two dense sections on the wire, the graph built on the device;
* ``host``: ``BatchMolGraph(mols, compact=False)``: gather lists packed on the host, fp32 rows uploaded -- the only
  path such batches had before the compact format carried extras.

Legs, ms per call: ``forward`` (the eval-mode ``no_grad`` encoder forward on resident graphs) and ``step``
(``train.train_step``, HipAdam's update included).  The versions are alternated REPEATS times in one process; per
repeat WARMUP calls, then a device-synchronised window of at least ``--min_seconds``.  Reported per version: every
repeat, the median and the spread (max - min); the host-to-device bytes per batch of its device graphs; the library
entry points called per forward and per step (counted on the ctypes handle, outside the timed windows).  For (4, 3)
the forward of the same molecules WITHOUT extras (``base``) is timed beside it: the cost of the tail."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'polymer-chemprop_amd')]
import torch  # noqa: E402

from chemprop_amd import TrainArgs, _native, synthetic, train  # noqa: E402
from chemprop_amd import featurization as F  # noqa: E402
from chemprop_amd.featurization import BatchMolGraph  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402

WARMUP, REPEATS, N_BATCHES = 20, 5, 4
CASES = [(B, da, db) for B in (50, 64) for da, db in ((4, 3), (40, 10))]


def timed(fn, dev, min_seconds):
    for i in range(WARMUP):
        fn(i)
    torch.cuda.synchronize(dev)
    n, t0 = 0, time.perf_counter()
    while True:
        for i in range(50):
            fn(n + i)
        n += 50
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / n * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--min_seconds', type=float, default=0.5)
    ap.add_argument('--label', default='this tree')
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    loss_func = train.get_loss_func('regression')
    lines = [f'extra features [{a.label}]: polymer batches, hidden 300, depth 3, 2-layer FFN, 1 task; {N_BATCHES} resident '
             f'batches per case; {WARMUP} warm-up calls, then windows of >= {a.min_seconds:g} s ending in a synchronise, '
             f'versions alternated {REPEATS} times in one process',
             f'device: {torch.cuda.get_device_name(dev)}']
    for B, da, db in CASES:
        base_mols = [synthetic.make_batch('polymer', B, 9000 + i) for i in range(N_BATCHES)]
        wide_mols = [synthetic.with_extra_features(m, da, db, 50 + i) for i, m in enumerate(base_mols)]
        targets = [[[float(v)] for v in torch.randn(B, generator=torch.Generator().manual_seed(i))]
                   for i in range(N_BATCHES)]
        versions = {'compact': dict(mols=wide_mols, compact=True, dims=(da, db)),
                    'host': dict(mols=wide_mols, compact=False, dims=(da, db))}
        if (da, db) == (4, 3):
            versions['base'] = dict(mols=base_mols, compact=True, dims=(0, 0))
        for name, v in versions.items():
            F.set_extra_atom_fdim(v['dims'][0])
            F.set_extra_bond_fdim(v['dims'][1])
            torch.manual_seed(0)
            m = MoleculeModel(TrainArgs(hidden_size=300, depth=3, device=dev))
            initialize_weights(m)
            v['model'] = m.to(dev)
            v['opt'] = train.build_optimizer(v['model'], 1e-4)
            v['graphs'] = [BatchMolGraph(x, compact=v['compact']) for x in v['mols']]
            enc = v['model'].encoder.encoder[0]
            dgs = [g.device_graph(dev, False, enc.bond_fdim) for g in v['graphs']]
            assert all(d.built_on_device == v['compact'] for d in dgs)
            v['h2d'] = sum(d.h2d_bytes for d in dgs) / len(dgs)
            v['edges'] = sum(d.n_edges for d in dgs) / len(dgs)

        def forward(v, i):
            with torch.no_grad():
                return v['model'].encoder.encoder[0](v['graphs'][i % N_BATCHES])

        def step(v, i):
            k = i % N_BATCHES
            return train.train_step(v['model'], [v['graphs'][k]], targets[k], loss_func, v['opt'])

        legs = {'forward': forward, 'step': step}
        ms = {(leg, name): [] for leg in legs for name in versions}
        for _ in range(REPEATS):
            for leg, fn in legs.items():
                for name, v in versions.items():
                    v['model'].train(leg == 'step')
                    ms[(leg, name)].append(timed(lambda i: fn(v, i), dev, a.min_seconds))
        lines.append(f'B = {B}, (da, db) = ({da}, {db}): atom_fdim {133 + da}, bond_fdim {147 + da + db}, '
                     f'{versions["compact"]["edges"]:.0f} directed bonds per batch')
        for (leg, name), x in ms.items():
            lines.append(f'    {leg:7s} {name:7s} ms: ' + ' '.join(f'{t:.4f}' for t in x) +
                         f'   median {statistics.median(x):.4f}   spread {max(x) - min(x):.4f}')
        for name, v in versions.items():
            lines.append(f'    h2d     {name:7s} bytes per batch: {v["h2d"]:.0f} ({v["h2d"] / v["edges"]:.1f} per directed bond)')
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
        try:
            for leg, fn in legs.items():
                for name, v in versions.items():
                    v['model'].train(leg == 'step')
                    seen.clear()
                    fn(v, 0)
                    torch.cuda.synchronize(dev)
                    lines.append(f'    {leg:7s} {name:7s} library calls: ' +
                                 ', '.join(f'{k[len("wdmpnn_"):]} x{n}' for k, n in sorted(seen.items())))
        finally:
            _native.lib = lambda: real
        del versions
    F.set_extra_atom_fdim(0)
    F.set_extra_bond_fdim(0)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
