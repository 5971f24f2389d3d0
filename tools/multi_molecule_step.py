"""Time one training step and one 2048-row prediction of a two-molecule model, natively and on the path such a
model took before it had one.

    python tools/multi_molecule_step.py [--what step predict] [--modes own shared] [--steps 200] [--out FILE]

Two molecules per row: a polymer (slot 0) and a qm9-sized molecule (slot 1); B = 50, hidden 300, depth 3, a
two-layer FFN, one regression task, no input features.  ``own``: one encoder per slot; ``shared``: ``mpn_shared``.

``step``: variants ``direct`` (``train_step`` on a ``SlotBatch``: the direct step, for a shared encoder over the
merged batch) and ``autograd`` (``direct=False`` on the plain list: N autograd forwards, ``torch.cat``, the head under
autograd, N backwards, a weight pack before every forward), each with its own model and optimizer from the same
seed, alternated REPEATS times in ONE process; per repeat 20 warm-up steps, then the timed steps ending in a
synchronise.  ``predict``: 2048 rows in batches of 50 through ``device_predictions`` (``native``: ``forward_many``
per group of eight batches, one ``wdmpnn_slots_join`` and the native head per batch) and through
``own_forward=True`` (per batch the model's own forward: N encoder calls, ``torch.cat``, the FFN's torch modules), the
graphs resident, each pass ending in a synchronise.

Reports each repeat, the medians and the spread (max - min) between the repeats of one variant; two medians differ
only when they are further apart than the larger spread.  With ``--what step --variants V --steps 5`` under
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
from chemprop_amd.ensemble import make_batches  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402
from chemprop_amd.predict import device_predictions  # noqa: E402
from chemprop_amd.slots import SlotBatch  # noqa: E402

BATCH, WARMUP, REPEATS, N_BATCHES, ROWS = 50, 20, 3, 4, 2048


def _report(lines, title, ms, extra):
    lines.append(title)
    for name, v in ms.items():
        lines.append(f'    {name:9s} ' + ' '.join(f'{x:.4f}' for x in v) +
                     f'   median {statistics.median(v):.4f}   spread {max(v) - min(v):.4f}   {extra[name]}')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--what', nargs='+', default=['step', 'predict'], choices=['step', 'predict'])
    ap.add_argument('--modes', nargs='+', default=['own', 'shared'], choices=['own', 'shared'])
    ap.add_argument('--variants', nargs='+', default=['direct', 'autograd'], choices=['direct', 'autograd'])
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    loss_func = train.get_loss_func('regression')
    lines = [f'multi-molecule model: polymer + qm9 slots, B = {BATCH}, hidden 300, depth 3, 2-layer FFN, 1 regression '
             f'task; device: {torch.cuda.get_device_name(dev)}']
    for mode in a.modes:
        shared = mode == 'shared'
        args = TrainArgs(hidden_size=300, depth=3, device=dev, number_of_molecules=2, mpn_shared=shared)

        def new_model():
            torch.manual_seed(0)
            m = MoleculeModel(args)
            initialize_weights(m)
            return m.to(dev)
        if 'step' in a.what:
            mols = [(synthetic.make_batch('polymer', BATCH, 9000 + i), synthetic.make_batch('qm9', BATCH, 9500 + i))
                    for i in range(N_BATCHES)]
            batches = [SlotBatch(list(m), shared=shared) for m in mols]
            targets = [[[float(rng.normal())] for _ in range(BATCH)] for _ in range(N_BATCHES)]
            models = {v: new_model().train() for v in a.variants}
            opts = {v: train.build_optimizer(m, 1e-4) for v, m in models.items()}
            ms, last = {v: [] for v in models}, {}
            for _ in range(REPEATS):
                for v, m in models.items():
                    def step(i):
                        k = i % N_BATCHES
                        b = batches[k] if v == 'direct' else list(batches[k])
                        return train.train_step(m, b, targets[k], loss_func, opts[v], direct=v == 'direct')
                    for i in range(WARMUP):
                        step(i)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for i in range(a.steps):
                        loss = step(i)
                    torch.cuda.synchronize(dev)
                    ms[v].append((time.perf_counter() - t0) / a.steps * 1e3)
                    last[v] = f'last loss {float(loss):.9g}'
            _report(lines, f'  training step, {mode} encoder(s), ms/step ({WARMUP} warm-up + {a.steps} timed steps per '
                           f'repeat, variants alternated {REPEATS} times):', ms, last)
        if 'predict' in a.what:
            rows = list(zip(synthetic.make_batch('polymer', ROWS, 7000), synthetic.make_batch('qm9', ROWS, 7500)))
            data = make_batches(rows, BATCH, shared=shared)
            m = new_model().eval()
            ms, out = {'native': [], 'own_forward': []}, {}
            for r in range(REPEATS + 1):  # (the first pass of each is the warm-up: device graphs, plans, packs)
                for v in ms:
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    preds = torch.cat([p for _, p in device_predictions(m, data, own_forward=v == 'own_forward')])
                    torch.cuda.synchronize(dev)
                    if r:
                        ms[v].append((time.perf_counter() - t0) * 1e3)
                    out[v] = preds
            err = float((out['native'] - out['own_forward']).abs().max() / out['own_forward'].abs().max())
            _report(lines, f'  prediction of {ROWS} rows in batches of {BATCH}, {mode} encoder(s), ms/pass (one warm-up '
                           f'pass, then {REPEATS} alternated):', ms,
                    {v: f'max |native - own_forward| / max |own_forward| = {err:.2e}' for v in ms})
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
