"""Time one epoch's scoring (the training split plus the validation split), two ways.

    python tools/eval_epoch.py [--repeats 7] [--batch_size 50] [--out FILE]

Three shapes, hidden 300, depth 3, a two-layer FFN, synthetic polymer graphs:

* ``regression``: 2048 + 256 rows, one task, metrics rmse, mae, r2;
* ``spectra``: 512 + 64 rows, T = 1801 positions, metrics sid, wasserstein;
* ``frozen``: the regression shape with a frozen encoder, scored from cached encodings (the head alone).

* ``A``: ``evaluate.evaluate`` -- the splits' ``BatchMolGraph`` s and ``TargetTable`` s are built once (outside the
  timed window, as ``chemprop_train --device_metrics`` builds them once per run); per split the batches in groups of
  eight through ``forward_many``, the native head, one ``wdmpnn_eval_add`` / ``wdmpnn_eval_spectra`` launch per
  batch, one small copy to the host;
* ``B``: what ``chemprop_train`` does without the flag: ``cli.predict`` (one forward per batch, a synchronous
  ``.cpu().numpy().tolist()`` after each) and ``cli.evaluate_predictions`` (sklearn per task and metric).

One warm-up run of each, then the two alternated ``--repeats`` times in ONE process; every run ends with a
synchronise.  Reports each repeat, the medians and the spread (max - min) of each path, and the largest relative
difference between the two paths' scores.  Two medians differ only when they are further apart than the larger
spread."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'polymer-chemprop_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from chemprop_amd import TargetTable, TrainArgs, cli, evaluate, synthetic  # noqa: E402
from chemprop_amd.ensemble import make_batches  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402
from chemprop_amd.train import frozen_encodings  # noqa: E402

SHAPES = {'regression': dict(kind='regression', rows=(2048, 256), tasks=1, metrics=['rmse', 'mae', 'r2'], frozen=False),
          'spectra': dict(kind='spectra', rows=(512, 64), tasks=1801, metrics=['sid', 'wasserstein'], frozen=False),
          'frozen': dict(kind='regression', rows=(2048, 256), tasks=1, metrics=['rmse', 'mae', 'r2'], frozen=True)}


def measure(name, shape, a, dev):
    kind, metrics, tasks = shape['kind'], shape['metrics'], shape['tasks']
    rng = np.random.default_rng(1)
    torch.manual_seed(0)
    model = MoleculeModel(TrainArgs(hidden_size=300, depth=3, dataset_type=kind, num_tasks=tasks, device=dev))
    initialize_weights(model)
    if shape['frozen']:
        cli.apply_freezing(model, frzn_encoder=True)
    model = model.to(dev).eval()
    scaler = cli.StandardScaler(rng.normal(size=tasks) * 10, 1 + rng.random(tasks)) if kind == 'regression' else None
    splits = []
    for s, n in enumerate(shape['rows']):
        graphs = []
        for i in range((n + 63) // 64):
            graphs += synthetic.make_batch('polymer', 64, 9000 + 100 * s + i)
        graphs = graphs[:n]
        if kind == 'spectra':
            t = np.exp(rng.standard_normal((n, tasks)))
            t = t / t.sum(axis=1, keepdims=True)
        else:
            t = rng.standard_normal((n, tasks)) * 10
        splits.append(dict(graphs=graphs, idx=list(range(n)), rows=t.tolist(), table=TargetTable(t, kind, dev),
                           batches=make_batches(graphs, a.batch_size),
                           enc=frozen_encodings(model, graphs, a.batch_size) if shape['frozen'] else None))

    def path_a():
        return [evaluate(model, a.batch_size if s['enc'] is not None else s['batches'], s['table'], metrics, scaler,
                         encodings=s['enc']) for s in splits]

    def path_b():
        return [cli.evaluate_predictions(cli.predict(model, s['graphs'], s['idx'], a.batch_size, scaler, s['enc']),
                                         s['rows'], tasks, metrics, kind) for s in splits]

    paths = {'A': path_a, 'B': path_b}
    res = {k: f() for k, f in paths.items()}  # warm-up (first-use costs, caches, allocator)
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in paths}
    for _ in range(a.repeats):
        for k, f in paths.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res[k] = f()
            torch.cuda.synchronize(dev)
            ms[k].append((time.perf_counter() - t0) * 1e3)
    diff = max(abs(x - y) / max(abs(y), 1e-300) for ra, rb in zip(res['A'], res['B']) for m in metrics
               for x, y in zip(ra[m], rb[m]))
    rows = ' + '.join(str(n) for n in shape['rows'])
    lines = [f'{name}: {kind}, {rows} rows (training + validation split), {tasks} output(s), batch size {a.batch_size}, '
             f'metrics {", ".join(metrics)}' + (', frozen encoder: cached encodings, the head alone' if shape['frozen']
                                                else '')]
    for k, v in ms.items():
        lines.append(f'    {k} ms/epoch scoring: ' + ' '.join(f'{x:.2f}' for x in v) +
                     f'   median {statistics.median(v):.2f}   spread {max(v) - min(v):.2f}')
    ma, mb = statistics.median(ms['A']), statistics.median(ms['B'])
    spread = max(max(v) - min(v) for v in ms.values())
    verdict = 'A is faster' if mb - ma > spread else 'B is faster' if ma - mb > spread else 'no difference shown'
    lines.append(f'    medians {abs(mb - ma):.2f} ms apart, larger spread {spread:.2f}: {verdict}'
                 f' ({mb / ma:.1f}x)   A vs B scores: max relative difference {diff:.2e}')
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--batch_size', type=int, default=50)
    ap.add_argument('--shapes', nargs='+', default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = [f'one epoch\'s scoring, hidden 300, depth 3, 2-layer FFN, synthetic polymer graphs; one warm-up run of each '
             f'path, then A and B alternated {a.repeats} times in one process',
             f'device: {torch.cuda.get_device_name(dev)}',
             '    A = evaluate.evaluate (resident targets, device partial sums), B = cli.predict + '
             'cli.evaluate_predictions (host copy per batch, sklearn)']
    for name in a.shapes:
        lines += measure(name, SHAPES[name], a, dev)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
