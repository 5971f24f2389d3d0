"""Time the prediction of an ensemble over a data set, two ways.

    python tools/ensemble_predict.py [--models 5] [--graphs 2048] [--batch_size 50] [--repeats 5] [--out FILE]

M regression models (hidden 300, depth 3, a two-layer FFN, each with its own weights and target scaler) over
synthetic polymer graphs:

* ``A``: ``ensemble.predict_ensemble`` -- the batches are packed once, every model runs them in groups of eight
  through ``forward_many``, the native head and one ``wdmpnn_ensemble_add`` launch per batch; mean and variance
  leave the device once, after the last model;
* ``B``: what the tree had before: ``cli.predict`` per model (one forward per batch, ``.cpu().numpy().tolist()``
  after each, the inverse scaling on the host), summed into numpy float64 arrays as make_predictions.py:129-201
  does, ``np.var`` over the kept predictions.

One warm-up run of each, then the two alternated ``--repeats`` times in ONE process; every run ends with a
synchronise.  Reports each repeat, the medians and the spread (max - min) of each path, and the largest difference
between the two paths' means and variances.  Two medians differ only when they are further apart than the larger
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

from chemprop_amd import TrainArgs, cli, synthetic  # noqa: E402
from chemprop_amd.ensemble import predict_ensemble  # noqa: E402
from chemprop_amd.model import MoleculeModel  # noqa: E402
from chemprop_amd.nn_utils import initialize_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--models', type=int, default=5)
    ap.add_argument('--graphs', type=int, default=2048)
    ap.add_argument('--batch_size', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None, help='also append the report to this file')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    graphs = []
    for i in range((a.graphs + 63) // 64):
        graphs += synthetic.make_batch('polymer', 64, 7000 + i)
    graphs = graphs[:a.graphs]
    rng = np.random.default_rng(0)
    members = []
    for k in range(a.models):
        torch.manual_seed(k)
        m = MoleculeModel(TrainArgs(hidden_size=300, depth=3, device=dev))
        initialize_weights(m)
        members.append((m.to(dev).eval(), cli.StandardScaler(rng.normal(size=1) * 10, 1 + rng.random(1)), None))
    idx = list(range(len(graphs)))

    def path_a():
        mean, var, _ = predict_ensemble(members, graphs, a.batch_size, variance=True, device=dev)
        return mean, var

    def path_b():
        total = np.zeros((len(graphs), 1))
        every = np.zeros((len(graphs), 1, len(members)))
        for k, (m, scaler, _) in enumerate(members):
            preds = np.array(cli.predict(m, graphs, idx, a.batch_size, scaler))
            total += preds
            every[:, :, k] = preds
        return total / len(members), np.var(every, axis=2)

    paths = {'A': path_a, 'B': path_b}
    res = {name: f() for name, f in paths.items()}  # warm-up (first-use costs, caches, allocator)
    torch.cuda.synchronize(dev)
    ms = {name: [] for name in paths}
    for _ in range(a.repeats):
        for name, f in paths.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res[name] = f()
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) * 1e3)
    scale = float(np.abs(res['B'][0]).max())
    lines = [f'ensemble prediction: {a.models} regression models (hidden 300, depth 3, 2-layer FFN) over {len(graphs)} '
             f'synthetic polymer graphs, batch size {a.batch_size}; one warm-up run of each path, then A and B '
             f'alternated {a.repeats} times in one process, mean and variance computed by both',
             f'device: {torch.cuda.get_device_name(dev)}',
             '    A = predict_ensemble (device accumulation), B = cli.predict per model + numpy float64 sum on the host']
    for name, v in ms.items():
        lines.append(f'    {name} ms/data set: ' + ' '.join(f'{x:.2f}' for x in v) +
                     f'   median {statistics.median(v):.2f}   spread {max(v) - min(v):.2f}')
    lines.append(f'    A vs B: max |mean difference| / max |mean| = {float(np.abs(res["A"][0] - res["B"][0]).max()) / scale:.2e}, '
                 f'max |variance difference| / max variance = '
                 f'{float(np.abs(res["A"][1] - res["B"][1]).max()) / float(res["B"][1].max()):.2e}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
