"""Wall time of ``fingerprint.molecule_fingerprint`` against the per-batch route it replaces (MI355X only).

    python tools/fingerprint_bench.py [--models 5] [--graphs 2048] [--hidden 300] [--batch_size 50] [--repeats 7]

Both routes produce the float64 ``[N][fp][M]`` array of the reference's ``molecule_fingerprint`` for M models and N
synthetic polymer graphs, batches built inside the timed window (once per call, as both need them):

* ``native``    ``molecule_fingerprint``: the encoder eight batches at a time, ``head_latent`` for ``last_FFN``, one
                ``wdmpnn_latent_add`` launch per batch, one host copy after the last model;
* ``per_batch`` what a caller had before: ``MoleculeModel.fingerprint`` as molecule_fingerprint.py:167-181 runs it, one
                forward per batch (for ``last_FFN`` the torch slice ``ffn[:-1]``), ``.cpu().tolist()`` every batch,
                the numpy array filled model by model.

Each timing is a host clock around a call that ends with the data on the host (so the device has finished).  One
warm-up call per route and type, then ``--repeats`` timed calls with the two routes alternating; median, minimum and
maximum are printed, one JSON line per fingerprint type, and the two results are compared (normwise).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'polymer-chemprop_amd'))

from chemprop_amd import MoleculeModel, TrainArgs, synthetic  # noqa: E402
from chemprop_amd.ensemble import make_batches  # noqa: E402
from chemprop_amd.fingerprint import fingerprint_width, molecule_fingerprint  # noqa: E402


def per_batch(models, graphs, batch_size, fingerprint_type):
    batches = make_batches(graphs, batch_size)
    out = np.zeros((len(graphs), fingerprint_width(models[0], fingerprint_type), len(models)))
    for index, model in enumerate(models):
        model.eval()
        fingerprints = []
        for batch in batches:
            with torch.no_grad():
                enc = model.encoder([batch])
                fp = enc if fingerprint_type == 'MPN' else model.ffn[:-1](enc)
            fingerprints.extend(fp.data.cpu().tolist())
        out[:, :, index] = fingerprints
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', type=int, default=5)
    ap.add_argument('--graphs', type=int, default=2048)
    ap.add_argument('--hidden', type=int, default=300)
    ap.add_argument('--batch_size', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fingerprint_bench needs the GPU: there is no CPU path to time')
    dev = torch.device('cuda', 0)
    graphs = synthetic.make_batch('polymer', a.graphs, 2024)
    models = []
    for k in range(a.models):
        m = MoleculeModel(TrainArgs(hidden_size=a.hidden, depth=3, num_tasks=1, device=dev))
        synthetic.fill_parameters(m, 300 + k)
        models.append(m.to(dev).eval())
    routes = {'native': lambda t: molecule_fingerprint(models, graphs, a.batch_size, t, device=dev),
              'per_batch': lambda t: per_batch(models, graphs, a.batch_size, t)}
    for t in ('MPN', 'last_FFN'):
        results = {name: fn(t) for name, fn in routes.items()}  # (the warm-up calls)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(t)
                times[name].append(time.perf_counter() - t0)
        ref = results['per_batch']
        err = float(np.abs(results['native'] - ref).max() / max(np.abs(ref).max(), 1e-30))
        line = {'fingerprint_type': t, 'models': a.models, 'graphs': a.graphs, 'hidden': a.hidden,
                'batch_size': a.batch_size, 'repeats': a.repeats, 'shape': list(ref.shape),
                'normwise_native_vs_per_batch': err}
        for name, ts in times.items():
            line[name] = {'median_s': float(np.median(ts)), 'min_s': float(min(ts)), 'max_s': float(max(ts))}
        line['per_batch_over_native'] = line['per_batch']['median_s'] / line['native']['median_s']
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
