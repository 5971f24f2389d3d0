"""Time the training step of a spectra model three ways: the direct step, the fused head under autograd, and
``fused_head=False`` (the torch ops of the reference's step: ffn, exp, sid_loss, autograd).

    python tools/spectra_step.py [--out FILE] [--label NAME] [--loss sid|wasserstein]
    python tools/spectra_step.py --modes direct --steps 20 --repeats 1      # under rocprofv3 --kernel-trace --stats
    python tools/spectra_step.py --kernel-table DIR [--out FILE]           # the table of such a run's kernel stats

Polymer batches of 64, hidden 300, depth 3, a two-layer FFN with T = 1801 outputs (one per wavenumber bin), exp
output activation; targets normalised rows with a tenth of the entries missing.  Per repeat: 20 warm-up steps, then
100 timed steps ending in a synchronise; the modes alternate three times in ONE process (each keeps its own model
and optimizer, same seed).  Reports each repeat, the medians and the spread (max - min) between the repeats of
one mode: two medians differ only when they are further apart than the larger spread.

``--kernel-table DIR`` reads the ``*kernel_stats.csv`` rocprofv3 wrote under DIR (a traced run of its own: tracing
slows the host, so no step time is taken from it) and prints every kernel's calls, average time, and share of the
summed kernel time, with the spectra head's kernels (``head_*``) and their share of the step's kernel time."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'polymer-chemprop_amd')]

BATCH, T, WARMUP = 64, 1801, 20


def kernel_table(path: str) -> str:
    files = sorted(glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True))
    if not files:
        raise SystemExit(f'no *kernel_stats.csv under {path}')
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    head = [r for r in rows if r['Name'].startswith(('head_', 'wd::head_', 'void wd::head_'))]
    lines = [f'kernel stats of {os.path.relpath(files[0], path)}: {len(rows)} kernels, '
             f'{total / 1e6:.3f} ms of kernel time in all']
    for r in rows[:24]:
        lines.append(f"  {r['Name'][:72]:72s} calls={r['Calls']:>6s} avg={float(r['AverageNs']) / 1e3:9.2f} us  "
                     f"{100 * float(r['TotalDurationNs']) / total:5.1f} %")
    lines.append('the FFN head\'s kernels:')
    for r in head:
        lines.append(f"  {r['Name'][:72]:72s} calls={r['Calls']:>6s} avg={float(r['AverageNs']) / 1e3:9.2f} us  "
                     f"{100 * float(r['TotalDurationNs']) / total:5.1f} %")
    lines.append(f'head share of the kernel time: {100 * sum(float(r["TotalDurationNs"]) for r in head) / total:.1f} %')
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--label', default='', help='a name for this run in the report (the tree it measures)')
    ap.add_argument('--loss', default='sid', choices=['sid', 'wasserstein'])
    ap.add_argument('--modes', nargs='+', default=['direct', 'autograd', 'torch'], choices=['direct', 'autograd', 'torch'])
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kernel-table', default=None, metavar='DIR')
    a = ap.parse_args()
    if a.kernel_table:
        text = kernel_table(a.kernel_table)
    else:
        text = measure(a)
    print(text, end='')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


def measure(a) -> str:
    import numpy as np
    import torch

    from chemprop_amd import TrainArgs, spectra_utils, synthetic
    from chemprop_amd.featurization import BatchMolGraph, get_bond_fdim
    from chemprop_amd.model import MoleculeModel
    from chemprop_amd.nn_utils import initialize_weights
    from chemprop_amd.train import _StackHead, _fusable_head, build_optimizer, get_loss_func, train_step

    dev = torch.device('cuda:0')
    loss_func = get_loss_func('spectra', None if a.loss == 'sid' else a.loss)
    batches = []
    for i in range(4):
        g = BatchMolGraph(synthetic.make_batch('polymer', BATCH, 7000 + i), device_bond_features=True)
        g.device_graph(dev, False, get_bond_fdim())
        rng = np.random.default_rng(i)
        raw = rng.gamma(2.0, size=(BATCH, T)) + 0.01
        raw[rng.random((BATCH, T)) < 0.1] = np.nan
        # (a float array with NaN = missing, as the command line hands its spectra batches to train_step)
        batches.append(([g], np.array(spectra_utils.normalize_spectra(raw, threshold=1e-8, excluded_sub_value=np.nan),
                                      dtype=np.float64)))
    lines = [f'spectra training step{" [" + a.label + "]" if a.label else ""}: polymer B = {BATCH}, hidden 300, depth 3, '
             f'two-layer FFN, T = {T}, exp, {a.loss} loss; {WARMUP} warm-up + {a.steps} timed steps per repeat, modes '
             f'alternated {a.repeats} times in one process', f'device: {torch.cuda.get_device_name(dev)}']
    args = TrainArgs(hidden_size=300, depth=3, device=dev, dataset_type='spectra')
    args.num_tasks = T
    modes = {}
    for name in a.modes:
        torch.manual_seed(0)
        m = MoleculeModel(args)
        initialize_weights(m)
        m = m.to(dev).train()
        kw = dict(dataset_type='spectra', direct=name == 'direct', fused_head=name != 'torch')
        modes[name] = (m, build_optimizer(m, 1e-4), kw)
    head = _fusable_head(next(iter(modes.values()))[0], loss_func, 'spectra')
    if not (isinstance(head, _StackHead) and head.spectra is not None):
        raise SystemExit('the spectra head does not take this model')  # (no fall-back to measure)
    ms = {name: [] for name in modes}
    last = {}
    for _ in range(a.repeats):
        for name, (m, opt, kw) in modes.items():
            for i in range(WARMUP):
                train_step(m, *batches[i % 4], loss_func, opt, **kw)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(a.steps):
                loss = train_step(m, *batches[i % 4], loss_func, opt, **kw)
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            last[name] = float(loss)
    for n in ms:
        lines.append(f'    {n:8s} ms/step: ' + ' '.join(f'{v:.4f}' for v in ms[n]) +
                     f'   median {statistics.median(ms[n]):.4f}   spread {max(ms[n]) - min(ms[n]):.4f}   '
                     f'last loss {last[n]:.6f}')
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    main()
