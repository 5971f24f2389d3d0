"""Generate tests/golden/ensemble/ensemble_ref.npz from the REAL reference ``spectra_utils.roundrobin_sid`` and
``StandardScaler.inverse_transform``, with numpy's float64 ``sum / M`` and ``np.var`` (what
make_predictions.py:129-201 computes for an ensemble).

Run where the reference tree is available (tools/ref_loader.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_ensemble_golden.py

Keys (W in 3, 7; M in 1, 2, 5; five models, five rows per block):

* ``b1_w<W>`` fp32 [5][5][W]: values near 1e4 with a spread of 1e-2 across the models: fp32 arithmetic and the
  sum-of-squares variance both fail on them (the printed errors);
* ``b2_w<W>`` fp32 [5][5][W]: values of order 1, one NaN cell in model 1; ``scale_mean_w<W>`` / ``scale_std_w<W>``
  float64 [W] and ``b2_w<W>_inv`` float64 [5][5][W]: the reference scaler's ``inverse_transform`` of each model's
  block (NaN where it returns None);
* ``<block>_mean_m<M>`` / ``<block>_var_m<M>`` float64 [5][W]: ``sum / M`` and ``np.var`` over the first M models
  (of ``b1`` as it is, of ``b2`` after the inverse transform);
* ``sid_<N>_<T>_<M>`` fp32 [M][N][T] spectra (row 1: the last 9 positions NaN in every model; a few values below
  1e-3) and ``sid_<N>_<T>_<M>_out`` float64 [N]: ``roundrobin_sid`` of them; ``sid_3_33_3_thr_out``: with
  ``threshold=1e-3``.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from ref_loader import REF  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'ensemble')
MODELS, ROWS = 5, 5
SID_CASES = ((3, 33, 2), (3, 33, 3), (2, 300, 5), (2, 33, 1))
THRESHOLD = 1e-3


def load_by_path(name, relpath):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    su = load_by_path('ref_spectra_utils', 'chemprop/spectra_utils.py')
    scaler_mod = load_by_path('ref_scaler', 'chemprop/data/scaler.py')
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20)
    out = {}
    for W in (3, 7):
        centre = 1e4 * (1 + 0.1 * rng.random((1, ROWS, W)))
        b1 = (centre + 1e-2 * rng.standard_normal((MODELS, ROWS, W))).astype(np.float32)
        b2 = rng.standard_normal((MODELS, ROWS, W)).astype(np.float32)
        b2[1, 3, W - 2] = np.nan
        means, stds = 50 * rng.standard_normal(W), 0.5 + 3 * rng.random(W)
        sc = scaler_mod.StandardScaler(means, stds)
        inv = np.array([[[np.nan if x is None else x for x in r] for r in np.asarray(sc.inverse_transform(b2[k]))]
                        for k in range(MODELS)], dtype=np.float64)
        out[f'b1_w{W}'], out[f'b2_w{W}'], out[f'b2_w{W}_inv'] = b1, b2, inv
        out[f'scale_mean_w{W}'], out[f'scale_std_w{W}'] = means, stds
        for name, v in ((f'b1_w{W}', b1.astype(np.float64)), (f'b2_w{W}', inv)):
            for M in (1, 2, 5):
                out[f'{name}_mean_m{M}'] = np.sum(v[:M], axis=0) / M
                out[f'{name}_var_m{M}'] = np.var(v[:M], axis=0)
        # what the block separates: Welford in fp64 against sum of squares in fp64 and Welford in fp32
        v, exact = b1.astype(np.float64), np.var(b1.astype(np.longdouble), axis=0).astype(np.float64)
        sq = np.sum(v * v, axis=0) / MODELS - (np.sum(v, axis=0) / MODELS) ** 2
        m32, s32 = b1[0].copy(), np.zeros_like(b1[0])
        for k in range(1, MODELS):
            d = b1[k] - m32
            m32 = m32 + d / np.float32(k + 1)
            s32 = s32 + d * (b1[k] - m32)
        rel = (lambda a: float(np.abs(a - exact).max() / exact.max()))
        print(f'W={W}: variance error np.var {rel(np.var(v, axis=0)):.1e}  sum of squares {rel(sq):.1e}  '
              f'fp32 Welford {rel(s32.astype(np.float64) / MODELS):.1e}')
    for N, T, M in SID_CASES:
        base = rng.gamma(2.0, size=(1, N, T))
        s = base * (1 + 0.3 * rng.random((M, N, T)))
        s = s / s.sum(axis=2, keepdims=True)
        s[:, :, 5] = 10.0 ** (-6 + 2.9 * rng.random((M, N)))  # below the threshold, and far apart
        s[:, 1, T - 9:] = np.nan
        s = s.astype(np.float32)
        key = f'sid_{N}_{T}_{M}'
        out[key] = s
        block = np.ascontiguousarray(np.transpose(s.astype(np.float64), (1, 2, 0)))  # (N, T, M), as the reference takes it
        with np.errstate(invalid='ignore'):
            out[f'{key}_out'] = np.array(su.roundrobin_sid(block.copy()), dtype=np.float64)
            if (N, T, M) == (3, 33, 3):
                out[f'{key}_thr_out'] = np.array(su.roundrobin_sid(block.copy(), threshold=THRESHOLD), dtype=np.float64)
                assert not np.allclose(out[f'{key}_thr_out'], out[f'{key}_out'], rtol=1e-3)
        print(key, out[f'{key}_out'])
    path = os.path.join(OUT, 'ensemble_ref.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
