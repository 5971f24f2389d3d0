"""The native spectra head (``wdmpnn_head_spectra`` / ``wdmpnn_head_spectra_predict``): FFNs with up to 8192
outputs, the exp / softplus output activation, the SID and Wasserstein row losses on the masked, row-normalised
output, and their wiring through ``chemprop_amd.train``, ``MoleculeModel`` and ``spectra_utils``.

CPU: header, binding and library agree on the new symbols and struct layouts (ABI still 12); refusals launch
nothing; the scratch size; structure recognition; the torch losses, ``normalize_spectra`` and the metrics against
the fixture made from the reference's own code (tools/make_spectra_golden.py); the host target check.
GPU: loss, output and every gradient against fp64 torch ops with explicit dropout masks; logits of +-100; a
present target with weight 0; bitwise repeatability and partial calls; the prediction head; training steps on
every path; a frozen encoder; the reference fixture."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import TrainArgs, _native, spectra_utils, synthetic
from chemprop_amd.featurization import BatchMolGraph
from chemprop_amd.model import MoleculeModel
from chemprop_amd.nn_utils import dropout_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')
TOL = 1e-5
DEV = torch.device('cuda:0')
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -1000, -1001, -1002, -1003
FIXTURE = 'spectra/model_polymer_spectra'
ACT = {'ReLU': 0, 'PReLU': 2}
S_ACT = {'exp': 0, 'softplus': 1}
LOSS = {'sid': 0, 'wasserstein': 1}


# ---------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_spectra_head(tmp_path):
    """The three new entry points are declared, bound and exported, the ABI version is still 12, and
    WdHeadSpectra / WdHeadSpectraPredict have the layout a C compiler gives the header."""
    text = open(HEADER).read()
    assert '#define WDMPNN_ABI_VERSION 12' in text and '#define WD_HEAD_MAX_SPECTRUM 8192' in text
    assert _native.ABI_VERSION == 12 and _native.HEAD_MAX_SPECTRUM == 8192
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for fn in ('wdmpnn_head_spectra', 'wdmpnn_head_spectra_predict', 'wdmpnn_head_spectra_scratch_bytes'):
        assert re.search(r'\bint\s+%s\s*\(' % fn, text), fn
        assert fn in _native.EXPORTED_SYMBOLS
        assert re.search(r'\bT %s\b' % fn, out), fn
    declared = sorted(set(re.findall(r'\b(wdmpnn_\w+)\s*\(', text)))  # (test_native_abi.declared_functions)
    assert declared == sorted(_native.EXPORTED_SYMBOLS)
    L = _native.lib()
    assert L.wdmpnn_abi_version() == 12
    assert L.wdmpnn_head_spectra.argtypes[0]._type_ is _native.WdHeadSpectra
    assert L.wdmpnn_head_spectra_predict.argtypes[0]._type_ is _native.WdHeadSpectraPredict
    S, P = _native.WdHeadSpectra, _native.WdHeadSpectraPredict
    sf = [n for n, _ in S._fields_]
    pf = [n for n, _ in P._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wdmpnn.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(WdHeadSpectra), sizeof(WdHeadSpectraPredict));\n' +
                   ''.join(f'  printf(" %zu", offsetof(WdHeadSpectra, {n}));\n' for n in sf) +
                   ''.join(f'  printf(" %zu", offsetof(WdHeadSpectraPredict, {n}));\n' for n in pf) +
                   '  printf("\\n"); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC', 'gcc'), '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert c == [ctypes.sizeof(S), ctypes.sizeof(P)] + [getattr(S, n).offset for n in sf] + \
        [getattr(P, n).offset for n in pf]


def _fake(L=3, T=65, s_act=0, kind=0, p=0.25, ld_table=None, B=4, scratch=4096, F=32, Hf=16, null_w=None, loss=4096):
    """A WdHeadSpectra of made-up addresses (never dereferenced: every call below is refused on the host)."""
    a = 4096
    h = _native.WdHeadSpectra()
    h.x, h.ld_x, h.B, h.F, h.Hf, h.T, h.L = a, F, B, F, Hf, T, L
    for i in range(min(max(L, 0), _native.HEAD_MAX_LAYERS)):
        h.W[i], h.b[i], h.dW[i], h.db[i] = a, a, a, a
    if null_w is not None:
        h.W[null_w] = 0
    h.slope, h.table, h.ld_table, h.inv_n, h.act = a, a, 2 * T if ld_table is None else ld_table, 1.0, 2
    h.p, h.seed, h.spectra_act, h.loss_kind = p, 7, s_act, kind
    h.scratch, h.scratch_bytes = scratch, 1 << 30
    h.dx, h.dslope, h.loss = a, a, loss
    return h


@pytest.mark.parametrize('kw,rc', [(dict(T=0), ERR_SHAPE),
                                   (dict(T=8193), ERR_UNSUPPORTED),
                                   (dict(L=0), ERR_SHAPE),
                                   (dict(L=7), ERR_UNSUPPORTED),
                                   (dict(s_act=2), ERR_UNSUPPORTED),
                                   (dict(kind=2), ERR_UNSUPPORTED),
                                   (dict(ld_table=2 * 65 - 1), ERR_SHAPE),
                                   (dict(p=1.0), ERR_ARG),
                                   (dict(null_w=1), ERR_ARG),
                                   (dict(loss=0), ERR_ARG),
                                   (dict(scratch=0), ERR_ARG)])
def test_spectra_head_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    h = _fake(**kw)
    got = L.wdmpnn_head_spectra(ctypes.byref(h), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()
    with pytest.raises((ValueError, NotImplementedError, _native.NativeError)):
        _native.check(got, 'head spectra')


def test_spectra_head_refuses_a_small_scratch_and_sizes_it():
    L = _native.lib()
    B, F, Hf, T, n = 5, 40, 37, 65, 3
    tiles = ((B + 15) // 16) * ((Hf + 15) // 16)
    # the stack head's regions (z, dz, dslope partial sums, its a_{L-1} slot, dout, the rows' losses), then z_L
    want = 4 * ((n - 1) * (2 * B * Hf + max(B, tiles)) + B * Hf + B * T + B + B * T)
    assert _native.head_spectra_scratch_bytes(B, F, Hf, T, n) == want
    assert _native.head_spectra_scratch_bytes(B, F, 0, T, 1) == 4 * (B * F + B * T + B + B * T)
    assert _native.head_spectra_scratch_bytes(B, F, Hf, T, n) == _native.head_stack_scratch_bytes(B, F, Hf, T, n) + \
        4 * B * T
    h = _fake(L=n, B=B, F=F, Hf=Hf, T=T)
    h.scratch_bytes = want - 4
    assert L.wdmpnn_head_spectra(ctypes.byref(h), None) == ERR_WORKSPACE
    assert 'scratch' in L.wdmpnn_last_error().decode()


def test_spectra_entries_without_rows_are_no_ops():
    L = _native.lib()
    assert L.wdmpnn_head_spectra(ctypes.byref(_fake(B=0)), None) == 0
    q = _native.WdHeadSpectraPredict()
    q.ld_x, q.B, q.F, q.Hf, q.T, q.L, q.act, q.spectra_act, q.normalize = 32, 0, 32, 16, 1801, 2, 2, 1, 1
    q.W[0], q.W[1], q.slope = 4096, 4096, 4096
    assert L.wdmpnn_head_spectra_predict(ctypes.byref(q), None) == 0
    q.T = 8193
    assert L.wdmpnn_head_spectra_predict(ctypes.byref(q), None) == ERR_UNSUPPORTED
    q.T, q.spectra_act = 1801, 2
    assert L.wdmpnn_head_spectra_predict(ctypes.byref(q), None) == ERR_UNSUPPORTED
    q.spectra_act, q.normalize = 0, 2
    assert L.wdmpnn_head_spectra_predict(ctypes.byref(q), None) == ERR_UNSUPPORTED
    # the other heads keep their limits and kinds
    s = _native.WdHeadStack()
    s.x, s.ld_x, s.B, s.F, s.Hf, s.T, s.L = 4096, 32, 4, 32, 16, 65, 2
    s.W[0], s.W[1], s.dW[0], s.dW[1] = 4096, 4096, 4096, 4096
    s.table, s.ld_table, s.inv_n, s.n_classes, s.scratch, s.scratch_bytes = 4096, 130, 1.0, 1, 4096, 1 << 30
    s.dx, s.loss = 4096, 4096
    assert L.wdmpnn_head_stack(ctypes.byref(s), None) == ERR_UNSUPPORTED
    s.T, s.ld_table, s.loss_kind = 6, 12, 3
    assert L.wdmpnn_head_stack(ctypes.byref(s), None) == ERR_UNSUPPORTED


def _cpu_model(layers=2, s_act='exp', tasks=1801, dataset='spectra', dropout=0.0, act='ReLU'):
    args = TrainArgs(hidden_size=32, depth=3, activation=act, ffn_hidden_size=24, ffn_num_layers=layers,
                     dropout=dropout, device=torch.device('cpu'), dataset_type=dataset, spectra_activation=s_act)
    args.num_tasks = tasks
    return MoleculeModel(args)


def test_spectra_ffn_structure_recognition():
    from chemprop_amd.train import _StackHead, _ffn_structure, _fusable_head, get_loss_func
    for layers in (1, 2, 3):
        for s_act in ('exp', 'softplus'):
            m = _cpu_model(layers, s_act, dropout=0.1)
            assert m.spectra and len(m.ffn) == 3 * layers
            st = _ffn_structure(m.ffn, True, spectra=True)
            assert isinstance(st, _StackHead) and st.spectra == S_ACT[s_act] and len(st.linears) == layers
            assert st.linears[-1].out_features == 1801 and st.p == pytest.approx(0.1)
            assert st.linears == [l for l in m.ffn if isinstance(l, torch.nn.Linear)]
            assert _ffn_structure(m.ffn, True) is None  # a trailing activation is a spectra FFN's only
            assert _fusable_head(m, get_loss_func('spectra'), 'spectra') is None  # (CPU parameters)
    assert _ffn_structure(_cpu_model(2, tasks=8192).ffn, True, spectra=True) is not None
    assert _ffn_structure(_cpu_model(2, tasks=8193).ffn, True, spectra=True) is None
    assert _ffn_structure(_cpu_model(7).ffn, True, spectra=True) is None
    m = _cpu_model(2)
    m.ffn[-1] = torch.nn.Softplus(beta=2.0)
    assert _ffn_structure(m.ffn, True, spectra=True) is None
    m.ffn[-1] = torch.nn.Sigmoid()
    assert _ffn_structure(m.ffn, True, spectra=True) is None
    # without a trailing activation it is not a spectra FFN; the other kinds keep their 64 outputs
    reg = _cpu_model(2, dataset='regression', tasks=3)
    assert _ffn_structure(reg.ffn, True, spectra=True) is None and _ffn_structure(reg.ffn, True).spectra is None
    assert _ffn_structure(_cpu_model(3, dataset='regression', tasks=65).ffn, True) is None
    assert _ffn_structure(_cpu_model(3, dataset='regression', tasks=64).ffn, True) is not None


def test_get_loss_func_for_spectra():
    from chemprop_amd.train import get_loss_func
    assert get_loss_func('spectra') is spectra_utils.sid_loss
    assert get_loss_func('spectra', 'wasserstein') is spectra_utils.wasserstein_loss
    assert type(get_loss_func('regression')) is torch.nn.MSELoss
    with pytest.raises(ValueError):
        get_loss_func('regression', 'wasserstein')
    with pytest.raises(ValueError):
        get_loss_func('spectra', 'mse')


def _fixture():
    return np.load(os.path.join(golden_io.GOLDEN_DIR, FIXTURE + '.npz'), allow_pickle=False)


def _fixture_targets(z):
    return [[None if np.isnan(v) else float(v) for v in row] for row in z['targets']]


def test_torch_losses_normalisation_and_metrics_reproduce_the_reference_fixture():
    """spectra_utils on the CPU against what the reference's own spectra_utils gave for the same numbers."""
    z = _fixture()
    y = z['output']
    present = ~np.isnan(z['targets'])
    assert 0 < (~present).sum() < present.size
    tgt = torch.from_numpy(np.where(present, z['targets'], 0.0)).float()
    mask = torch.from_numpy(present)
    w = torch.Tensor(z['target_weights']) * torch.Tensor(z['data_weights']).unsqueeze(1) * mask
    for name, fn in (('sid', spectra_utils.sid_loss), ('wasserstein', spectra_utils.wasserstein_loss)):
        per = fn(torch.from_numpy(y), tgt, mask) * w
        assert golden_io.normwise(per.sum(dim=1).numpy(), z[f'{name}/lossrow']) <= TOL
        assert golden_io.normwise(float(per.sum() / mask.sum()), float(z[f'{name}/train_loss'])) <= TOL
    norm = np.array(spectra_utils.normalize_spectra(y.tolist(), z['phase_features'], z['phase_mask'],
                                                    excluded_sub_value=float('nan')), np.float64)
    assert np.array_equal(np.isnan(norm), np.isnan(z['normalized'])) and np.isnan(norm).any()
    assert golden_io.normwise(np.nan_to_num(norm), np.nan_to_num(z['normalized'])) <= 1e-12
    assert np.allclose(np.nansum(norm, axis=1), 1.0, atol=1e-12)
    assert np.array_equal(spectra_utils.phase_row_mask(z['phase_features'], z['phase_mask']), ~np.isnan(norm))
    targets = _fixture_targets(z)
    assert spectra_utils.sid_metric(y.tolist(), targets) == pytest.approx(float(z['sid_metric']), rel=1e-12)
    assert spectra_utils.wasserstein_metric(y.tolist(), targets) == \
        pytest.approx(float(z['wasserstein_metric']), rel=1e-12)
    # excluded_sub_value None, a threshold, and missing inputs
    rows = spectra_utils.normalize_spectra([[1.0, None, 3.0], [0.0, 2.0, 2.0]], threshold=0.5)
    assert rows == [[0.25, None, 0.75], [0.5 / 4.5, 2 / 4.5, 2 / 4.5]]


def test_metrics_average_over_all_rows_not_the_last_batch():
    """120 rows (more than the reference's batch of 50): the mean over all of them, by hand."""
    rng = np.random.default_rng(3)
    p = rng.random((120, 7)) + 0.1
    y = rng.random((120, 7)) + 0.1
    y /= y.sum(axis=1, keepdims=True)
    q = p / p.sum(axis=1, keepdims=True)
    sid = np.mean((q * np.log(q / y) + y * np.log(y / q)).sum(axis=1))
    assert spectra_utils.sid_metric(p.tolist(), y.tolist()) == pytest.approx(sid, rel=1e-12)
    was = np.mean(np.abs(np.cumsum(y, axis=1) - np.cumsum(q, axis=1)).sum(axis=1))
    assert spectra_utils.wasserstein_metric(p.tolist(), y.tolist()) == pytest.approx(was, rel=1e-12)
    last = np.mean((q[100:] * np.log(q[100:] / y[100:]) + y[100:] * np.log(y[100:] / q[100:])).sum(axis=1))
    assert abs(last - sid) > 1e-6  # (what the reference's last-batch mean would have given)


@pytest.mark.parametrize('bad', [0.0, -0.25, float('nan'), float('inf')])
def test_host_check_names_the_row_and_column_of_a_bad_spectra_target(bad):
    from chemprop_amd.train import _loss_table, check_spectra_targets
    rows = [[0.25, 0.75, None], [None, 0.5, 0.5], [0.5, None, 0.5]]
    check_spectra_targets(rows)
    rows[2][2] = bad
    with pytest.raises(ValueError, match=r'row 2, column 2'):
        check_spectra_targets(rows)
    with pytest.raises(ValueError, match=r'row 2, column 2'):
        _loss_table(rows, None, None, torch.device('cpu'), spectra=True)
    rows[2][2] = 0.5
    table, n_t, n_mask = _loss_table(rows, None, [1.0, 0.0, 2.0], torch.device('cpu'), spectra=True)
    assert n_t == 3 and n_mask == 6
    # 0 = missing in the target half; a present target with data weight 0 stays present
    assert table.tolist() == [[0.25, 0.75, 0.0, 1.0, 1.0, 0.0], [0.0, 0.5, 0.5, 0.0, 0.0, 0.0],
                              [0.5, 0.0, 0.5, 2.0, 0.0, 2.0]]


# ---------------------------------------------------------------------------------------------------
# GPU: the entry point itself
# ---------------------------------------------------------------------------------------------------
def _call(x, Ws, bs, slope, act, p, seed, s_act, kind, table, inv_n, want=None, want_out=True):
    """One wdmpnn_head_spectra call on device tensors (numpy results).  ``want``: the gradients asked for (None:
    all of them); the others get a NULL pointer."""
    B, F = x.shape
    n, T = len(Ws), Ws[-1].shape[0]
    Hf = Ws[0].shape[0] if n > 1 else 0
    nbytes = _native.head_spectra_scratch_bytes(B, F, Hf, T, n)
    # NaN-filled: the entry point must write everything it reads
    scratch = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device=DEV)
    new = lambda t: torch.full_like(t, float('nan'))  # noqa: E731
    names = ['dx', 'dslope'] + [f'dW{i + 1}' for i in range(n)] + [f'db{i + 1}' for i in range(n) if bs[i] is not None]
    want = set(names) if want is None else set(want)
    assert want <= set(names)
    bufs = {'dx': new(x), 'dslope': torch.full((1,), float('nan'), dtype=torch.float32, device=DEV)}
    for i in range(n):
        bufs[f'dW{i + 1}'] = new(Ws[i])
        if bs[i] is not None:
            bufs[f'db{i + 1}'] = new(bs[i])
    out = torch.full((B, T), float('nan'), dtype=torch.float32, device=DEV)
    loss = torch.full((), float('nan'), dtype=torch.float32, device=DEV)
    h = _native.WdHeadSpectra()
    h.x, h.ld_x, h.B, h.F, h.Hf, h.T, h.L = x.data_ptr(), F, B, F, Hf, T, n
    ptr = lambda k: bufs[k].data_ptr() if k in want else 0  # noqa: E731
    for i in range(n):
        h.W[i], h.b[i], h.dW[i] = Ws[i].data_ptr(), _native.ptr(bs[i]), ptr(f'dW{i + 1}')
        h.db[i] = ptr(f'db{i + 1}') if bs[i] is not None else 0
    h.slope, h.table, h.ld_table, h.inv_n, h.act = _native.ptr(slope), table.data_ptr(), table.shape[1], inv_n, act
    h.p, h.seed, h.spectra_act, h.loss_kind = p, seed, s_act, kind
    h.scratch, h.scratch_bytes = scratch.data_ptr(), nbytes
    h.out, h.dx, h.dslope, h.loss = out.data_ptr() if want_out else 0, ptr('dx'), ptr('dslope'), loss.data_ptr()
    _native.check(_native.lib().wdmpnn_head_spectra(ctypes.byref(h), _native.current_stream(DEV)), 'head spectra')
    torch.cuda.synchronize()
    res = {'loss': loss.cpu().numpy()}
    if want_out:
        res['out'] = out.cpu().numpy()
    for k in want:
        res[k] = bufs[k].cpu().numpy()
    return res


def _reference(x, Ws, bs, slope, act, p, seed, s_act, kind, table, inv_n, mask_from_w=False):
    """The same head in fp64 torch ops on the CPU with explicit masks from dropout_mask.  exp: p and log p as the
    max-subtracted softmax over the present positions (log_softmax); rows without a present target contribute
    nothing."""
    B = x.shape[0]
    f64 = lambda t: None if t is None else t.detach().cpu().double().requires_grad_(True)  # noqa: E731
    x, Ws, bs, slope = f64(x), [f64(W) for W in Ws], [f64(b) for b in bs], f64(slope)
    table = table.cpu().double()

    def drop(v, site):
        return v * torch.from_numpy(dropout_mask(seed, site, B, v.shape[1], p)).double() if p > 0 else v

    a = drop(x, 0)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        z = a @ W.t() + (0 if b is None else b)
        if i < len(Ws) - 1:
            a = {0: torch.relu, 2: lambda v: torch.nn.functional.prelu(v, slope)}[act](z)
            a = drop(a, i + 1)
    T = z.shape[1]
    y, w = table[:, :T], table[:, T:2 * T]
    m = (w != 0) if mask_from_w else (y != 0)
    rows = m.any(dim=1)
    zr, mr, yr, wr = z[rows], m[rows], y[rows], w[rows]
    if s_act == 0:
        logp = torch.log_softmax(zr.masked_fill(~mr, -math.inf), dim=1)
        pr = torch.exp(logp)
        logp = torch.where(mr, logp, torch.zeros_like(logp))
    else:
        s = torch.nn.functional.softplus(zr) * mr
        pr = s / s.sum(dim=1, keepdim=True)
        logp = torch.log(torch.where(mr, pr, torch.ones_like(pr)))
    if kind == 0:
        per = torch.where(mr, (pr - yr) * (logp - torch.log(torch.where(mr, yr, torch.ones_like(yr)))),
                          torch.zeros_like(pr))
    else:
        per = torch.abs(torch.cumsum(yr, dim=1) - torch.cumsum(pr, dim=1))
    loss = (per * wr).sum() * inv_n
    loss.backward()
    out = torch.exp(z) if s_act == 0 else torch.nn.functional.softplus(z)
    res = {'loss': loss.detach().numpy(), 'out': out.detach().numpy(), 'dx': x.grad.numpy(),
           'dslope': slope.grad.numpy() if slope is not None and slope.grad is not None else np.zeros(1)}
    for i in range(len(Ws)):
        res[f'dW{i + 1}'] = Ws[i].grad.numpy()
        if bs[i] is not None:
            res[f'db{i + 1}'] = bs[i].grad.numpy()
    return res


def _problem(B, T, Hf, n, act, F=40, seed=0):
    """Random layers and inputs, and a loss table: positive targets (each row summing to about 1), about a quarter
    of them missing (target 0, weight 0), non-unit weights; with B >= 5 row 1 has no target at all and row 3 a
    single one."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + n + seed)
    widths = [F] + [Hf] * (n - 1) + [T]
    Ws = [(torch.randn(widths[i + 1], widths[i], generator=g) / math.sqrt(widths[i])).to(DEV) for i in range(n)]
    bs = [(0.3 * torch.randn(widths[i + 1], generator=g)).to(DEV) for i in range(n)]
    x = torch.randn(B, F, generator=g).to(DEV)
    slope = torch.tensor([0.2], device=DEV) if act == 'PReLU' else None
    present = torch.rand(B, T, generator=g) >= 0.25
    if T == 1:
        present[:] = True
    if B >= 5:
        present[1, :] = False
        present[3, :] = False
        present[3, T // 2] = True
    y = torch.rand(B, T, generator=g) + 0.05
    y = y * present
    y = y / y.sum(dim=1, keepdim=True).clamp_min(1e-30) * (0.8 + 0.4 * torch.rand(B, 1, generator=g))
    w = (0.5 + torch.rand(B, T, generator=g)) * present
    table = torch.cat([y, w], dim=1).float().to(DEV)
    return x, Ws, bs, slope, ACT[act], table, 1.0 / float(present.sum())


# B: one row, no multiple of a tile, more than one tile; T: one element, just past a wave, no multiple of 16 or
# 256, more than four elements per thread; Hf 37 / 48; L 1 .. 3; both activations, both losses, dropout, PReLU
GRID = [(1, 1, 37, 1, 'exp', 'sid', 0.0, 'ReLU'),
        (1, 65, 37, 2, 'exp', 'wasserstein', 0.25, 'PReLU'),
        (1, 300, 48, 3, 'softplus', 'sid', 0.0, 'ReLU'),
        (1, 1030, 37, 2, 'softplus', 'wasserstein', 0.0, 'PReLU'),
        (5, 1, 48, 2, 'exp', 'wasserstein', 0.0, 'ReLU'),
        (5, 65, 37, 1, 'exp', 'sid', 0.25, 'ReLU'),
        (5, 65, 48, 3, 'softplus', 'wasserstein', 0.25, 'PReLU'),
        (5, 300, 37, 2, 'exp', 'sid', 0.0, 'PReLU'),
        (5, 300, 48, 1, 'softplus', 'wasserstein', 0.0, 'ReLU'),
        (5, 1030, 37, 3, 'exp', 'wasserstein', 0.25, 'ReLU'),
        (5, 1030, 48, 2, 'softplus', 'sid', 0.25, 'PReLU'),
        (5, 1030, 37, 1, 'softplus', 'sid', 0.25, 'ReLU'),
        (18, 1, 37, 3, 'exp', 'sid', 0.25, 'PReLU'),
        (18, 65, 48, 2, 'softplus', 'sid', 0.0, 'ReLU'),
        (18, 65, 37, 2, 'exp', 'wasserstein', 0.0, 'ReLU'),
        (18, 300, 37, 3, 'softplus', 'sid', 0.25, 'PReLU'),
        (18, 300, 48, 2, 'exp', 'wasserstein', 0.25, 'ReLU'),
        (18, 1030, 48, 1, 'exp', 'sid', 0.0, 'ReLU'),
        (18, 1030, 37, 2, 'softplus', 'wasserstein', 0.25, 'PReLU'),
        (18, 1030, 48, 3, 'exp', 'sid', 0.0, 'PReLU')]


def _compare(got, ref, dslope):
    assert got.keys() <= ref.keys()
    errs = {k: golden_io.normwise(got[k], ref[k]) for k in got if k != 'dslope'}
    if dslope:
        errs['dslope'] = golden_io.normwise(got['dslope'], ref['dslope'])
    elif 'dslope' in got:
        assert got['dslope'][0] == 0.0
    print({k: f'{v:.2e}' for k, v in errs.items()})
    assert all(np.isfinite(v).all() for v in got.values())
    for k, e in errs.items():
        assert e <= TOL, (k, e)


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,Hf,n,s_act,loss,p,act', GRID)
def test_spectra_head_matches_the_fp64_reference(B, T, Hf, n, s_act, loss, p, act):
    """Loss, act_s(z_L) and every gradient within 1e-5 normwise of fp64 torch ops with the masks of dropout_mask."""
    x, Ws, bs, slope, code, table, inv_n = _problem(B, T, Hf, n, act)
    seed = 0xC0FFEE + n
    args = (x, Ws, bs, slope, code, p, seed, S_ACT[s_act], LOSS[loss], table, inv_n)
    _compare(_call(*args), _reference(*args), act == 'PReLU' and n > 1)


@pytest.mark.gpu
@pytest.mark.parametrize('loss', ['sid', 'wasserstein'])
def test_logits_of_plus_and_minus_100_stay_finite(loss):
    """exp with the last layer's biases at +100, -100 and 0 in turn: exp(z) itself overflows fp32, the loss and
    the gradients are finite and within the bar of the fp64 max-subtracted form."""
    x, Ws, bs, slope, code, table, inv_n = _problem(5, 65, 37, 2, 'PReLU')
    with torch.no_grad():
        bs[-1].copy_(torch.tensor([100.0, -100.0, 0.0], device=DEV).repeat(22)[:65])
    args = (x, Ws, bs, slope, code, 0.0, 1, 0, LOSS[loss], table, inv_n)
    got = _call(*args, want_out=False)
    ref = _reference(*args)
    assert ref['out'].max() > 3.5e38  # (beyond fp32)
    del ref['out']
    _compare(got, ref, True)
    assert float(np.abs(got['dW2']).max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize('s_act,loss', [('exp', 'sid'), ('softplus', 'wasserstein')])
def test_a_present_target_with_weight_zero_still_counts_in_the_row_sum(s_act, loss):
    """Present targets whose weight is 0 (a data or target weight of 0) stay in S: the mask comes from the
    table's targets, not from w.  The oracle with the mask taken from w gives another loss."""
    x, Ws, bs, slope, code, table, inv_n = _problem(5, 65, 37, 2, 'ReLU')
    with torch.no_grad():
        table[0, 65:] = 0.0        # a row whose data weight is 0: present everywhere it was
        table[2, 65:65 + 20] = 0.0
        table[4, 65 + 7] = 0.0
    assert int(((table[:, :65] != 0) & (table[:, 65:] == 0)).sum()) > 20
    args = (x, Ws, bs, slope, code, 0.0, 1, S_ACT[s_act], LOSS[loss], table, inv_n)
    got, ref = _call(*args), _reference(*args)
    _compare(got, ref, False)
    other = _reference(*args, mask_from_w=True)
    assert golden_io.normwise(other['loss'], ref['loss']) > 1e-3
    assert golden_io.normwise(got['loss'], other['loss']) > 1e-3


@pytest.mark.gpu
def test_spectra_head_is_bitwise_repeatable_and_partial_calls_agree():
    """Two calls give identical bytes; a call that asks for some gradients only gives those bitwise as the full
    call does (and the loss and the output)."""
    x, Ws, bs, slope, code, table, inv_n = _problem(18, 1030, 37, 3, 'PReLU')
    for s_act, kind in ((0, 1), (1, 0)):
        args = (x, Ws, bs, slope, code, 0.25, 99, s_act, kind, table, inv_n)
        a, b = _call(*args), _call(*args)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        assert _call(*args[:6], 100, *args[7:])['loss'] != a['loss']
        for want in (set(), {'dx'}, {'dW3'}, {'db3', 'dslope'}, {'dW2', 'db1'}, {'dW1'}):
            part = _call(*args, want=want)
            assert set(part) == want | {'loss', 'out'}
            for k in part:
                assert np.array_equal(part[k], a[k]), (want, k)


# ---------------------------------------------------------------------------------------------------
# GPU: through chemprop_amd.train and MoleculeModel
# ---------------------------------------------------------------------------------------------------
def _model(tasks, layers=2, act='ReLU', dropout=0.0, s_act='exp', hidden=48, ffn_hidden=40):
    from chemprop_amd.nn_utils import initialize_weights
    args = TrainArgs(hidden_size=hidden, depth=3, activation=act, ffn_hidden_size=ffn_hidden, ffn_num_layers=layers,
                     dropout=dropout, device=DEV, dataset_type='spectra', spectra_activation=s_act, bias=True)
    args.num_tasks = tasks
    torch.manual_seed(0)
    m = MoleculeModel(args)
    initialize_weights(m)
    with torch.no_grad():  # (initialize_weights zeroes every 1-D parameter: give the slopes and the FFN's biases values)
        g = torch.Generator().manual_seed(5)
        for mod in m.modules():
            if isinstance(mod, torch.nn.PReLU):
                mod.weight.fill_(0.25)
        for mod in m.ffn:
            if isinstance(mod, torch.nn.Linear):
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
    return m.to(DEV)


def _spectra_targets(b, T, seed):
    """Normalised positive rows with about 15 % of the entries missing (never a whole row)."""
    rng = np.random.default_rng(seed)
    raw = [[None if rng.random() < 0.15 else float(rng.gamma(2.0)) + 0.01 for _ in range(T)] for _ in range(b)]
    return spectra_utils.normalize_spectra(raw, threshold=1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [65, 1030])
def test_spectra_predict_head(T):
    """normalize=0 is the model's torch FFN; normalize=1 is normalize_spectra, with and without a mask: NaN at the
    excluded positions, the included ones summing to 1; the eval no-grad forward IS the native head."""
    from chemprop_amd.train import _StackHead, _predict_head, head_predict
    b = 9
    for layers, s_act in ((2, 'exp'), (1, 'softplus'), (3, 'softplus')):
        m = _model(T, layers, 'PReLU', 0.1, s_act).eval()
        head = _predict_head(m)
        assert isinstance(head, _StackHead) and head.spectra == S_ACT[s_act]
        g = BatchMolGraph(synthetic.make_batch('polymer', b, 77), device_bond_features=True)
        ref = m([g]).detach()  # (grad enabled: the torch ops)
        with torch.no_grad():
            emb = m.encoder([g])
            out = head_predict(m, emb)
            fwd = m([g])
            norm = head_predict(m, emb, normalize=True)
            mask = torch.rand(b, T, generator=torch.Generator().manual_seed(T)) < 0.7
            mask[0, :] = True
            masked = head_predict(m, emb, normalize=True, mask=mask.to(DEV))
            masked8 = head_predict(m, emb, normalize=True, mask=mask.to(DEV).to(torch.uint8))
        assert out.shape == ref.shape == (b, T) and torch.equal(fwd, out)
        assert golden_io.normwise(out.cpu().numpy(), ref.cpu().numpy()) <= TOL
        want = np.array(spectra_utils.normalize_spectra(ref.cpu().numpy().tolist()), np.float64)
        assert golden_io.normwise(norm.cpu().numpy(), want) <= TOL
        assert float((norm.sum(dim=1) - 1).abs().max()) <= 1e-6
        got = masked.cpu().numpy()
        assert torch.equal(masked.isnan(), masked8.isnan()) and torch.equal(masked.nan_to_num(), masked8.nan_to_num())
        assert np.array_equal(np.isnan(got), ~mask.numpy()) and np.isnan(got).any()
        # (normalize_spectra's phase mask: one phase per row here, the row's own mask)
        want = np.array(spectra_utils.normalize_spectra(ref.cpu().numpy().tolist(), np.eye(b), mask.numpy(),
                                                        excluded_sub_value=float('nan')), np.float64)
        assert np.array_equal(np.isnan(want), np.isnan(got))
        assert golden_io.normwise(np.nan_to_num(got), np.nan_to_num(want)) <= TOL
        assert float(np.abs(np.nansum(got.astype(np.float64), axis=1) - 1).max()) <= 1e-6
    with pytest.raises(ValueError):
        head_predict(m, emb, normalize=False, mask=mask.to(DEV))
    with pytest.raises(ValueError):
        head_predict(m, emb, normalize=True, mask=mask[:, :-1].to(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize('alt', [None, 'wasserstein'])
def test_spectra_steps_take_the_fused_direct_path(alt):
    """T = 300, two batches over two epochs: the direct step and the autograd step with the fused head give
    bitwise equal losses and parameters, both within 1e-5 (losses) / 1e-4 normwise (parameters) of the torch ops."""
    from chemprop_amd.train import _StackHead, _direct_encoder, _fusable_head, build_optimizer, get_loss_func, train_step
    T = 300
    graphs = [BatchMolGraph(synthetic.make_batch('polymer', 12, 60 + i), device_bond_features=True) for i in range(2)]
    targets = [_spectra_targets(12, T, 7 + i) for i in range(2)]
    lf = get_loss_func('spectra', alt)
    res = []
    for mode in ('direct', 'autograd', 'torch'):
        m = _model(T, 2, 'ReLU')
        head = _fusable_head(m.train(), lf, 'spectra')
        assert isinstance(head, _StackHead) and head.spectra == 0 and head.kind == (1 if alt else 0)
        assert _fusable_head(m, get_loss_func('regression'), 'regression') is None
        assert _direct_encoder(m, [graphs[0]], None, head) is m.encoder.encoder[0]
        opt = build_optimizer(m, 1e-3)
        losses = [float(train_step(m, [g], t, lf, opt, dataset_type='spectra', direct=mode == 'direct',
                                   fused_head=mode != 'torch'))
                  for _ in range(2) for g, t in zip(graphs, targets)]
        assert all(math.isfinite(v) for v in losses)
        res.append((losses, [q.detach().clone() for q in m.parameters()]))
    assert res[0][0] == res[1][0]
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    for a, b in zip(res[0][0], res[2][0]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (a, b)
    for a, b in zip(res[0][1], res[2][1]):
        assert golden_io.normwise(a.cpu().numpy(), b.cpu().numpy()) <= 1e-4
    # the other dataset types keep their limits: 65 outputs are not a fusable multiclass head
    args = TrainArgs(hidden_size=48, depth=3, ffn_num_layers=3, device=DEV, dataset_type='multiclass',
                     multiclass_num_classes=5)
    args.num_tasks = 13
    assert _fusable_head(MoleculeModel(args).to(DEV).train(), get_loss_func('multiclass'), 'multiclass') is None


@pytest.mark.gpu
def test_a_frozen_encoder_steps_from_cached_encodings():
    """Encoder frozen, T = 300 with a softplus output: the step runs from ``frozen_encodings`` and leaves the head
    gradients the unfrozen machinery (head_loss under autograd on the same encodings) computes, bitwise."""
    from chemprop_amd.train import _fusable_head, build_optimizer, frozen_encodings, get_loss_func, head_loss, train_step
    T, b = 300, 12
    mols = synthetic.make_batch('polymer', b, 91)
    targets = _spectra_targets(b, T, 3)
    lf = get_loss_func('spectra')
    frozen, free = _model(T, 2, 'PReLU', s_act='softplus'), _model(T, 2, 'PReLU', s_act='softplus')
    for q in frozen.encoder.parameters():
        q.requires_grad = False
    enc = frozen_encodings(frozen, mols, 8)
    assert enc.shape == (b, 48)
    head = _fusable_head(free.train(), lf, 'spectra')
    x = enc.clone().requires_grad_(True)
    ref_loss = head_loss(x, head, targets)
    ref_loss.backward()
    assert x.grad is not None and bool(x.grad.abs().sum() > 0)
    opt = build_optimizer(frozen, 1e-3)
    loss = train_step(frozen, None, targets, lf, opt, dataset_type='spectra', encodings=enc)
    assert float(loss) == float(ref_loss.detach())
    for (n, a), (_, c) in zip(frozen.ffn.named_parameters(), free.ffn.named_parameters()):
        assert a.grad is not None and torch.equal(a.grad, c.grad), n
    assert all(q.grad is None for q in frozen.encoder.parameters())


def _fixture_model(case):
    a = case.args
    a.device = DEV
    m = MoleculeModel(a)
    synthetic.fill_parameters(m, case.seed)
    return m.to(DEV)


@pytest.mark.gpu
def test_reference_spectra_model():
    """The reference's own spectra MoleculeModel (2 layers, hidden 48, 65 outputs, exp): the eval output, both
    training losses and their gradients through head_loss within 1e-5 normwise; the normalised predictions under
    the 2-phase mask and both metrics match the stored values."""
    from chemprop_amd.train import _StackHead, _fusable_head, get_loss_func, head_loss, head_predict
    case = golden_io.load(FIXTURE)
    z = _fixture()
    m = _fixture_model(case).eval()
    assert m.spectra and m.ffn[4].out_features == 65 and len(m.ffn) == 6
    with torch.no_grad():
        out = m(case.graphs, None)
    assert out.shape == case.output.shape == (8, 65)
    assert golden_io.normwise(out.cpu().numpy(), case.output) <= TOL
    row_mask = spectra_utils.phase_row_mask(z['phase_features'], z['phase_mask'])
    with torch.no_grad():
        norm = head_predict(m, m.encoder(case.graphs, None), normalize=True,
                            mask=torch.from_numpy(row_mask).to(DEV)).cpu().numpy()
    assert np.array_equal(np.isnan(norm), np.isnan(z['normalized'])) and np.isnan(norm).any()
    assert golden_io.normwise(np.nan_to_num(norm), np.nan_to_num(z['normalized'])) <= TOL
    targets = _fixture_targets(z)
    assert sum(v is None for r in targets for v in r) >= 20
    preds = out.cpu().numpy().tolist()
    assert spectra_utils.sid_metric(preds, targets) == pytest.approx(float(z['sid_metric']), rel=TOL)
    assert spectra_utils.wasserstein_metric(preds, targets) == pytest.approx(float(z['wasserstein_metric']), rel=TOL)
    m.train()
    for name, alt in (('sid', None), ('wasserstein', 'wasserstein')):
        m.zero_grad()
        head = _fusable_head(m, get_loss_func('spectra', alt), 'spectra')
        assert isinstance(head, _StackHead)
        loss = head_loss(m.encoder(case.graphs, None), head, targets, list(z['target_weights']),
                         list(z['data_weights']))
        loss.backward()
        got, ref = float(loss.detach()), float(z[f'{name}/train_loss'])
        print(f'{name}: spectra head loss {got!r} reference {ref!r}')
        assert golden_io.normwise(got, ref) <= TOL
        names = [k[len(f'{name}/train_grad/'):] for k in z.files if k.startswith(f'{name}/train_grad/')]
        assert sorted(names) == sorted(n for n, q in m.named_parameters() if q.grad is not None)
        for n, q in m.named_parameters():
            if q.grad is not None:
                e = golden_io.normwise(q.grad.cpu().numpy(), z[f'{name}/train_grad/{n}'])
                assert e <= TOL, (name, n, e)
