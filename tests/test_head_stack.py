"""The native stack head (``wdmpnn_head_stack`` / ``wdmpnn_head_stack_predict``): FFNs with 1 .. 6 Linear
layers, active dropout (counter-hash masks, ``nn_utils.dropout_mask``) and PReLU, and their wiring through
``chemprop_amd.train`` and ``MoleculeModel``.

CPU: the header, the binding and the library agree on the new symbols and struct layouts (ABI still 12); the
entry points' refusals (nothing is launched); ``dropout_mask``; structure recognition.
GPU: the mask contract, loss and every gradient against fp64 torch ops with explicit masks, bitwise
repeatability, the direct and the autograd step, the torch path of the same models, the fixture made from the
reference's own model (tools/make_head_stack_golden.py), ``head_predict``."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import TrainArgs, _native, synthetic
from chemprop_amd.featurization import BatchMolGraph
from chemprop_amd.model import MoleculeModel
from chemprop_amd.nn_utils import dropout_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')
TOL = 1e-5
DEV = torch.device('cuda:0')
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -1000, -1001, -1002, -1003
FIXTURE = 'head_stack/model_polymer_ffn3_prelu'
ACT = {'ReLU': 0, 'PReLU': 2, 'tanh': 3}


# ---------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_stack_head(tmp_path):
    """The three new entry points are declared, bound and exported, the ABI version is still 12, and
    WdHeadStack / WdHeadStackPredict have the layout a C compiler gives the header."""
    text = open(HEADER).read()
    assert '#define WDMPNN_ABI_VERSION 12' in text and '#define WD_HEAD_MAX_LAYERS 6' in text
    assert _native.ABI_VERSION == 12 and _native.HEAD_MAX_LAYERS == 6
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for fn in ('wdmpnn_head_stack', 'wdmpnn_head_stack_predict', 'wdmpnn_head_stack_scratch_bytes'):
        assert re.search(r'\bint\s+%s\s*\(' % fn, text), fn
        assert fn in _native.EXPORTED_SYMBOLS
        assert re.search(r'\bT %s\b' % fn, out), fn
    L = _native.lib()
    assert L.wdmpnn_abi_version() == 12
    assert L.wdmpnn_head_stack.argtypes[0]._type_ is _native.WdHeadStack
    assert L.wdmpnn_head_stack_predict.argtypes[0]._type_ is _native.WdHeadStackPredict
    S, P = _native.WdHeadStack, _native.WdHeadStackPredict
    sf = [n for n, _ in S._fields_]
    pf = [n for n, _ in P._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wdmpnn.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(WdHeadStack), sizeof(WdHeadStackPredict));\n' +
                   ''.join(f'  printf(" %zu", offsetof(WdHeadStack, {n}));\n' for n in sf) +
                   ''.join(f'  printf(" %zu", offsetof(WdHeadStackPredict, {n}));\n' for n in pf) +
                   '  printf("\\n"); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC', 'gcc'), '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert c == [ctypes.sizeof(S), ctypes.sizeof(P)] + [getattr(S, n).offset for n in sf] + \
        [getattr(P, n).offset for n in pf]


def _fake_stack(L=3, T=6, kind=2, n_classes=3, p=0.25, ld_table=None, B=4, scratch=4096, F=32, Hf=16):
    """A WdHeadStack of made-up addresses (never dereferenced: every call below is refused on the host)."""
    a = 4096
    h = _native.WdHeadStack()
    h.x, h.ld_x, h.B, h.F, h.Hf, h.T, h.L = a, F, B, F, Hf, T, L
    for i in range(min(max(L, 0), _native.HEAD_MAX_LAYERS)):
        h.W[i], h.b[i], h.dW[i], h.db[i] = a, a, a, a
    tasks = T // n_classes if n_classes > 0 and T % n_classes == 0 else T
    h.slope, h.table, h.ld_table, h.inv_n, h.act = a, a, 2 * tasks if ld_table is None else ld_table, 1.0, 2
    h.p, h.seed, h.loss_kind, h.n_classes = p, 7, kind, n_classes
    h.scratch, h.scratch_bytes = scratch, 1 << 30
    h.dx, h.dslope, h.loss = a, a, a
    return h


@pytest.mark.parametrize('kw,rc', [(dict(L=0), ERR_SHAPE),
                                   (dict(L=7), ERR_UNSUPPORTED),
                                   (dict(T=65, n_classes=5), ERR_UNSUPPORTED),
                                   (dict(T=65, kind=0, n_classes=1), ERR_UNSUPPORTED),
                                   (dict(F=4097), ERR_UNSUPPORTED),
                                   (dict(Hf=4097), ERR_UNSUPPORTED),
                                   (dict(p=-0.1), ERR_ARG),
                                   (dict(p=1.0), ERR_ARG),
                                   (dict(p=float('nan')), ERR_ARG),
                                   (dict(T=7, n_classes=3), ERR_SHAPE),
                                   (dict(kind=0, n_classes=3), ERR_SHAPE),
                                   (dict(kind=3, n_classes=1), ERR_UNSUPPORTED),
                                   (dict(ld_table=3), ERR_SHAPE),
                                   (dict(scratch=0), ERR_ARG)])
def test_stack_head_refusals_launch_nothing(kw, rc):
    L = _native.lib()
    h = _fake_stack(**kw)
    got = L.wdmpnn_head_stack(ctypes.byref(h), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()
    with pytest.raises((ValueError, NotImplementedError, _native.NativeError)):
        _native.check(got, 'head stack')


def test_stack_head_refuses_a_small_scratch_and_sizes_it():
    L = _native.lib()
    B, F, Hf, T, n = 5, 40, 37, 6, 3
    tiles = ((B + 15) // 16) * ((Hf + 15) // 16)
    want = 4 * ((n - 1) * (2 * B * Hf + max(B, tiles)) + B * Hf + B * T + B)
    assert _native.head_stack_scratch_bytes(B, F, Hf, T, n) == want
    assert _native.head_stack_scratch_bytes(B, F, 0, T, 1) == 4 * (B * F + B * T + B)
    h = _fake_stack(L=n, B=B, F=F, Hf=Hf, T=T)
    h.scratch_bytes = want - 4
    assert L.wdmpnn_head_stack(ctypes.byref(h), None) == ERR_WORKSPACE
    assert 'scratch' in L.wdmpnn_last_error().decode()


def test_stack_entries_without_rows_are_no_ops():
    L = _native.lib()
    h = _fake_stack(B=0)
    assert L.wdmpnn_head_stack(ctypes.byref(h), None) == 0
    q = _native.WdHeadStackPredict()
    q.ld_x, q.B, q.F, q.Hf, q.T, q.L, q.act, q.out_kind, q.n_classes = 32, 0, 32, 16, 6, 2, 2, 2, 3
    q.W[0], q.W[1], q.slope = 4096, 4096, 4096
    assert L.wdmpnn_head_stack_predict(ctypes.byref(q), None) == 0
    q.T = 65
    assert L.wdmpnn_head_stack_predict(ctypes.byref(q), None) == ERR_UNSUPPORTED
    q.T, q.L = 6, 7
    assert L.wdmpnn_head_stack_predict(ctypes.byref(q), None) == ERR_UNSUPPORTED


def test_dropout_mask_contract():
    p = 0.3
    m = dropout_mask(1234567890123, 2, 256, 256, p)
    assert m.dtype == np.float32 and m.shape == (256, 256)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert set(np.unique(m).tolist()) == {0.0, float(keep)}
    n = m.size
    frac = float((m > 0).mean())
    assert abs(frac - (1 - p)) <= 3 * math.sqrt(p * (1 - p) / n), frac
    assert np.array_equal(m, dropout_mask(1234567890123, 2, 256, 256, p))
    assert not np.array_equal(m, dropout_mask(1234567890123, 3, 256, 256, p))
    assert not np.array_equal(m, dropout_mask(1234567890124, 2, 256, 256, p))
    # a smaller mask is the corner of a larger one: the element's hash depends on (row, col) alone
    assert np.array_equal(dropout_mask(5, 0, 7, 9, p), dropout_mask(5, 0, 64, 64, p)[:7, :9])
    assert np.array_equal(dropout_mask(5, 0, 4, 4, 0.0), np.ones((4, 4), np.float32))
    # one element by hand (python integers): splitmix64's finaliser of seed ^ G (layer + 1) ^ (row << 32 | col)
    M, G = (1 << 64) - 1, 0x9E3779B97F4A7C15
    x = (5 ^ (G * 2 & M) ^ ((3 << 32) | 6)) + G & M
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9 & M
    x = (x ^ (x >> 27)) * 0x94D049BB133111EB & M
    x ^= x >> 31
    u = np.float32(x >> 40) * np.float32(1.0 / 16777216.0)
    assert dropout_mask(5, 1, 4, 7, p)[3, 6] == (keep if u >= np.float32(p) else 0.0)


def _cpu_model(layers=2, act='ReLU', dropout=0.0, tasks=2, dataset='regression', C=3):
    args = TrainArgs(hidden_size=32, depth=3, activation=act, ffn_hidden_size=24, ffn_num_layers=layers,
                     dropout=dropout, device=torch.device('cpu'), dataset_type=dataset, multiclass_num_classes=C)
    args.num_tasks = tasks
    return MoleculeModel(args)


def test_ffn_structure_recognition():
    """The structure helper (no device needed) accepts every FFN of create_ffn within the limits; _fusable_head
    on a CPU model is None (its parameters are not on the GPU)."""
    from chemprop_amd.train import _StackHead, _ffn_structure, _fusable_head, get_loss_func
    for layers in (1, 2, 3, 6):
        m = _cpu_model(layers, 'PReLU', 0.1)
        st = _ffn_structure(m.ffn, True)
        assert isinstance(st, _StackHead) and len(st.linears) == layers
        assert st.linears == [l for l in m.ffn if isinstance(l, torch.nn.Linear)]
        assert st.p == pytest.approx(0.1) and _ffn_structure(m.ffn, False).p == 0.0
        if layers > 1:
            assert st.act == 2 and st.slope is m.ffn[2].weight
            assert [id(t) for t in st.params() if t is not None].count(id(st.slope)) == 1
        else:
            assert st.act == 6 and st.slope is None
        assert _fusable_head(m, get_loss_func('regression'), 'regression') is None  # (CPU parameters)
    assert _ffn_structure(_cpu_model(7).ffn, True) is None
    assert _ffn_structure(_cpu_model(3, tasks=65).ffn, True) is None
    assert _ffn_structure(_cpu_model(3, tasks=64).ffn, True) is not None
    m = _cpu_model(3, 'PReLU')
    shared = torch.nn.PReLU(num_parameters=24)
    m.ffn[2] = m.ffn[5] = shared
    assert _ffn_structure(m.ffn, True) is None
    m = _cpu_model(3, 'PReLU')
    m.ffn[5] = torch.nn.PReLU()  # two slopes: not the reference's single activation module
    assert _ffn_structure(m.ffn, True) is None
    m = _cpu_model(2)
    m.ffn.append(torch.nn.Softplus())
    assert _ffn_structure(m.ffn, True) is None


# ---------------------------------------------------------------------------------------------------
# GPU: the entry point itself
# ---------------------------------------------------------------------------------------------------
def _call_stack(x, Ws, bs, slope, act, p, seed, kind, C, table, inv_n):
    """One wdmpnn_head_stack call on device tensors: loss, out, dx, dW, db, dslope (numpy)."""
    B, F = x.shape
    n, T = len(Ws), Ws[-1].shape[0]
    Hf = Ws[0].shape[0] if n > 1 else 0
    nbytes = _native.head_stack_scratch_bytes(B, F, Hf, T, n)
    # NaN-filled: the entry point must write everything it reads
    scratch = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device=DEV)
    new = lambda t: torch.full_like(t, float('nan'))  # noqa: E731
    dx, dW, db = new(x), [new(W) for W in Ws], [None if b is None else new(b) for b in bs]
    out = torch.full((B, T), float('nan'), dtype=torch.float32, device=DEV)
    dslope = torch.full((1,), float('nan'), dtype=torch.float32, device=DEV)
    loss = torch.full((), float('nan'), dtype=torch.float32, device=DEV)
    h = _native.WdHeadStack()
    h.x, h.ld_x, h.B, h.F, h.Hf, h.T, h.L = x.data_ptr(), F, B, F, Hf, T, n
    for i in range(n):
        h.W[i], h.b[i], h.dW[i], h.db[i] = Ws[i].data_ptr(), _native.ptr(bs[i]), dW[i].data_ptr(), _native.ptr(db[i])
    h.slope, h.table, h.ld_table, h.inv_n, h.act = _native.ptr(slope), table.data_ptr(), table.shape[1], inv_n, act
    h.p, h.seed, h.loss_kind, h.n_classes = p, seed, kind, C
    h.scratch, h.scratch_bytes = scratch.data_ptr(), nbytes
    h.out, h.dx, h.dslope, h.loss = out.data_ptr(), dx.data_ptr(), dslope.data_ptr(), loss.data_ptr()
    _native.check(_native.lib().wdmpnn_head_stack(ctypes.byref(h), _native.current_stream(DEV)), 'head stack')
    torch.cuda.synchronize()
    res = {'loss': loss.cpu().numpy(), 'out': out.cpu().numpy(), 'dx': dx.cpu().numpy(),
           'dslope': dslope.cpu().numpy()}
    for i in range(n):
        res[f'dW{i + 1}'] = dW[i].cpu().numpy()
        if db[i] is not None:
            res[f'db{i + 1}'] = db[i].cpu().numpy()
    return res


@pytest.mark.gpu
def test_mask_contract_on_the_device():
    """L = 1 with W_1 = I and no bias: the FFN's output IS drop_0(x), exactly x * dropout_mask(seed, 0, ...);
    with MSE against zero targets dx = 2 / n * drop_0(drop_0(x)) is zero exactly where the mask is."""
    B, F, p, seed = 5, 40, 0.25, 0x1234567890ABCDEF
    x = torch.randn(B, F, generator=torch.Generator().manual_seed(0)).to(DEV)
    W = torch.eye(F, device=DEV)
    table = torch.cat([torch.zeros(B, F), torch.ones(B, F)], dim=1).to(DEV)
    r = _call_stack(x, [W], [None], None, 0, p, seed, 0, 1, table, 1.0 / (B * F))
    mask = dropout_mask(seed, 0, B, F, p)
    assert 0 < (mask == 0).sum() < mask.size
    assert np.array_equal(r['out'], x.cpu().numpy() * mask)
    assert np.array_equal(r['dx'] == 0, mask == 0)
    assert r['dslope'][0] == 0.0


def _reference(x, Ws, bs, slope, act, p, seed, kind, C, table, inv_n):
    """The same head in fp64 torch ops on the CPU with explicit masks from dropout_mask."""
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
            a = {0: torch.relu, 3: torch.tanh, 2: lambda v: torch.nn.functional.prelu(v, slope)}[act](z)
            a = drop(a, i + 1)
    K = z.shape[1] // C
    y, w = table[:, :K], table[:, K:2 * K]
    if kind == 0:
        per = (z - y) ** 2
    elif kind == 1:
        per = torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction='none')
    else:
        logits = z.reshape(B, K, C)
        per = torch.stack([torch.nn.functional.cross_entropy(logits[:, k, :], y[:, k].long(), reduction='none')
                           for k in range(K)], dim=1)
    loss = (per * w).sum() * inv_n
    loss.backward()
    res = {'loss': loss.detach().numpy(), 'out': z.detach().numpy(), 'dx': x.grad.numpy(),
           'dslope': slope.grad.numpy() if slope is not None and slope.grad is not None else np.zeros(1)}
    for i in range(len(Ws)):
        res[f'dW{i + 1}'] = Ws[i].grad.numpy()
        if bs[i] is not None:
            res[f'db{i + 1}'] = bs[i].grad.numpy()
    return res


def _problem(n, act, kind, Hf, bias, B=5, F=40):
    """Random layers, inputs and a loss table with missing targets (weight 0) and non-unit weights."""
    g = torch.Generator().manual_seed(100 * n + 10 * kind + ACT[act])
    C = 3 if kind == 2 else 1
    T = 6 if kind == 2 else 3
    widths = [F] + [Hf] * (n - 1) + [T]
    Ws = [(torch.randn(widths[i + 1], widths[i], generator=g) / math.sqrt(widths[i])).to(DEV) for i in range(n)]
    bs = [(0.3 * torch.randn(widths[i + 1], generator=g)).to(DEV) if bias else None for i in range(n)]
    x = torch.randn(B, F, generator=g).to(DEV)
    slope = torch.tensor([0.2], device=DEV) if act == 'PReLU' else None
    K = T // C
    if kind == 0:
        y = torch.randn(B, K, generator=g)
    elif kind == 1:
        y = (torch.rand(B, K, generator=g) < 0.5).float()
    else:
        y = torch.randint(0, C, (B, K), generator=g).float()
    w = 0.5 + torch.rand(B, K, generator=g)
    w[1, 0] = 0.0  # a missing target
    w[3, :] = 0.0  # a row without targets
    table = torch.cat([y, w], dim=1).to(DEV)
    return x, Ws, bs, slope, ACT[act], C, table, 1.0 / float((w > 0).sum())


GRID = [(1, 0.0, 'ReLU', 0, 37, True),
        (1, 0.25, 'ReLU', 1, 37, True),
        (2, 0.25, 'PReLU', 0, 37, True),
        (2, 0.0, 'tanh', 2, 37, True),
        (3, 0.25, 'PReLU', 2, 37, True),
        (3, 0.0, 'PReLU', 1, 330, True),   # the K loop crosses SG_KC = 320
        (4, 0.25, 'tanh', 1, 37, False),   # no biases
        (4, 0.0, 'ReLU', 0, 37, True),
        (3, 0.25, 'ReLU', 2, 37, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('n,p,act,kind,Hf,bias', GRID)
def test_stack_head_matches_the_fp64_reference(n, p, act, kind, Hf, bias):
    """Loss, outputs and every gradient within 1e-5 normwise of fp64 torch ops with the masks of dropout_mask:
    B = 5 (no multiple of the 4 rows per workgroup nor of a tile), F = 40, Hf = 37, T = 3 (6 = 2 x 3 classes for
    kind 2), missing targets, non-unit weights."""
    x, Ws, bs, slope, code, C, table, inv_n = _problem(n, act, kind, Hf, bias)
    seed = 0xC0FFEE + n
    got = _call_stack(x, Ws, bs, slope, code, p, seed, kind, C, table, inv_n)
    ref = _reference(x, Ws, bs, slope, code, p, seed, kind, C, table, inv_n)
    assert got.keys() == ref.keys()
    errs = {k: golden_io.normwise(got[k], ref[k]) for k in ref if k != 'dslope'}
    if act == 'PReLU' and n > 1:
        errs['dslope'] = golden_io.normwise(got['dslope'], ref['dslope'])
    else:
        assert got['dslope'][0] == 0.0
    print({k: f'{v:.2e}' for k, v in errs.items()})
    assert all(np.isfinite(v).all() for v in got.values())
    for k, e in errs.items():
        assert e <= TOL, (k, e)
    if p > 0:  # the masks matter: the same call without dropout gives another loss
        other = _call_stack(x, Ws, bs, slope, code, 0.0, seed, kind, C, table, inv_n)
        assert other['loss'] != got['loss']


@pytest.mark.gpu
def test_stack_head_is_bitwise_repeatable_and_seeded():
    x, Ws, bs, slope, code, C, table, inv_n = _problem(3, 'PReLU', 2, 330, True)
    a = _call_stack(x, Ws, bs, slope, code, 0.25, 99, 2, C, table, inv_n)
    b = _call_stack(x, Ws, bs, slope, code, 0.25, 99, 2, C, table, inv_n)
    c = _call_stack(x, Ws, bs, slope, code, 0.25, 100, 2, C, table, inv_n)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert a['loss'] != c['loss']


@pytest.mark.gpu
@pytest.mark.parametrize('shape,kind,act,bias', [((5, 37, 19, 3, 1), 0, 'ReLU', True),
                                                 ((5, 37, 19, 3, 1), 1, 'tanh', True),
                                                 ((5, 37, 19, 3, 1), 0, 'tanh', False),   # b1 = b2 = NULL
                                                 ((9, 700, 33, 6, 1), 0, 'tanh', True),
                                                 ((9, 700, 33, 6, 1), 1, 'ReLU', True),
                                                 ((9, 700, 33, 6, 3), 2, 'ReLU', True),
                                                 ((9, 700, 33, 6, 3), 2, 'tanh', True)])
def test_two_layer_predict_entry_is_the_stack_predict_at_two_layers(shape, kind, act, bias):
    """wdmpnn_head_predict and wdmpnn_head_stack_predict with L = 2 on the same device inputs: bitwise equal
    outputs (scratch and out NaN-filled first: nothing left from an earlier call can pass), and within 1e-5
    normwise of an fp64 numpy evaluation.  B = 5 is a partial 4-row workgroup with partial 16 x 16 tiles;
    F = 700 is three 320-deep K stages, the last one partial; kind 2 is two tasks of three classes."""
    B, F, Hf, T, C = shape
    g = torch.Generator().manual_seed(1000 * kind + F + ACT[act])
    x = torch.randn(B, F, generator=g).to(DEV)
    W1 = (torch.randn(Hf, F, generator=g) / math.sqrt(F)).to(DEV)
    W2 = (torch.randn(T, Hf, generator=g) / math.sqrt(Hf)).to(DEV)
    b1 = (0.3 * torch.randn(Hf, generator=g)).to(DEV) if bias else None
    b2 = (0.3 * torch.randn(T, generator=g)).to(DEV) if bias else None
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=DEV)  # noqa: E731
    a, scratch, out_two, out_stack = nan(B, Hf), nan(B * Hf), nan(B, T), nan(B, T)
    ptr, stream = _native.ptr, _native.current_stream(DEV)
    p = _native.WdHeadPredict(ptr(x), F, B, F, Hf, T, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ACT[act], ptr(a),
                              ptr(out_two), kind, C)
    _native.check(_native.lib().wdmpnn_head_predict(ctypes.byref(p), stream), 'head predict')
    q = _native.WdHeadStackPredict()
    q.x, q.ld_x, q.B, q.F, q.Hf, q.T, q.L = ptr(x), F, B, F, Hf, T, 2
    q.W[0], q.b[0], q.W[1], q.b[1] = ptr(W1), ptr(b1), ptr(W2), ptr(b2)
    q.act, q.scratch, q.scratch_bytes = ACT[act], ptr(scratch), 4 * B * Hf
    q.out, q.out_kind, q.n_classes = ptr(out_stack), kind, C
    _native.check(_native.lib().wdmpnn_head_stack_predict(ctypes.byref(q), stream), 'head stack predict')
    torch.cuda.synchronize()
    assert torch.isfinite(out_two).all() and torch.equal(out_two, out_stack)
    assert torch.equal(a.view(-1), scratch)  # (z_1 in either scratch)
    f64 = lambda t: 0.0 if t is None else t.cpu().double().numpy()  # noqa: E731
    z = f64(x) @ f64(W1).T + f64(b1)
    ref = (np.maximum(z, 0) if act == 'ReLU' else np.tanh(z)) @ f64(W2).T + f64(b2)
    if kind == 1:
        ref = 1 / (1 + np.exp(-ref))
    elif kind == 2:
        e = np.exp(ref.reshape(B, T // C, C) - ref.reshape(B, T // C, C).max(axis=2, keepdims=True))
        ref = (e / e.sum(axis=2, keepdims=True)).reshape(B, T)
    err = golden_io.normwise(out_two.cpu().numpy(), ref)
    print(f'two-layer predict vs fp64: {err:.2e}')
    assert err <= TOL, err


# ---------------------------------------------------------------------------------------------------
# GPU: through chemprop_amd.train and MoleculeModel
# ---------------------------------------------------------------------------------------------------
def _model(layers, act='ReLU', dropout=0.0, dataset='regression', tasks=2, C=3, hidden=48, ffn_hidden=40):
    from chemprop_amd.nn_utils import initialize_weights
    args = TrainArgs(hidden_size=hidden, depth=3, activation=act, ffn_hidden_size=ffn_hidden, ffn_num_layers=layers,
                     dropout=dropout, device=DEV, dataset_type=dataset, multiclass_num_classes=C, bias=True)
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


def _targets(dataset, b, tasks, C, seed):
    rng = np.random.default_rng(seed)

    def one():
        if rng.random() < 0.15:
            return None
        if dataset == 'regression':
            return float(rng.normal())
        return float(rng.random() < 0.5) if dataset == 'classification' else float(rng.integers(C))
    return [[one() for _ in range(tasks)] for _ in range(b)]


@pytest.mark.gpu
def test_dropout_prelu_three_layer_steps_direct_equals_autograd():
    """dropout 0.2, ffn_num_layers 3, PReLU: the model trains through the stack head and the direct step, and
    the direct and autograd paths give bitwise equal losses, parameters and gradients under one torch seed;
    another seed gives other masks and another loss."""
    from chemprop_amd.train import _StackHead, _direct_encoder, _fusable_head, build_optimizer, get_loss_func, train_step
    graphs = [BatchMolGraph(synthetic.make_batch('polymer', 12, 30 + i), device_bond_features=True) for i in range(3)]
    targets = [_targets('regression', 12, 2, 1, i) for i in range(3)]
    lf = get_loss_func('regression')
    res = []
    for direct, seed in ((True, 11), (False, 11), (True, 12)):
        m = _model(3, 'PReLU', 0.2).train()
        head = _fusable_head(m, lf, 'regression')
        assert isinstance(head, _StackHead) and head.p == pytest.approx(0.2) and len(head.linears) == 3
        assert _direct_encoder(m, [graphs[0]], None, head) is m.encoder.encoder[0]
        opt = build_optimizer(m, 1e-3)
        torch.manual_seed(seed)
        losses = [float(train_step(m, [g], t, lf, opt, direct=direct)) for g, t in zip(graphs, targets)]
        assert all(math.isfinite(v) for v in losses)
        res.append((losses, [q.detach().clone() for q in m.parameters()],
                    [q.grad.clone() for q in m.parameters() if q.requires_grad]))
    assert res[0][0] == res[1][0]
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    assert res[0][0][0] != res[2][0][0]


@pytest.mark.gpu
@pytest.mark.parametrize('layers,dataset', [(1, 'regression'), (3, 'classification'), (3, 'multiclass')])
def test_deeper_heads_without_dropout_match_the_torch_path(layers, dataset):
    """L = 1 and L = 3 (PReLU) without dropout over four steps: direct and autograd bitwise equal, and within
    1e-5 (losses) / 1e-4 normwise (parameters) of the torch ops (fused_head=False)."""
    from chemprop_amd.train import _StackHead, _fusable_head, build_optimizer, get_loss_func, train_step
    C = 3 if dataset == 'multiclass' else 1
    graphs = [BatchMolGraph(synthetic.make_batch('polymer', 12, 60 + i), device_bond_features=True) for i in range(2)]
    targets = [_targets(dataset, 12, 2, C, 7 + i) for i in range(2)]
    lf = get_loss_func(dataset)
    res = []
    for mode in ('direct', 'autograd', 'torch'):
        m = _model(layers, 'PReLU', 0.0, dataset, 2, max(C, 2))
        assert isinstance(_fusable_head(m.train(), lf, dataset), _StackHead)
        opt = build_optimizer(m, 1e-3)
        losses = [float(train_step(m, [g], t, lf, opt, dataset_type=dataset, direct=mode == 'direct',
                                   fused_head=mode != 'torch'))
                  for _ in range(2) for g, t in zip(graphs, targets)]
        res.append((losses, [q.detach().clone() for q in m.parameters()]))
    assert res[0][0] == res[1][0]
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    for a, b in zip(res[0][0], res[2][0]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (a, b)
    for a, b in zip(res[0][1], res[2][1]):
        assert golden_io.normwise(a.cpu().numpy(), b.cpu().numpy()) <= 1e-4


@pytest.mark.gpu
def test_the_two_layer_head_keeps_its_tuple_and_entry_point():
    """Two Linears, no active dropout, no PReLU: the 5-tuple as before; with PReLU, or dropout while training,
    the stack head; 65 outputs: None."""
    from chemprop_amd.train import _StackHead, _fusable_head, _predict_head, get_loss_func
    lf = get_loss_func('regression')
    m = _model(2, 'ReLU').train()
    assert _fusable_head(m, lf, 'regression') == (m.ffn[1], m.ffn[4], 0, 0, 1)
    m = _model(2, 'ReLU', 0.1)
    assert isinstance(_fusable_head(m.train(), lf, 'regression'), _StackHead)
    assert _predict_head(m.eval()) == (m.ffn[1], m.ffn[4], 0, 0, 1)  # (eval: the dropout is inactive)
    assert isinstance(_fusable_head(_model(2, 'PReLU').train(), lf, 'regression'), _StackHead)
    assert _fusable_head(_model(3, 'PReLU', tasks=65).train(), lf, 'regression') is None
    m = _model(3, 'PReLU')
    m.ffn[2] = m.ffn[5] = torch.nn.PReLU(num_parameters=40).to(DEV)
    assert _fusable_head(m.train(), lf, 'regression') is None and _predict_head(m.eval()) is None


@pytest.mark.gpu
@pytest.mark.parametrize('layers', [1, 3])
@pytest.mark.parametrize('dataset,tasks,C', [('regression', 3, 1), ('classification', 2, 1), ('multiclass', 3, 5)])
def test_head_predict_runs_deeper_heads(layers, dataset, tasks, C):
    """head_predict against the model's torch forward in eval mode (grad enabled: the torch ops) within 1e-5;
    the multiclass no-grad forward IS the stack prediction head."""
    from chemprop_amd.train import _StackHead, _predict_head, head_predict
    b = 9
    m = _model(layers, 'PReLU', 0.1, dataset, tasks, max(C, 2)).eval()
    assert isinstance(_predict_head(m), _StackHead)
    g = BatchMolGraph(synthetic.make_batch('polymer', b, 77), device_bond_features=True)
    ref = m([g]).detach()
    with torch.no_grad():
        emb = m.encoder([g])
        out = head_predict(m, emb)
        fwd = m([g])
    assert out.shape == ref.shape == ((b, tasks, C) if dataset == 'multiclass' else (b, tasks))
    assert golden_io.normwise(out.cpu().numpy(), ref.cpu().numpy()) <= TOL
    if dataset == 'multiclass':
        assert torch.equal(fwd, out)
        assert float((out.sum(dim=2) - 1).abs().max()) <= 1e-6


def _fixture_model(case):
    a = case.args
    a.device = DEV
    m = MoleculeModel(a)
    synthetic.fill_parameters(m, case.seed)
    return m.to(DEV)


@pytest.mark.gpu
def test_reference_three_layer_prelu_model():
    """The reference's own MoleculeModel (ffn_num_layers 3, PReLU, 2 regression tasks): the eval output through
    the model's forward and through head_predict, train_loss and every train_grad/* through head_loss, within
    1e-5 normwise."""
    from chemprop_amd.train import _StackHead, _fusable_head, get_loss_func, head_loss, head_predict
    case = golden_io.load(FIXTURE)
    z = np.load(os.path.join(golden_io.GOLDEN_DIR, FIXTURE + '.npz'), allow_pickle=False)
    m = _fixture_model(case).eval()
    assert len([l for l in m.ffn if isinstance(l, torch.nn.Linear)]) == 3 and type(m.ffn[2]) is torch.nn.PReLU
    out = m(case.graphs, case.features)
    assert out.shape == case.output.shape == (7, 2)
    assert golden_io.normwise(out.detach().cpu().numpy(), case.output) <= TOL
    with torch.no_grad():
        pred = head_predict(m, m.encoder(case.graphs, case.features))
    assert golden_io.normwise(pred.cpu().numpy(), case.output) <= TOL
    targets = [[None if np.isnan(v) else float(v) for v in row] for row in z['targets']]
    assert sum(v is None for r in targets for v in r) >= 2
    m.train()
    head = _fusable_head(m, get_loss_func('regression'), 'regression')
    assert isinstance(head, _StackHead)
    loss = head_loss(m.encoder(case.graphs, case.features), head, targets, list(z['target_weights']),
                     list(z['data_weights']))
    loss.backward()
    ref = float(z['train_loss'])
    got = float(loss.detach())
    print(f'stack head loss {got!r} reference {ref!r}')
    assert golden_io.normwise(got, ref) <= TOL
    names = [k[len('train_grad/'):] for k in z.files if k.startswith('train_grad/')]
    assert sorted(names) == sorted(n for n, q in m.named_parameters() if q.grad is not None)
    assert 'ffn.2.weight' in names
    for n, q in m.named_parameters():
        if q.grad is not None:
            e = golden_io.normwise(q.grad.cpu().numpy(), z['train_grad/' + n])
            assert e <= TOL, (n, e)
