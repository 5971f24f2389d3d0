"""Latent vectors on the GPU: ``wdmpnn_head_stack_latent`` against an fp64 numpy evaluation and, bitwise, against the
``z_l`` of ``wdmpnn_head_stack_predict``; ``wdmpnn_latent_add`` against numpy's own folds; ``model_fingerprint``,
``device_predictions(with_encodings=True)``, ``molecule_fingerprint`` and ``predict_ensemble(embeddings=True)``
against the real reference's numbers (tests/golden/fingerprint/fingerprint_ref.npz, made by
tools/make_fingerprint_golden.py); ``MoleculeModel.fingerprint``'s native path; both CLIs end to end.

The bound on the latent head is the stack head's forward bound of tests/test_head_stack.py (``TOL``, normwise),
which is also the project's bar against the reference's fp32 numbers."""
import csv
import ctypes
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import golden_io
from test_head_stack import TOL
from chemprop_amd import MoleculeModel, _native, cli, synthetic, train
from chemprop_amd.ensemble import predict_ensemble
from chemprop_amd.features import FeatureTable
from chemprop_amd.featurization import BatchMolGraph
from chemprop_amd.fingerprint import LatentAccumulator, model_fingerprint, molecule_fingerprint
from chemprop_amd.graph_io import load_graphs
from chemprop_amd.predict import device_predictions

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
HERE = os.path.dirname(os.path.abspath(__file__))
CSV = os.path.join(HERE, 'data', 'polymer10.csv')
NPZ = os.path.join(HERE, 'data', 'polymer10_graphs.npz')
ACT = {'ReLU': 0, 'LeakyReLU': 1, 'PReLU': 2, 'tanh': 3, 'SELU': 4, 'ELU': 5}
SENTINEL = -12345.678
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946


@pytest.fixture(scope='module')
def ref():
    return dict(np.load(os.path.join(golden_io.GOLDEN_DIR, 'fingerprint', 'fingerprint_ref.npz'), allow_pickle=False))


# ---------------------------------------------------------------------------------------------------
# wdmpnn_head_stack_latent
# ---------------------------------------------------------------------------------------------------
def _act64(act, z, slope):
    if act == 'ReLU':
        return np.maximum(z, 0)
    if act == 'LeakyReLU':
        return np.where(z > 0, z, 0.1 * z)
    if act == 'PReLU':
        return np.where(z > 0, z, slope * z)
    if act == 'tanh':
        return np.tanh(z)
    if act == 'SELU':
        return SELU_SCALE * np.where(z > 0, z, SELU_ALPHA * np.expm1(z))
    return np.where(z > 0, z, np.expm1(z))


# (B, F, Hf, L): one row and partial tiles; two row tiles and three column tiles; the benchmark's width (K below
# one 320-deep stage, 19 column tiles, the last one partial); the deepest stack.  Every activation once.
LATENT_CASES = [((1, 33, 20, 2), 'ReLU', True),
                ((17, 64, 48, 3), 'PReLU', True),
                ((5, 300, 300, 2), 'tanh', True),
                ((3, 40, 16, 6), 'SELU', True),
                ((17, 64, 48, 3), 'LeakyReLU', False),   # no biases
                ((3, 40, 16, 6), 'ELU', True)]


@pytest.mark.parametrize('shape,act,bias', LATENT_CASES)
def test_latent_head_matches_fp64_and_the_prediction_heads_z(shape, act, bias):
    """out = act(z_{L-1}) within TOL normwise of fp64 numpy, with ld_x = F + 3 and ld_out = Hf + 5: the padding
    columns of out and two rows beyond B keep their sentinel.  For L >= 3 the scratch z_1 .. z_{L-2} are bitwise those
    wdmpnn_head_stack_predict leaves for the same inputs; a second call gives identical bits."""
    B, F, Hf, L = shape
    T, ld_x, ld_out = 2, F + 3, Hf + 5
    g = torch.Generator().manual_seed(100 * F + 10 * L + ACT[act])
    xp = torch.full((B, ld_x), 777.0)
    xp[:, :F] = torch.randn(B, F, generator=g)
    widths = [F] + [Hf] * (L - 1) + [T]
    Ws = [(torch.randn(widths[i + 1], widths[i], generator=g) / math.sqrt(widths[i])).to(DEV) for i in range(L)]
    bs = [(0.3 * torch.randn(widths[i + 1], generator=g)).to(DEV) if bias else None for i in range(L)]
    slope = torch.tensor([0.37], device=DEV) if act == 'PReLU' else None   # (not PReLU's default 0.25)
    xp = xp.to(DEV)
    ptr, stream = _native.ptr, _native.current_stream(DEV)
    n_z = (L - 2) * B * Hf

    def latent():
        out = torch.full((B + 2, ld_out), SENTINEL, dtype=torch.float32, device=DEV)
        scratch = torch.full((max(n_z, 4),), float('nan'), dtype=torch.float32, device=DEV)
        h = _native.WdHeadLatent()
        h.x, h.ld_x, h.B, h.F, h.Hf, h.L = ptr(xp), ld_x, B, F, Hf, L
        for i in range(L - 1):   # (the last Linear is not the latent stack's)
            h.W[i], h.b[i] = ptr(Ws[i]), ptr(bs[i])
        h.slope, h.act = ptr(slope), ACT[act]
        h.scratch, h.scratch_bytes, h.out, h.ld_out = ptr(scratch), 4 * n_z, ptr(out), ld_out
        _native.check(_native.lib().wdmpnn_head_stack_latent(ctypes.byref(h), stream), 'head latent')
        return out, scratch

    out, scratch = latent()
    out2, scratch2 = latent()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[B:] == np.float32(SENTINEL)) and np.all(got[:, Hf:] == np.float32(SENTINEL))
    assert torch.equal(out, out2) and torch.equal(scratch[:n_z], scratch2[:n_z])
    f64 = lambda t: 0.0 if t is None else t.cpu().double().numpy()  # noqa: E731
    a = f64(xp)[:, :F]
    for i in range(L - 1):
        a = _act64(act, a @ f64(Ws[i]).T + f64(bs[i]), 0.37)
    err = golden_io.normwise(got[:B, :Hf], a)
    print(f'latent head {shape} {act}: {err:.2e} of fp64')
    assert np.isfinite(got[:B, :Hf]).all() and err <= TOL, err
    if L >= 3:
        q = _native.WdHeadStackPredict()
        pz = torch.full(((L - 1) * B * Hf,), float('nan'), dtype=torch.float32, device=DEV)
        pout = torch.empty((B, T), dtype=torch.float32, device=DEV)
        q.x, q.ld_x, q.B, q.F, q.Hf, q.T, q.L = ptr(xp), ld_x, B, F, Hf, T, L
        for i in range(L):
            q.W[i], q.b[i] = ptr(Ws[i]), ptr(bs[i])
        q.slope, q.act, q.scratch, q.scratch_bytes = ptr(slope), ACT[act], ptr(pz), 4 * pz.numel()
        q.out, q.out_kind, q.n_classes = ptr(pout), 0, 1
        _native.check(_native.lib().wdmpnn_head_stack_predict(ctypes.byref(q), stream), 'head stack predict')
        torch.cuda.synchronize()
        assert torch.isfinite(scratch[:n_z]).all() and torch.equal(scratch[:n_z], pz[:n_z])
        # and the latent vector is the activation of the prediction head's last z plane
        last = _act64(act, pz[n_z:].cpu().double().numpy().reshape(B, Hf), 0.37)
        assert golden_io.normwise(got[:B, :Hf], last) <= TOL


# ---------------------------------------------------------------------------------------------------
# wdmpnn_latent_add
# ---------------------------------------------------------------------------------------------------
ROWS, ROW_BLOCKS = 9, ((0, 4), (4, 3))   # (rows 7 and 8 are never covered)


@pytest.mark.parametrize('M', [1, 2, 5])
@pytest.mark.parametrize('W', [3, 7])
@pytest.mark.parametrize('c0', [0, 2])
def test_latent_add_is_numpys_fold(M, W, c0):
    """cols = (double)v at the [N][W][M] offsets, sum = the sequential np.float32 accumulation in model order, both
    bitwise; a NaN stays in its cell; rows and columns outside the blocks keep their sentinel (ld_src = c0 + W + 2,
    ld_sum = W + 2)."""
    rng = np.random.default_rng(100 * M + 10 * W + c0)
    ld_src, ld_sum = c0 + W + 2, W + 2
    src = (rng.standard_normal((M, ROWS, ld_src)) * 10.0 ** rng.integers(-3, 4, (M, ROWS, ld_src))).astype(np.float32)
    src[M - 1, 1, c0 + 1] = np.nan
    cols = torch.full((ROWS, W, M), SENTINEL, dtype=torch.float64, device=DEV)
    acc = torch.full((ROWS, ld_sum), SENTINEL, dtype=torch.float32, device=DEV)
    for k in range(M):
        for row0, B in ROW_BLOCKS:
            v = torch.from_numpy(np.ascontiguousarray(src[k, row0:row0 + B])).to(DEV)
            e = _native.WdLatentAdd()
            e.src, e.ld_src, e.B, e.W, e.c0, e.M, e.k, e.row0 = v.data_ptr(), ld_src, B, W, c0, M, k, row0
            e.cols, e.sum, e.ld_sum = cols.data_ptr(), acc.data_ptr(), ld_sum
            _native.check(_native.lib().wdmpnn_latent_add(ctypes.byref(e), _native.current_stream(DEV)), 'latent add')
    torch.cuda.synchronize()
    used = src[:, :7, c0:c0 + W]
    want_cols = np.full((ROWS, W, M), SENTINEL)
    want_cols[:7] = np.transpose(used, (1, 2, 0)).astype(np.float64)
    want_sum = np.full((ROWS, ld_sum), SENTINEL, dtype=np.float32)
    s = used[0].copy()
    for k in range(1, M):
        s += used[k]
    assert s.dtype == np.float32
    want_sum[:7, :W] = s
    got_cols, got_sum = cols.cpu().numpy(), acc.cpu().numpy()
    nan = np.isnan(got_sum)   # (the NaN alone in its cell; every other cell bit for bit)
    assert nan.sum() == 1 and nan[1, 1] and np.isnan(got_cols).sum() == 1 and np.isnan(got_cols[1, 1, M - 1])
    assert np.isnan(want_sum[1, 1]) and np.isnan(want_cols[1, 1, M - 1])
    got_cols[1, 1, M - 1] = want_cols[1, 1, M - 1] = got_sum[1, 1] = want_sum[1, 1] = 0
    assert np.array_equal(got_cols.view(np.int64), want_cols.view(np.int64))
    assert np.array_equal(got_sum.view(np.int32), want_sum.view(np.int32))


@pytest.mark.parametrize('M', [1, 2, 5])
def test_latent_accumulator_columns_and_mean32(M):
    """The class over the kernel: columns() and mean32() bitwise numpy's ``[N][W][M]`` fill and ``sum / M`` on fp32;
    one set of buffers without the other."""
    N, W, c0 = 7, 5, 2
    rng = np.random.default_rng(M)
    src = rng.standard_normal((M, N, c0 + W + 1)).astype(np.float32)
    both = LatentAccumulator(N, W, DEV, n_models=M, running_sum=True, c0=c0)
    only_sum = LatentAccumulator(N, W, DEV, n_models=M, columns=False, running_sum=True, c0=c0)
    for k in range(M):
        for row0, B in ((0, 4), (4, 3)):
            v = torch.from_numpy(np.ascontiguousarray(src[k, row0:row0 + B])).to(DEV)
            both.add(v, row0, k)
            only_sum.add(v, row0, k)
        if k < M - 1:
            with pytest.raises(ValueError):
                both.columns()                                        # unfinished
    used = src[:, :, c0:c0 + W]
    block = np.zeros((N, W, M))
    s = None
    for k in range(M):
        block[:, :, k] = used[k]
        s = used[k].copy() if s is None else s + used[k]
    mean = s / M
    assert mean.dtype == np.float32
    assert both.columns().dtype == torch.float64 and np.array_equal(both.columns().cpu().numpy(), block)
    for acc in (both, only_sum):
        got = acc.mean32()
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), mean.view(np.int32))


# ---------------------------------------------------------------------------------------------------
# against the reference
# ---------------------------------------------------------------------------------------------------
FIXTURES = ['model_polymer_regression', 'head_stack/model_polymer_ffn3_prelu', 'model_two_mols_features_cls']


def _fixture(name):
    case = golden_io.load(name)
    a = case.args
    a.device = DEV
    m = MoleculeModel(a)
    synthetic.fill_parameters(m, case.seed)
    m = m.to(DEV).eval()
    batches = [case.graphs[0] if len(case.graphs) == 1 else case.graphs]
    table = None if case.features is None else FeatureTable(np.stack(case.features), DEV)
    return m, batches, table


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_models_match_the_reference(ref, name):
    """model_fingerprint for both types and the embeddings of device_predictions(with_encodings=True) within TOL
    normwise of the reference's; the predictions next to the embeddings bitwise those of the plain call."""
    m, batches, table = _fixture(name)
    key = name.split('/')[-1]
    for t in ('MPN', 'last_FFN'):
        got = model_fingerprint(m, batches, t, table)
        want = ref[f'{key}/{t}']
        assert got.dtype == torch.float32 and got.device == DEV and tuple(got.shape) == want.shape
        err = golden_io.normwise(got.cpu().numpy(), want)
        print(f'{key} {t}: {err:.2e}')
        assert err <= TOL, (t, err)
    plain = list(device_predictions(m, batches, table))
    both = list(device_predictions(m, batches, table, with_encodings=True))
    assert len(plain) == len(both) == 1 and len(plain[0]) == 2 and len(both[0]) == 3
    assert plain[0][0] == both[0][0] == 0 and torch.equal(plain[0][1], both[0][1])
    want = ref[f'{key}/embeddings']
    assert tuple(both[0][2].shape) == want.shape
    assert golden_io.normwise(both[0][2].cpu().numpy(), want) <= TOL
    assert torch.equal(both[0][2], model_fingerprint(m, batches, 'MPN', table))


def test_device_predictions_latent_refusals():
    m, batches, table = _fixture('model_polymer_regression')
    with pytest.raises(ValueError):
        list(device_predictions(m, batches, table, latent='first_FFN'))
    with pytest.raises(ValueError):
        list(device_predictions(m, batches, table, latent='MPN', with_encodings=True))
    one = MoleculeModel(types.SimpleNamespace(**{**vars(golden_io.load('model_polymer_regression').args),
                                                 'ffn_num_layers': 1, 'device': DEV})).to(DEV).eval()
    with pytest.raises(ValueError, match='ffn_num_layers of 1'):
        model_fingerprint(one, batches, 'last_FFN')
    with pytest.raises(ValueError, match='ffn_num_layers of 1'):
        train.head_latent(one, torch.zeros(2, 64, device=DEV))
    assert tuple(model_fingerprint(one, batches, 'MPN').shape) == (5, 64)
    m.train()
    with pytest.raises(ValueError):
        train.head_latent(m, torch.zeros(2, 64, device=DEV))


@pytest.fixture(scope='module')
def ensemble(ref):
    """The fixture's two-model ensemble: polymer graphs, three input features, ffn_num_layers 2, two parameter
    seeds."""
    cfg = json.loads(str(ref['ensemble/config']))
    kind, B, seed = json.loads(str(ref['ensemble/graphs']))
    mols = synthetic.make_batch(kind, B, seed)
    models = []
    for pseed in ref['ensemble/param_seeds'].tolist():
        m = MoleculeModel(types.SimpleNamespace(**cfg, device=DEV))
        synthetic.fill_parameters(m, int(pseed))
        models.append(m.to(DEV).eval())
    return types.SimpleNamespace(cfg=cfg, mols=mols, models=models, feats=ref['ensemble/features'],
                                 items=[(m, None, None) for m in models])


def test_two_model_ensemble_matches_the_reference(ref, ensemble):
    """molecule_fingerprint's [N][fp][M] blocks and predict_ensemble's fp32 mean embeddings within TOL normwise of
    the reference's, in batches of 4 (two batches, the second short); the fold of our own per-model vectors is
    bitwise numpy's; MPN drops the feature columns, with or without the features given."""
    e = ensemble
    N, H, Hf, Ff = len(e.mols), e.cfg['hidden_size'], e.cfg['ffn_hidden_size'], e.cfg['features_size']
    batches = [BatchMolGraph(e.mols[s:s + 4]) for s in range(0, N, 4)]
    table = FeatureTable(e.feats, DEV)
    for t, fp in (('MPN', H), ('last_FFN', Hf)):
        got = molecule_fingerprint(e.items, e.mols, 4, t, features=e.feats, device=DEV)
        want = ref[f'ensemble/{t}_block']
        assert got.dtype == np.float64 and got.shape == want.shape == (N, fp, 2)
        err = golden_io.normwise(got, want)
        print(f'ensemble {t} block: {err:.2e}')
        assert err <= TOL, (t, err)
        block = np.zeros((N, fp, 2))
        for k, m in enumerate(e.models):
            own = model_fingerprint(m, batches, t, table).cpu().numpy()
            assert own.shape == (N, H + Ff if t == 'MPN' else Hf)
            assert golden_io.normwise(own, ref[f'ensemble/m{k}/{t}']) <= TOL
            block[:, :, k] = own[:, :fp]
        assert np.array_equal(got, block)
        if t == 'MPN':  # the encoders alone: no features needed, the same bits
            assert np.array_equal(molecule_fingerprint(e.items, e.mols, 4, 'MPN', device=DEV), got)
        else:
            with pytest.raises(ValueError):
                molecule_fingerprint(e.items, e.mols, 4, 'last_FFN', device=DEV)
    plain = predict_ensemble(e.items, e.mols, 4, features=e.feats, device=DEV)
    mean, spread, individual, emb = predict_ensemble(e.items, e.mols, 4, features=e.feats, device=DEV, embeddings=True)
    assert len(plain) == 3 and np.array_equal(plain[0], mean) and spread is None and individual is None
    want = ref['ensemble/mean_embeddings']
    assert emb.dtype == np.float32 and emb.shape == want.shape == (N, H + Ff)
    err = golden_io.normwise(emb, want)
    print(f'ensemble mean embeddings: {err:.2e}')
    assert err <= TOL, err
    total = None
    for k, m in enumerate(e.models):
        x = torch.cat([x for _, _, x in device_predictions(m, batches, table, with_encodings=True)]).cpu().numpy()
        assert golden_io.normwise(x, ref[f'ensemble/m{k}/embeddings']) <= TOL
        if total is None:
            total = x.copy()
        else:
            total += x
    own_mean = total / len(e.models)
    assert own_mean.dtype == np.float32 and np.array_equal(emb.view(np.int32), own_mean.view(np.int32))


def test_model_fingerprint_takes_the_native_latent_head(monkeypatch):
    """MoleculeModel.fingerprint('last_FFN') in eval mode under no_grad runs train.head_latent; with gradients
    enabled it runs the torch slice; the two agree within TOL normwise (both fp32 evaluations of one formula)."""
    m, batches, _ = _fixture('head_stack/model_polymer_ffn3_prelu')
    calls = []
    real = train.head_latent

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(train, 'head_latent', counting)
    with torch.no_grad():
        native = m.fingerprint(batches[:1], fingerprint_type='last_FFN')
    assert len(calls) == 1 and not native.requires_grad
    with torch.enable_grad():
        sliced = m.fingerprint(batches[:1], fingerprint_type='last_FFN')
    assert len(calls) == 1 and sliced.requires_grad
    assert native.shape == sliced.shape == (7, 48)
    err = golden_io.normwise(native.cpu().numpy(), sliced.detach().cpu().numpy())
    print(f'native last_FFN vs the torch slice: {err:.2e}')
    assert err <= TOL, err
    m.train()
    with torch.no_grad():
        m.fingerprint(batches[:1], fingerprint_type='last_FFN')
    assert len(calls) == 1                                             # training mode: the torch slice


# ---------------------------------------------------------------------------------------------------
# chemprop_fingerprint and chemprop_predict --save_graph_embeddings end to end
# ---------------------------------------------------------------------------------------------------
def _read(path):
    with open(path) as f:
        return list(csv.reader(f))


def test_fingerprint_and_embeddings_cli_end_to_end(tmp_path):
    d = tmp_path / 'e'
    cli.chemprop_train(['--data_path', CSV, '--graphs_path', NPZ, '--polymer', '--epochs', '1', '--warmup_epochs',
                        '0.5', '--batch_size', '4', '--hidden_size', '32', '--ensemble_size', '2', '--save_dir', str(d)])
    ckpts = [str(d / f'model_{k}' / 'best_model.pt') for k in range(2)]
    graphs = load_graphs(NPZ)
    first, smiles = _read(CSV)[0][0], [r[0] for r in _read(CSV)[1:]]
    common = ['--test_path', CSV, '--graphs_path', NPZ, '--batch_size', '4']
    fps = {}
    for t in ('MPN', 'last_FFN'):
        out = str(tmp_path / 'fp' / f'{t}.csv')
        fp = fps[t] = cli.chemprop_fingerprint(common + ['--preds_path', out, '--checkpoint_dir', str(d), '--fingerprint_type', t])
        assert fp.dtype == np.float64 and fp.shape == (10, 32, 2)
        assert np.array_equal(fp, molecule_fingerprint(ckpts, graphs, 4, t, device=DEV))
        assert not np.array_equal(fp[:, :, 0], fp[:, :, 1])
        rows = _read(out)
        assert rows[0] == [first] + [f'fp_{j}_model_{i}' for j in range(32) for i in range(2)]
        assert [r[0] for r in rows[1:]] == smiles
        assert np.array_equal(np.array([[float(c) for c in r[1:]] for r in rows[1:]]).reshape(10, 32, 2), fp)
    one = str(tmp_path / 'one.csv')   # one model, the default type
    fp1 = cli.chemprop_fingerprint(common + ['--preds_path', one, '--checkpoint_path', ckpts[1]])
    assert fp1.shape == (10, 32, 1) and np.array_equal(fp1[:, :, 0], fps['MPN'][:, :, 1])
    assert not np.array_equal(fps['MPN'], fps['last_FFN'])
    assert _read(one)[0] == [first] + [f'fp_{j}' for j in range(32)]
    assert np.array_equal(fp1, molecule_fingerprint(ckpts[1:], graphs, 4, 'MPN', device=DEV))
    # chemprop_predict: the embeddings next to an unchanged predictions CSV
    plain, with_emb, npy = str(tmp_path / 'p.csv'), str(tmp_path / 'q.csv'), str(tmp_path / 'emb' / 'g.npy')
    cli.chemprop_predict(common + ['--preds_path', plain, '--checkpoint_paths'] + ckpts)
    cli.chemprop_predict(common + ['--preds_path', with_emb, '--checkpoint_paths'] + ckpts +
                         ['--save_graph_embeddings', '--graph_embeddings_path', npy])
    assert open(plain, 'rb').read() == open(with_emb, 'rb').read()
    emb = np.load(npy)
    assert emb.dtype == np.float32 and emb.shape == (10, 32)
    want = predict_ensemble(ckpts, graphs, 4, device=DEV, embeddings=True)[3]
    assert np.array_equal(emb.view(np.int32), want.view(np.int32))
    # the mean embedding is the fp32 mean of the two models' MPN fingerprints
    both = molecule_fingerprint(ckpts, graphs, 4, 'MPN', device=DEV).astype(np.float32)
    assert np.array_equal(emb, (both[:, :, 0] + both[:, :, 1]) / 2)
    with pytest.raises(ValueError):
        cli.chemprop_predict(common + ['--preds_path', plain, '--checkpoint_paths'] + ckpts + ['--save_graph_embeddings'])
