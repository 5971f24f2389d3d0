"""Molecule features natively, on the GPU: the join / gather / split kernel (``wdmpnn_join_rows``) against torch
indexing and ``torch.cat``, bit for bit; the direct training step of models with input features against the
autograd step fed a list of numpy rows (the path every such model took before); frozen encoders and cached
encodings; inference; ``chemprop_train --features_path`` end to end.

Every row index a kernel sees here is inside its table: the raw kernel calls assert it on the host, everything
else goes through ``FeatureTable.index``."""
import csv
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import FeatureTable, TrainArgs, _native, cli, polymer, synthetic
from chemprop_amd import train as T
from chemprop_amd.featurization import BatchMolGraph
from chemprop_amd.graph_io import load_graphs, save_graphs
from chemprop_amd.model import MoleculeModel
from chemprop_amd.nn_utils import initialize_weights

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


# ---------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _rand(rows, cols, seed):
    return torch.randn((rows, cols), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _join(B, segs, pad=0, sentinel=None):
    """One wdmpnn_join_rows call.  ``segs``: (source [rows][ld] on the GPU, c0, w, index list or None).  Returns
    (out [B][sum w + pad], the same from torch indexing and torch.cat)."""
    j = _native.WdJoin()
    j.B, j.n_seg = B, len(segs)
    keep, want = [], []
    for k, (src, c0, w, idx) in enumerate(segs):
        assert src.is_contiguous() and src.dtype == torch.float32 and 0 <= c0 and c0 + w <= src.shape[1]
        g = j.seg[k]
        g.src, g.ld, g.c0, g.w = src.data_ptr(), src.shape[1], c0, w
        if idx is None:
            assert src.shape[0] >= B
            rows = src[:B]
        else:
            assert len(idx) == B and all(0 <= i < src.shape[0] for i in idx)  # (the kernel clamps nothing)
            it = torch.tensor(idx, dtype=torch.int64, device=DEV)
            keep.append(it)
            g.idx = it.data_ptr()
            rows = src[it]
        want.append(rows[:, c0:c0 + w])
    width = sum(s[2] for s in segs)
    out = torch.full((B, width + pad), float('nan') if sentinel is None else sentinel, dtype=torch.float32, device=DEV)
    j.out, j.ld_out = out.data_ptr(), width + pad
    _native.check(_native.lib().wdmpnn_join_rows(ctypes.byref(j), _native.current_stream(DEV)), 'join rows')
    torch.cuda.synchronize()
    return out, torch.cat(want, dim=1)


def _same(out, want):
    return torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize('B', [5, 1, 300])
def test_join_scalar_and_vector_paths(B):
    """(a) [emb 48 | table[idx] columns 1..5 of 8] -> ld_out 53: nothing is 16-byte aligned past row 0, the scalar
    path; (b) [emb 48 | table[idx] 16 of 16] -> ld_out 64: both segments on the vector path; (d) one row, and 300
    rows (more than one 256-thread block on either path)."""
    idx = [6, 0, 0, 3, 6] if B == 5 else [(7 * i + 3) % 7 for i in range(B)]
    emb = _rand(B, 48, 1)
    out, want = _join(B, [(emb, 0, 48, None), (_rand(7, 8, 2), 1, 5, idx)])
    assert out.shape == (B, 53) and _same(out, want)
    out, want = _join(B, [(emb, 0, 48, None), (_rand(7, 16, 3), 0, 16, idx)])
    assert out.shape == (B, 64) and _same(out, want)
    # gather: one segment with an index
    out, want = _join(B, [(_rand(7, 16, 4), 0, 16, idx)])
    assert _same(out, want)
    out, want = _join(B, [(_rand(7, 5, 5), 0, 5, idx)])
    assert _same(out, want)


@pytest.mark.parametrize('B', [5, 300])
def test_split_makes_a_column_range_contiguous(B):
    """(c) source [B][53]: columns 0..48 (dEmb = dx[:, 0:H]) and columns 3..8; and from an aligned source."""
    src = _rand(B, 53, 6)
    for c0, w in ((0, 48), (3, 5)):
        out, want = _join(B, [(src, c0, w, None)])
        assert out.shape == (B, w) and out.is_contiguous() and _same(out, want) and _same(out, src[:, c0:c0 + w])
    src = _rand(B, 64, 7)
    for c0, w in ((0, 48), (16, 48), (4, 6), (2, 8)):
        out, want = _join(B, [(src, c0, w, None)])
        assert _same(out, want)
    assert _same(T.split_columns(src, 0, 48), src[:, :48])


def test_four_segments_in_one_call():
    """(e) four segments; with ld_out 20 the segments take: the vector path (8), the vector path from column 4 of
    12 (4, gathered), the vector path with a two-word tail (6), the scalar path (destination offset 18)."""
    B = 37
    idx = [(5 * i + 1) % 9 for i in range(B)]
    segs = [(_rand(B, 8, 8), 0, 8, None), (_rand(9, 12, 9), 4, 4, idx), (_rand(B, 8, 10), 0, 6, None),
            (_rand(9, 3, 11), 1, 2, idx)]
    out, want = _join(B, segs)
    assert out.shape == (B, 20) and _same(out, want)
    out, want = _join(B, segs[1:] + segs[:1])  # (another order: other offsets, other paths)
    assert _same(out, want)
    out, want = _join(B, [(s[0], s[1], s[2], None if s[3] is None else idx[::-1]) for s in segs[::-1]])
    assert _same(out, want)


@pytest.mark.parametrize('width', [(48, 5), (48, 16)])
def test_columns_beyond_the_segments_are_not_written(width):
    """(f) ld_out = sum w + 3, prefilled with a sentinel."""
    B = 70
    idx = [(3 * i) % 7 for i in range(B)]
    out, want = _join(B, [(_rand(B, width[0], 12), 0, width[0], None), (_rand(7, 16, 13), 0, width[1], idx)], pad=3,
                      sentinel=-77.25)
    n = sum(width)
    assert _same(out[:, :n], want)
    assert bool((out[:, n:] == -77.25).all())


@pytest.mark.parametrize('ld', [16, 5])
def test_every_payload_bit_survives(ld):
    """(g) quiet and signalling NaNs with payloads, both infinities, -0.0 and denormals, on both paths."""
    pats = [0x7fc00001, -0x3edcbb, 0x7f800001, -0x7fffff, 0x7f800000, -0x800000, -0x80000000, 1, -0x7fffffff,
            0x7fffffff, 0x3f800000]
    n = 7 * ld
    raw = torch.tensor([pats[i % len(pats)] for i in range(n)], dtype=torch.int32).view(7, ld)
    table = raw.to(DEV).view(torch.float32)
    emb = torch.tensor([pats[(3 * i) % len(pats)] for i in range(5 * 48)], dtype=torch.int32).view(5, 48).to(DEV)
    emb = emb.view(torch.float32)
    idx = [6, 0, 0, 3, 6]
    out, _ = _join(5, [(emb, 0, 48, None), (table, 0, ld, idx)])
    want = torch.cat([emb.view(torch.int32), raw.to(DEV)[torch.tensor(idx, device=DEV)]], dim=1)
    assert torch.equal(out.view(torch.int32), want)
    assert bool(torch.isnan(out).any()) and bool(torch.isinf(out).any())


def test_feature_rows_gather_and_join():
    a = np.random.default_rng(0).standard_normal((7, 5)) * 100
    table = FeatureTable(a, DEV)
    assert torch.equal(table.data.cpu(), torch.from_numpy(a).float())
    idx = table.index([6, 0, 0, 3, 6, 1])
    rows = idx[1:5]
    want = torch.from_numpy(a[[0, 0, 3, 6]]).float().to(DEV)
    assert torch.equal(rows.to_tensor(), want)
    emb = _rand(4, 48, 20)
    assert torch.equal(T.join_features(emb, rows), torch.cat([emb, want], dim=1))
    assert torch.equal(T.join_features(emb, want), torch.cat([emb, want], dim=1))
    assert T.join_features(emb[:0], idx[2:2]).shape == (0, 53)
    with pytest.raises(ValueError):
        T.join_features(emb, idx[0:3])
    with pytest.raises(ValueError):
        table.index([7])


# ---------------------------------------------------------------------------------------------------
# the training step
# ---------------------------------------------------------------------------------------------------
B_STEP = 12
STEP_MOLS = [synthetic.make_batch('polymer', B_STEP, 30 + i) for i in range(3)]


def _feature_rows(ff, seed=11):
    return np.random.default_rng(seed).standard_normal((3 * B_STEP, ff))


def _targets(dataset, i, tasks):
    rng = np.random.default_rng(50 + i)
    if dataset == 'spectra':
        t = rng.random((B_STEP, tasks)) + 0.05
        t /= t.sum(axis=1, keepdims=True)
        rows = t.tolist()
        rows[1][4] = None
        return rows

    def one():
        if rng.random() < 0.15:
            return None
        if dataset == 'regression':
            return float(rng.normal())
        return float(rng.random() < 0.5) if dataset == 'classification' else float(rng.integers(3))
    return [[one() for _ in range(tasks)] for _ in range(B_STEP)]


def _model(ff, dataset='regression', tasks=2, freeze=False, **kw):
    args = TrainArgs(hidden_size=48, depth=3, device=DEV, dataset_type=dataset, num_tasks=tasks,
                     multiclass_num_classes=3, use_input_features=True, features_size=ff, **kw)
    torch.manual_seed(0)
    m = MoleculeModel(args)
    initialize_weights(m)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.PReLU):
                mod.weight.fill_(0.25)
    if freeze:
        cli.apply_freezing(m, frzn_encoder=True, frzn_ffn_layers=0)
    return m.to(DEV).train()


def _steps(m, dataset, tasks, feats, mode, use_bucket=False, counts=None, encodings=None):
    """2 x 3 steps.  mode 'direct' (device rows: the new path), 'tensor' (the same with a device tensor),
    'autograd' (list of numpy rows, fused head: the oracle), 'torch' (list of numpy rows, torch ops)."""
    from chemprop_amd.dp import GradBucket
    lf = T.get_loss_func(dataset)
    opt = T.build_optimizer(m, 1e-3)
    bucket = GradBucket(m) if use_bucket else None
    table = FeatureTable(feats, DEV)
    losses = []
    for _ in range(2):
        index = table.index(range(3 * B_STEP))
        for i in range(3):
            s = slice(B_STEP * i, B_STEP * (i + 1))
            if mode == 'direct':
                f = index[s]
            elif mode == 'tensor':
                f = torch.from_numpy(feats[s]).float().to(DEV)
            else:
                f = [feats[k] for k in range(s.start, s.stop)]
            kw = dict(encodings=encodings[s]) if encodings is not None else {}
            before = {k: counts[k] for k in ('direct', 'join')} if counts is not None else None
            losses.append(float(T.train_step(m, None if encodings is not None else [BatchMolGraph(STEP_MOLS[i])],
                                             _targets(dataset, i, tasks), lf, opt, dataset_type=dataset,
                                             features_batch=f, bucket=bucket, fused_head=mode != 'torch',
                                             direct=mode in ('direct', 'tensor'), **kw)))
            if counts is not None:
                counts.setdefault('per_step', []).append({k: counts[k] - before[k] for k in before})
    assert all(math.isfinite(v) for v in losses)
    return losses, {k: v.detach().clone() for k, v in m.named_parameters()}, \
        {k: (None if v.grad is None else v.grad.clone()) for k, v in m.named_parameters()}


@pytest.fixture
def counts(monkeypatch):
    """Calls of train._direct_step and of the join entry point."""
    c = {'direct': 0, 'join': 0}
    real_step, real_join = T._direct_step, _native.join_rows

    def step(*a, **kw):
        c['direct'] += 1
        return real_step(*a, **kw)

    def join(*a, **kw):
        c['join'] += 1
        return real_join(*a, **kw)
    monkeypatch.setattr(T, '_direct_step', step)
    monkeypatch.setattr(_native, 'join_rows', join)
    return c


def _assert_bitwise(got, ref):
    assert got[0] == ref[0]
    for k in ref[1]:
        assert torch.equal(got[1][k], ref[1][k]), k
    for k in ref[2]:
        assert (got[2][k] is None) == (ref[2][k] is None), k
        assert got[2][k] is None or torch.equal(got[2][k], ref[2][k]), k


CASES = {'regression': dict(dataset='regression'),
         'bucket': dict(dataset='regression', use_bucket=True),
         'classification': dict(dataset='classification'),
         'multiclass': dict(dataset='multiclass'),
         'prelu3_dropout': dict(dataset='regression', activation='PReLU', ffn_num_layers=3, dropout=0.2, bias=True)}


@pytest.mark.parametrize('ff', [5, 16])
@pytest.mark.parametrize('case', list(CASES))
def test_direct_step_with_features_equals_the_autograd_step(case, ff, counts):
    """The direct step on device rows gives, bitwise, the losses, parameters and gradients of the autograd step
    on a list of numpy rows (the fused head under autograd, ``torch.cat`` and its backward), over 2 x 3 steps;
    every such step is a ``_direct_step`` with two join launches (x, and the encoder's slice of dx)."""
    kw = dict(CASES[case])
    dataset, use_bucket = kw.pop('dataset'), kw.pop('use_bucket', False)
    feats = _feature_rows(ff)
    res = {}
    for mode in ('direct', 'autograd'):
        counts['direct'] = counts['join'] = 0
        m = _model(ff, dataset, **kw)
        assert m.ffn[1].in_features == 48 + ff
        torch.manual_seed(1)  # (the dropout seeds of the steps)
        res[mode] = _steps(m, dataset, 2, feats, mode, use_bucket, counts if mode == 'direct' else None)
        if mode == 'direct':
            assert counts['direct'] == 6
            assert counts.pop('per_step') == [{'direct': 1, 'join': 2}] * 6
        else:
            assert counts['direct'] == 0
    _assert_bitwise(res['direct'], res['autograd'])
    assert len(set(res['direct'][0])) == 6


def test_a_device_tensor_of_features_takes_the_direct_step_too(counts):
    feats = _feature_rows(5)
    got = _steps(_model(5), 'regression', 2, feats, 'tensor', counts=counts)
    assert counts['direct'] == 6 and counts['join'] == 12
    counts['direct'] = 0
    ref = _steps(_model(5), 'regression', 2, feats, 'autograd')
    assert counts['direct'] == 0
    _assert_bitwise(got, ref)


@pytest.mark.parametrize('dataset', ['regression', 'classification'])
def test_direct_step_with_features_against_the_torch_ops(dataset):
    """The tolerances of test_classification_steps_take_the_fused_direct_path: losses within 1e-5 (relative),
    parameters within 1e-4 normwise of the reference's torch ops on a list of rows."""
    feats = _feature_rows(5)
    got = _steps(_model(5, dataset), dataset, 2, feats, 'direct')
    ref = _steps(_model(5, dataset), dataset, 2, feats, 'torch')
    for a, b in zip(got[0], ref[0]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (a, b)
    for k in ref[1]:
        e = golden_io.normwise(got[1][k].cpu().numpy(), ref[1][k].cpu().numpy())
        assert e <= 1e-4, (k, e)


def test_spectra_model_with_phase_features_takes_the_direct_step(counts):
    """T = 33 and 2 one-hot phase features (the usual spectra model): direct step == autograd step, bitwise."""
    phases = np.eye(2)[np.arange(3 * B_STEP) % 2]
    res = {}
    for mode in ('direct', 'autograd'):
        counts['direct'] = 0
        m = _model(2, 'spectra', tasks=33)
        assert m.ffn[1].in_features == 50 and m.ffn[4].out_features == 33
        res[mode] = _steps(m, 'spectra', 33, phases, mode)
        assert counts['direct'] == (6 if mode == 'direct' else 0)
    _assert_bitwise(res['direct'], res['autograd'])


@pytest.mark.parametrize('ff', [5, 16])
def test_frozen_encoder_with_features(ff, counts):
    """A frozen encoder: the direct step on device rows (one join launch: there is no dx to split) and the step
    from cached encodings are bitwise the autograd step on a list of rows; frozen parameters end every step
    without a gradient."""
    feats = _feature_rows(ff)
    ref = _steps(_model(ff, freeze=True), 'regression', 2, feats, 'autograd')
    assert counts['direct'] == 0
    m = _model(ff, freeze=True)
    counts['join'] = 0
    got = _steps(m, 'regression', 2, feats, 'direct', counts=counts)
    assert counts['direct'] == 6 and counts['join'] == 6
    _assert_bitwise(got, ref)
    frozen = [k for k, q in m.named_parameters() if not q.requires_grad]
    assert any(k.startswith('encoder.') for k in frozen)
    assert all(got[2][k] is None for k in frozen)
    assert all(got[2][k] is not None for k, q in m.named_parameters() if q.requires_grad)
    # the same steps from cached encodings
    m = _model(ff, freeze=True)
    rows = T.frozen_encodings(m, [g for mols in STEP_MOLS for g in mols], B_STEP)
    assert rows.shape == (3 * B_STEP, 48)
    counts['direct'] = counts['join'] = 0
    cached = _steps(m, 'regression', 2, feats, 'direct', counts=counts, encodings=rows)
    assert counts['direct'] == 6 and counts['join'] == 6
    _assert_bitwise(cached, ref)
    with pytest.raises(ValueError, match='encodings'):  # (the widths must add up to the FFN's input)
        T.train_step(m, None, _targets('regression', 0, 2), T.get_loss_func('regression'), T.build_optimizer(m, 1e-3),
                     encodings=rows[:B_STEP], features_batch=FeatureTable(_feature_rows(ff + 1), DEV).rows(range(B_STEP)))


def test_inference_with_feature_rows(counts):
    feats = _feature_rows(5)
    m = _model(5).eval()
    g = BatchMolGraph(STEP_MOLS[0])
    rows = FeatureTable(feats, DEV).rows(range(B_STEP))
    as_list = [feats[k] for k in range(B_STEP)]
    with torch.no_grad():
        want = m([g], as_list)
        counts['join'] = 0
        got = m([g], rows)
        assert counts['join'] == 1  # (the whole of [encoding | rows]: one launch)
        assert torch.equal(got, want)
        assert torch.equal(m([g], rows.to_tensor()), want)
        assert torch.equal(m.encoder([g], rows), m.encoder([g], as_list))
    out = m([g], rows)  # gradients on: the gather, then torch.cat under autograd
    assert out.requires_grad and torch.equal(out.detach(), want)
    assert torch.equal(m([g], as_list).detach(), want)


# ---------------------------------------------------------------------------------------------------
# chemprop_train --features_path
# ---------------------------------------------------------------------------------------------------
def _write(path, rows):
    with open(path, 'w', newline='') as f:
        csv.writer(f).writerows(rows)


def _cli_data(tmp_path, n=16):
    rng = np.random.default_rng(4)
    rows, graphs = [], []
    for k in range(n):
        fa = float(rng.choice([0.25, 0.5, 0.75]))
        s = f'[*:1]c1ccc([*:2])cc1.[*:3]CC[*:4]|{fa}|{1 - fa}|<1-3:0.5:0.5<2-4:0.5:0.5<1-2:0.5:0.5~{10:g}'
        rows.append([s, f'{2 * fa + 0.1 * rng.normal():.6g}'])
        graphs.append(polymer.synthetic_polymer_graph(s, seed=k))
    feats = rng.standard_normal((n, 3)) * np.array([3.0, 1.0, 10.0]) + np.array([1.0, 0.0, -5.0])
    feats[:, 1] = 2.5
    feats[3, 2] = np.nan
    paths = {k: str(tmp_path / v) for k, v in (('csv', 'd.csv'), ('npz', 'd.npz'), ('feat', 'f.csv'))}
    _write(paths['csv'], [['smiles', 'y']] + rows)
    save_graphs(paths['npz'], graphs)
    _write(paths['feat'], [['f0', 'f1', 'f2']] + [['nan' if np.isnan(v) else repr(float(v)) for v in r] for r in feats])
    return paths, feats


def test_chemprop_train_with_a_features_file(tmp_path, monkeypatch):
    paths, feats = _cli_data(tmp_path)
    seen = {'steps': 0, 'direct': 0, 'cached': 0, 'encodings': 0}
    real_step, real_direct, real_enc = cli.train_step, T._direct_step, cli.frozen_encodings

    def step(*a, **kw):
        seen['steps'] += 1
        return real_step(*a, **kw)

    def direct(*a, **kw):
        seen['direct'] += 1
        enc = kw.get('encodings', a[9] if len(a) > 9 else None)
        seen['cached'] += enc is not None
        return real_direct(*a, **kw)

    def encodings(*a, **kw):
        seen['encodings'] += 1
        return real_enc(*a, **kw)
    monkeypatch.setattr(cli, 'train_step', step)
    monkeypatch.setattr(T, '_direct_step', direct)
    monkeypatch.setattr(cli, 'frozen_encodings', encodings)
    argv = ['--data_path', paths['csv'], '--graphs_path', paths['npz'], '--polymer', '--epochs', '2',
            '--warmup_epochs', '1', '--batch_size', '4', '--hidden_size', '48', '--features_path', paths['feat'],
            '--save_dir']
    d = tmp_path / 'a'
    scores = cli.chemprop_train(argv + [str(d)])
    assert math.isfinite(scores['rmse'][0])
    split = json.load(open(d / 'split_indices.json'))
    assert len(split['train']) == 12 and len(split['test']) == 2
    assert seen == {'steps': 6, 'direct': 6, 'cached': 0, 'encodings': 0}
    # the model, its arguments and the features scaler travel in the checkpoint
    ckpt = str(d / 'best_model.pt')
    m = cli.load_checkpoint(ckpt, 'cuda:0')
    assert m.ffn[1].in_features == 51 and m.encoder.use_input_features
    state = torch.load(ckpt, weights_only=True)
    assert state['args']['features_path'] == [paths['feat']] and state['args']['features_size'] == 3
    assert state['args']['no_features_scaling'] is False
    scaled, sc = cli.scale_features(cli.load_input_features([paths['feat']], 16), split['train'])
    assert state['features_scaler'] == {'means': np.asarray(sc.means).tolist(), 'stds': np.asarray(sc.stds).tolist()}
    data_scaler, features_scaler = cli.load_scalers(ckpt)[:2]
    assert np.array_equal(features_scaler.transform(feats), scaled) and features_scaler.stds[1] == 1.0
    # predictions from the checkpoint, with numpy rows and with a resident table
    preds = list(csv.reader(open(d / 'test_preds.csv')))
    want = np.array([[float(c) for c in r[1:]] for r in preds[1:]])
    graphs = load_graphs(paths['npz'])
    again = cli.predict(m, graphs, split['test'], 4, data_scaler, None, scaled)
    assert np.allclose(np.array(again), want, rtol=1e-5, atol=0)
    table = FeatureTable(scaled[split['test']], DEV)
    assert np.allclose(np.array(cli.predict(m, graphs, split['test'], 4, data_scaler, None, table)), want, rtol=1e-5,
                       atol=0)
    # the features matter: other rows, other predictions
    other = cli.predict(m, graphs, split['test'], 4, data_scaler, None, scaled[::-1].copy())
    assert not np.allclose(np.array(other), want, rtol=1e-5, atol=0)
    # fine-tuning from that checkpoint with a frozen encoder: the encodings are computed once per split and every
    # step is the head alone, on [cached encoding | feature rows]
    for k in seen:
        seen[k] = 0
    f = tmp_path / 'f'
    scores = cli.chemprop_train(argv + [str(f), '--frzn_encoder', '--checkpoint_frzn', ckpt])
    assert math.isfinite(scores['rmse'][0])
    assert seen == {'steps': 6, 'direct': 6, 'cached': 6, 'encodings': 3}
    preds = [[float(c) for c in r[1:]] for r in list(csv.reader(open(f / 'test_preds.csv')))[1:]]
    assert len(preds) == 2 and all(math.isfinite(v) for r in preds for v in r)
    state = torch.load(str(f / 'best_model.pt'), weights_only=True)
    assert state['features_scaler'] == {'means': np.asarray(sc.means).tolist(), 'stds': np.asarray(sc.stds).tolist()}
