"""Multiclass models on the native head: softmax cross-entropy in the fused training head
(``wdmpnn_head_mse`` with ``loss_kind`` 2), the prediction head (``wdmpnn_head_predict``) and their wiring
through ``chemprop_amd.train`` and ``MoleculeModel``.

CPU: the header, the ctypes binding and the library agree on the new ABI; the entry points' argument checks
(nothing is launched); class-index validation on the host.
GPU: the fused loss and every gradient against the torch ops of the reference's step, large logits, the
fallback beyond 64 outputs, the direct step, ``head_predict`` for the three dataset types, and the fixture
made from the reference's own multiclass model (tools/make_multiclass_golden.py)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')
TOL = 1e-5
DEV = torch.device('cuda:0')
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1000, -1001, -1003
FIXTURE = 'multiclass/model_polymer_multiclass'


# ---------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_abi_12(tmp_path):
    """wdmpnn_head_predict is declared, bound and exported; the library reports ABI 12; WdHead ends in
    n_classes right behind loss_kind and WdHeadPredict has the header's layout: sizes and offsets as a C
    compiler sees the header.  (sizeof(WdHead) itself stays 176 bytes: on LP64 the new int32 takes the four
    bytes that padded the struct's tail, so the offset and the C layout are what is pinned.)"""
    text = open(HEADER).read()
    assert re.search(r'\bint\s+wdmpnn_head_predict\s*\(\s*const\s+WdHeadPredict\s*\*', text)
    assert '#define WDMPNN_ABI_VERSION 12' in text
    assert 'wdmpnn_head_predict' in _native.EXPORTED_SYMBOLS
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r'\bT wdmpnn_head_predict\b', out)
    L = _native.lib()
    assert _native.ABI_VERSION == 12 and L.wdmpnn_abi_version() == 12
    assert L.wdmpnn_head_predict.argtypes[0]._type_ is _native.WdHeadPredict
    H = _native.WdHead
    assert [n for n, _ in H._fields_][-2:] == ['loss_kind', 'n_classes']
    assert H.n_classes.offset == H.loss_kind.offset + 4 and H.n_classes.size == 4
    assert ctypes.sizeof(H) >= H.n_classes.offset + 4
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wdmpnn.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(WdHead), '
                   'offsetof(WdHead, loss_kind), offsetof(WdHead, n_classes), sizeof(WdHeadPredict), '
                   'offsetof(WdHeadPredict, a), offsetof(WdHeadPredict, out_kind), '
                   'offsetof(WdHeadPredict, n_classes)); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC', 'gcc'), '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _native.WdHeadPredict
    assert c == [ctypes.sizeof(H), H.loss_kind.offset, H.n_classes.offset, ctypes.sizeof(P), P.a.offset,
                 P.out_kind.offset, P.n_classes.offset]


def _head_struct(T=6, kind=2, n_classes=3, ld_table=None, B=4):
    p = 4096  # never dereferenced: every call below is refused by the host-side checks
    tasks = T // n_classes if n_classes > 0 and T % n_classes == 0 else T
    return _native.WdHead(p, 32, B, 32, 16, T, p, p, p, p, p, 2 * tasks if ld_table is None else ld_table, 1.0, 0,
                          p, p, p, p, p, p, p, p, p, p, kind, n_classes)


@pytest.mark.parametrize('kw,rc', [(dict(kind=2, n_classes=1), ERR_SHAPE),
                                   (dict(kind=2, T=7, n_classes=3), ERR_SHAPE),
                                   (dict(kind=2, n_classes=0), ERR_SHAPE),
                                   (dict(kind=0, n_classes=3), ERR_SHAPE),
                                   (dict(kind=1, n_classes=2), ERR_SHAPE),
                                   (dict(kind=2, T=65, n_classes=5), ERR_UNSUPPORTED),
                                   (dict(kind=0, T=65, n_classes=1), ERR_UNSUPPORTED),
                                   (dict(kind=3, n_classes=1), ERR_UNSUPPORTED),
                                   (dict(kind=2, T=6, n_classes=3, ld_table=3), ERR_SHAPE)])
def test_head_entry_points_refuse_bad_class_counts_without_launching(kw, rc):
    """loss_kind 2 needs n_classes >= 2 dividing T, kinds 0 and 1 need n_classes == 1, more than 64 outputs
    are unsupported, and the table holds 2 * tasks columns; the same checks guard wdmpnn_head_predict."""
    L = _native.lib()
    h = _head_struct(**kw)
    got = L.wdmpnn_head_mse(ctypes.byref(h), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()
    with pytest.raises((ValueError, NotImplementedError)):
        _native.check(got, 'head')
    if 'ld_table' not in kw:
        p = 4096
        q = _native.WdHeadPredict(p, 32, 4, 32, 16, h.T, p, p, p, p, 0, p, p, h.loss_kind, h.n_classes)
        assert L.wdmpnn_head_predict(ctypes.byref(q), None) == rc


def test_head_predict_without_rows_is_a_no_op():
    p = 4096
    q = _native.WdHeadPredict(0, 32, 0, 32, 16, 6, p, p, p, p, 0, 0, 0, 2, 3)
    assert _native.lib().wdmpnn_head_predict(ctypes.byref(q), None) == 0


@pytest.mark.parametrize('bad', [2.5, -1, 4, float('nan')])
def test_class_index_validation_names_row_and_task(bad):
    """Every present multiclass target must be an integer in [0, C): checked on the host (torch's own check is
    a device-side assert), for the loss table of the fused step as well."""
    from chemprop_amd.train import _loss_table, check_class_targets
    good = [[0, 3], [None, 1], [2, None], [None, None]]
    check_class_targets(good, 4)
    check_class_targets([], 4)
    table, n_t, n_mask = _loss_table(good, None, None, torch.device('cpu'), num_classes=4)
    assert (n_t, n_mask) == (2, 4) and table.shape == (4, 4)
    rows = [list(r) for r in good]
    rows[2][1] = bad
    with pytest.raises(ValueError, match=r'row 2, task 1'):
        check_class_targets(rows, 4)
    with pytest.raises(ValueError, match=r'row 2, task 1'):
        _loss_table(rows, None, None, torch.device('cpu'), num_classes=4)
    _loss_table(rows, None, None, torch.device('cpu'))  # (regression / classification tables are not checked)


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
def _model(tasks, C, act='ReLU', features=0, ffn_hidden=48, hidden=96, dataset='multiclass', depth=3):
    from chemprop_amd.nn_utils import initialize_weights
    args = TrainArgs(hidden_size=hidden, depth=depth, activation=act, ffn_hidden_size=ffn_hidden, device=DEV,
                     dataset_type=dataset, multiclass_num_classes=C)
    args.num_tasks = tasks
    if features:
        args.use_input_features, args.features_size = True, features
    torch.manual_seed(0)
    m = MoleculeModel(args)
    initialize_weights(m)
    return m.to(DEV)


def _batch(b, tasks, C, features):
    """A polymer batch with ~20 % missing class targets, one row with every target missing, target and data
    weights, optional molecule features."""
    g = BatchMolGraph(synthetic.make_batch('polymer', b, 31 + b), device_bond_features=True)
    rng = np.random.default_rng(b)
    targets = [[None if rng.random() < 0.2 else float(rng.integers(C)) for _ in range(tasks)] for _ in range(b)]
    targets[1] = [None] * tasks
    tw = list(rng.uniform(0.5, 1.5, tasks))
    dw = list(rng.uniform(0.5, 1.5, b))
    feats = [rng.normal(size=features).astype(np.float32) for _ in range(b)] if features else None
    return g, targets, tw, dw, feats


def _fused_and_torch(m, g, feats, targets, tw, dw):
    """(loss, gradients) of the fused head and of the torch ops, with an incoming gradient of 0.75."""
    from chemprop_amd.train import _fusable_head, batch_loss, get_loss_func, head_loss
    lf = get_loss_func('multiclass')
    head = _fusable_head(m, lf, 'multiclass')
    assert head is not None and head[3] == 2 and head[4] == m.num_classes and head[:2] == (m.ffn[1], m.ffn[4])
    res = []
    for fused in (True, False):
        m.zero_grad(set_to_none=True)
        if fused:
            loss = head_loss(m.encoder([g], feats), head, targets, tw, dw)
        else:
            loss = batch_loss(m([g], feats), targets, lf, 'multiclass', tw, dw)
        (loss * 0.75).backward()
        res.append((float(loss), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}))
    return res


def _assert_same(res):
    (l0, g0), (l1, g1) = res
    errs = {n: golden_io.normwise(g0[n].cpu().numpy(), g1[n].cpu().numpy()) for n in g1}
    print(f'fused loss {l0!r} torch loss {l1!r} |diff| {abs(l0 - l1):.3g} worst gradient {max(errs.values()):.3g}')
    assert math.isfinite(l0) and math.isfinite(l1)
    assert abs(l0 - l1) <= 1e-6 * max(1.0, abs(l1)), (l0, l1)
    assert g0.keys() == g1.keys()
    for n in g1:
        assert errs[n] <= TOL, (n, errs[n])


@pytest.mark.gpu
@pytest.mark.parametrize('b,tasks,C,act,features,ffn_hidden', [(5, 1, 2, 'ReLU', 0, 48),
                                                               (33, 3, 5, 'tanh', 5, 80),
                                                               (16, 8, 8, 'ELU', 0, 80),
                                                               (20, 2, 3, 'SELU', 0, 300)])
def test_fused_multiclass_head_loss_matches_torch(b, tasks, C, act, features, ffn_hidden):
    """wdmpnn_head_mse with loss_kind 2 gives the loss of the torch ops (ffn, reshape, CrossEntropyLoss per task,
    weights, mask) within 1e-6 * max(1, |loss|) and every gradient, head and encoder, within 1e-5 normwise:
    rows not a multiple of the 4 waves per workgroup, Hf below and not a multiple of 64, the 64-output cap,
    the default hidden width, missing targets, a row without targets, weights, a scaled incoming gradient."""
    m = _model(tasks, C, act, features, ffn_hidden).train()
    g, targets, tw, dw, feats = _batch(b, tasks, C, features)
    _assert_same(_fused_and_torch(m, g, feats, targets, tw, dw))


@pytest.mark.gpu
def test_fused_multiclass_head_with_logits_beyond_the_exp_range():
    """Logits past 90 in magnitude (fp32 exp overflows from 88.7): the max-subtracted form keeps the loss finite
    and within the same bars as above, the gradients within 1e-5 normwise; the same model through head_predict
    gives no NaN and probabilities that sum to 1 within 1e-6."""
    from chemprop_amd.train import head_predict
    b, tasks, C = 33, 3, 5
    m = _model(tasks, C, 'tanh', 5, 80).train()
    g, targets, tw, dw, feats = _batch(b, tasks, C, 5)
    with torch.no_grad():
        top = float(m([g], feats).abs().max())
        m.ffn[4].weight.mul_(120.0 / top)
        logits = m([g], feats)
    assert float(logits.abs().max()) > 90.0
    _assert_same(_fused_and_torch(m, g, feats, targets, tw, dw))
    m.eval()
    with torch.no_grad():
        p = head_predict(m, m.encoder([g], feats))
    assert p.shape == (b, tasks, C) and bool(torch.isfinite(p).all())
    assert float((p.sum(dim=2) - 1).abs().max()) <= 1e-6
    assert float(p.min()) >= 0.0


@pytest.mark.gpu
def test_more_than_64_outputs_keep_the_torch_path():
    from chemprop_amd.train import _fusable_head, build_optimizer, get_loss_func, train_step
    tasks, C, b = 13, 5, 6
    m = _model(tasks, C, hidden=48)
    lf = get_loss_func('multiclass')
    assert m.ffn[4].out_features == 65 and _fusable_head(m, lf, 'multiclass') is None
    g, targets, _, _, _ = _batch(b, tasks, C, 0)
    before = m.ffn[4].weight.detach().clone()
    loss = float(train_step(m, [g], targets, lf, build_optimizer(m, 1e-3), dataset_type='multiclass'))
    assert math.isfinite(loss) and not torch.equal(before, m.ffn[4].weight.detach())


@pytest.mark.gpu
def test_multiclass_steps_take_the_fused_direct_path():
    """A multiclass MoleculeModel trains through the fused head and the direct step: the same losses and
    parameters bitwise as the fused head under autograd, and within 1e-5 (losses) / 1e-4 normwise (parameters)
    of the torch ops (fused_head=False) over two batches x two epochs."""
    from chemprop_amd.train import _fusable_head, build_optimizer, get_loss_func, train_step
    graphs = [BatchMolGraph(synthetic.make_batch('polymer', 12, 60 + i), device_bond_features=True) for i in range(2)]
    rng = np.random.default_rng(3)
    targets = [[[None if rng.random() < 0.15 else float(rng.integers(3)) for _ in range(2)] for _ in range(12)]
               for _ in range(2)]
    lf = get_loss_func('multiclass')
    res = []
    for mode in ('direct', 'autograd', 'torch'):
        m = _model(2, 3, hidden=48, ffn_hidden=None)
        assert _fusable_head(m, lf, 'multiclass') is not None
        opt = build_optimizer(m, 1e-3)
        losses = [float(train_step(m, [g], t, lf, opt, dataset_type='multiclass', direct=mode == 'direct',
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
def test_fused_step_refuses_a_bad_class_index_on_the_host():
    from chemprop_amd.train import build_optimizer, get_loss_func, train_step
    m = _model(2, 3, hidden=48)
    g, targets, _, _, _ = _batch(6, 2, 3, 0)
    targets[0] = [3.0, 0.0]
    with pytest.raises(ValueError, match='row 0, task 0'):
        train_step(m, [g], targets, get_loss_func('multiclass'), build_optimizer(m, 1e-3), dataset_type='multiclass')


@pytest.mark.gpu
@pytest.mark.parametrize('dataset,tasks,C', [('regression', 3, 1), ('classification', 2, 1), ('multiclass', 3, 5)])
def test_head_predict_matches_the_torch_head(dataset, tasks, C):
    """head_predict against model.ffn(emb) plus the sigmoid, or the reshape plus the softmax, within 1e-5
    normwise; for multiclass MoleculeModel's no-grad eval forward IS head_predict (bitwise), while with grad
    enabled it still builds an autograd graph (the torch ops)."""
    from chemprop_amd.train import head_predict
    b = 9
    m = _model(tasks, max(C, 2), 'LeakyReLU', 0, 80, dataset=dataset).eval()
    g = BatchMolGraph(synthetic.make_batch('polymer', b, 77), device_bond_features=True)
    with torch.no_grad():
        emb = m.encoder([g])
        ref = m.ffn(emb)
        if dataset == 'classification':
            ref = torch.sigmoid(ref)
        elif dataset == 'multiclass':
            ref = torch.softmax(ref.reshape(b, tasks, C), dim=2)
        out = head_predict(m, emb)
    assert out.shape == ((b, tasks, C) if dataset == 'multiclass' else (b, tasks))
    assert golden_io.normwise(out.cpu().numpy(), ref.cpu().numpy()) <= TOL
    if dataset == 'multiclass':
        with torch.no_grad():
            fwd, emb2 = m([g], return_embeddings=True)
        assert torch.equal(fwd, out) and torch.equal(emb2, emb) and fwd.grad_fn is None
        with_grad = m([g])
        assert with_grad.grad_fn is not None
        assert golden_io.normwise(with_grad.detach().cpu().numpy(), ref.cpu().numpy()) <= TOL
    m.train()
    with pytest.raises(ValueError):
        head_predict(m, emb)


def _fixture_model(case):
    a = case.args
    a.device = DEV
    m = MoleculeModel(a)
    synthetic.fill_parameters(m, case.seed)
    return m.to(DEV)


@pytest.mark.gpu
def test_reference_multiclass_model_eval_output_and_gradients():
    """The reference's own multiclass MoleculeModel (eval): class probabilities and the gradients of
    sum(out * R) within 1e-5 normwise with grad enabled (the torch head), and the same probabilities from the
    no-grad forward (the native prediction head)."""
    case = golden_io.load(FIXTURE)
    m = _fixture_model(case).eval()
    out = m(case.graphs, case.features)
    assert out.shape == case.output.shape == (7, 3, 5)
    assert golden_io.normwise(out.detach().cpu().numpy(), case.output) <= TOL
    (out * torch.from_numpy(case.R).to(DEV)).sum().backward()
    grads = {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters() if p.grad is not None}
    assert case.grads
    for n, ref in case.grads.items():
        assert golden_io.normwise(grads[n], ref) <= TOL, n
    with torch.no_grad():
        out_ng = m(case.graphs, case.features)
    assert out_ng.grad_fn is None
    assert golden_io.normwise(out_ng.cpu().numpy(), case.output) <= TOL


@pytest.mark.gpu
def test_reference_multiclass_training_loss_and_gradients():
    """The reference model in train mode with train.py:67-74's loss on the stored targets and weights:
    head_loss gives train_loss within 1e-6 relative and every train_grad/* within 1e-5 normwise."""
    from chemprop_amd.train import _fusable_head, get_loss_func, head_loss
    case = golden_io.load(FIXTURE)
    z = np.load(os.path.join(golden_io.GOLDEN_DIR, FIXTURE + '.npz'), allow_pickle=False)
    targets = [[None if np.isnan(v) else float(v) for v in row] for row in z['targets']]
    assert sum(v is None for r in targets for v in r) >= 3
    m = _fixture_model(case).train()
    head = _fusable_head(m, get_loss_func('multiclass'), 'multiclass')
    assert head is not None
    loss = head_loss(m.encoder(case.graphs, case.features), head, targets, list(z['target_weights']),
                     list(z['data_weights']))
    loss.backward()
    ref = float(z['train_loss'])
    print(f'fused loss {float(loss)!r} reference {ref!r} relative {abs(float(loss) - ref) / abs(ref):.3g}')
    assert abs(float(loss) - ref) <= 1e-6 * abs(ref), (float(loss), ref)
    names = [k[len('train_grad/'):] for k in z.files if k.startswith('train_grad/')]
    assert sorted(names) == sorted(n for n, p in m.named_parameters() if p.grad is not None)
    for n, p in m.named_parameters():
        if p.grad is not None:
            e = golden_io.normwise(p.grad.cpu().numpy(), z['train_grad/' + n])
            assert e <= TOL, (n, e)
