"""Fine-tuning with frozen layers on the GPU: the partial stack head (``wdmpnn_head_stack_partial``) against
``wdmpnn_head_stack`` and fp64 torch ops, the direct step of partly frozen models against the autograd step and
the torch-op step, the frozen encoder's weight pack, cached encodings, the fallbacks, and ``chemprop_train``
with ``--checkpoint_frzn``."""
import csv
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import TrainArgs, _native, cli, polymer, synthetic
from chemprop_amd.featurization import BatchMolGraph
from chemprop_amd.graph_io import save_graphs
from chemprop_amd.model import MoleculeModel
from chemprop_amd.nn_utils import dropout_mask, initialize_weights

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ACT = {'ReLU': 0, 'PReLU': 2, 'tanh': 3}
F, HF = 24, 40
GUARD = 64  # floats on either side of every buffer of the guard-band test
SENTINEL = -7.25


# ---------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------
def _problem(n, act, kind, bias, B):
    """Random layers, inputs and a loss table with non-unit weights and, from two rows on, missing targets."""
    g = torch.Generator().manual_seed(1000 * n + 100 * kind + 10 * ACT[act] + B)
    C = 3 if kind == 2 else 1
    T = 6 if kind == 2 else 3
    widths = [F] + [HF] * (n - 1) + [T]
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
    if B > 1:
        w[1, 0] = 0.0
    if B > 3:
        w[3, :] = 0.0
    table = torch.cat([y, w], dim=1).to(DEV)
    return dict(x=x, Ws=Ws, bs=bs, slope=slope, act=ACT[act], C=C, kind=kind, table=table,
                inv_n=1.0 / float((w > 0).sum()))


def _want(n, dx=True, dW=True, db=True, dslope=True):
    """Which outputs a call asks for: booleans, or one per layer for dW / db."""
    one = lambda v: list(v) if isinstance(v, (list, tuple)) else [bool(v)] * n  # noqa: E731
    return dict(dx=bool(dx), dW=one(dW), db=one(db), dslope=bool(dslope))


def _patterns(n, bias):
    """The want-patterns of one problem: (name, want)."""
    out = [('everything', _want(n)),
           ('no dx', _want(n, dx=False))]
    for f in range(2, n + 1):  # the first f - 1 layers dropped (f == n: the last layer only)
        keep = [l >= f - 1 for l in range(n)]
        out.append((f'from layer {f}', _want(n, dx=False, dW=keep, db=keep, dslope=False)))
    if bias:
        out.append(('bias without weight', _want(n, dx=False, dW=[l != 0 for l in range(n)], dslope=False)))
        out.append(('one bias alone', _want(n, dx=False, dW=False, db=[l == 0 for l in range(n)], dslope=False)))
    out.append(('dslope alone', _want(n, dx=False, dW=False, db=False, dslope=True)))
    out.append(('dx alone', _want(n, dx=True, dW=False, db=False, dslope=False)))
    out.append(('loss alone', _want(n, dx=False, dW=False, db=False, dslope=False)))
    return out


def _call(entry, pr, p, seed, want, arena=None):
    """One call of ``entry`` (wdmpnn_head_stack or wdmpnn_head_stack_partial) on the problem ``pr``; outputs that
    ``want`` leaves out get NULL.  Returns name -> device tensor of what was asked for, and the loss.  ``arena``:
    a callable (name, floats) -> tensor that places every output and the scratch (the guard-band test)."""
    x, Ws, bs = pr['x'], pr['Ws'], pr['bs']
    B, n, T = x.shape[0], len(Ws), Ws[-1].shape[0]
    Hf = Ws[0].shape[0] if n > 1 else 0
    new = arena or (lambda name, k: torch.full((k,), float('nan'), dtype=torch.float32, device=DEV))
    nbytes = _native.head_stack_scratch_bytes(B, F, Hf, T, n)
    scratch = new('scratch', max(nbytes // 4, 4))
    h = _native.WdHeadStack()
    h.x, h.ld_x, h.B, h.F, h.Hf, h.T, h.L = x.data_ptr(), F, B, F, Hf, T, n
    res = {'loss': new('loss', 1)}
    for i in range(n):
        h.W[i], h.b[i] = Ws[i].data_ptr(), _native.ptr(bs[i])
        if want['dW'][i]:
            res[f'dW{i + 1}'] = new(f'dW{i + 1}', Ws[i].numel()).view_as(Ws[i])
            h.dW[i] = res[f'dW{i + 1}'].data_ptr()
        if want['db'][i] and bs[i] is not None:
            res[f'db{i + 1}'] = new(f'db{i + 1}', bs[i].numel())
            h.db[i] = res[f'db{i + 1}'].data_ptr()
    if want['dx']:
        res['dx'] = new('dx', x.numel()).view_as(x)
        h.dx = res['dx'].data_ptr()
    if want['dslope']:
        res['dslope'] = new('dslope', 1)
        h.dslope = res['dslope'].data_ptr()
    h.slope, h.table, h.ld_table = _native.ptr(pr['slope']), pr['table'].data_ptr(), pr['table'].shape[1]
    h.inv_n, h.act, h.p, h.seed, h.loss_kind, h.n_classes = pr['inv_n'], pr['act'], p, seed, pr['kind'], pr['C']
    h.scratch, h.scratch_bytes = scratch.data_ptr(), scratch.numel() * 4
    h.loss = res['loss'].data_ptr()
    _native.check(entry(ctypes.byref(h), _native.current_stream(DEV)), 'head stack')
    torch.cuda.synchronize()
    return res


def _reference(pr, p, seed):
    """The same head in fp64 torch ops on the CPU with explicit masks from dropout_mask."""
    B = pr['x'].shape[0]
    f64 = lambda t: None if t is None else t.detach().cpu().double().requires_grad_(True)  # noqa: E731
    x, Ws, bs, slope = f64(pr['x']), [f64(W) for W in pr['Ws']], [f64(b) for b in pr['bs']], f64(pr['slope'])
    table, C, kind = pr['table'].cpu().double(), pr['C'], pr['kind']

    def drop(v, site):
        return v * torch.from_numpy(dropout_mask(seed, site, B, v.shape[1], p)).double() if p > 0 else v

    a = drop(x, 0)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        z = a @ W.t() + (0 if b is None else b)
        if i < len(Ws) - 1:
            a = {0: torch.relu, 3: torch.tanh, 2: lambda v: torch.nn.functional.prelu(v, slope)}[pr['act']](z)
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
    loss = (per * w).sum() * pr['inv_n']
    loss.backward()
    res = {'loss': loss.detach().numpy().reshape(1), 'dx': x.grad.numpy()}
    if slope is not None and slope.grad is not None:
        res['dslope'] = slope.grad.numpy()
    for i in range(len(Ws)):
        res[f'dW{i + 1}'] = Ws[i].grad.numpy()
        if bs[i] is not None:
            res[f'db{i + 1}'] = bs[i].grad.numpy()
    return res


@pytest.mark.parametrize('act', ['ReLU', 'tanh', 'PReLU'])
@pytest.mark.parametrize('n', [1, 2, 4])
def test_partial_head_is_bitwise_the_full_head(n, act):
    """Every wanted output and the loss of ``wdmpnn_head_stack_partial`` are ``torch.equal`` to what
    ``wdmpnn_head_stack`` writes on the same inputs and seed: B in {1, 5, 37} (one row; no multiple of the 4 rows
    of a row workgroup; three 16-row tiles), F = 24, Hf = 40 (no multiple of 16 or 32), T = 3 (multiclass 6 = 2 x 3),
    the three loss kinds, p in {0, 0.25}, with and without biases, and every want-pattern of ``_patterns``.  One
    pattern per problem with biases is also held against fp64 torch ops at 1e-5 normwise."""
    L = _native.lib()
    checked = 0
    for B in (1, 5, 37):
        for kind in (0, 1, 2):
            for p in (0.0, 0.25):
                for bias in (True, False):
                    pr = _problem(n, act, kind, bias, B)
                    seed = 0xC0FFEE + 7 * n + B
                    full = _call(L.wdmpnn_head_stack, pr, p, seed, _want(n))
                    assert all(torch.isfinite(v).all() for v in full.values())
                    pats = _patterns(n, bias)
                    for name, want in pats:
                        got = _call(L.wdmpnn_head_stack_partial, pr, p, seed, want)
                        assert 'loss' in got and set(got) <= set(full)
                        for k, v in got.items():
                            assert torch.equal(v, full[k]), (B, kind, p, bias, name, k)
                        checked += 1
                    if bias and kind == {'ReLU': 0, 'tanh': 1, 'PReLU': 2}[act] and B == 37:
                        # (against fp64: a pattern that stops the chain in the middle, or at dx for one layer)
                        name, want = pats[2] if n > 1 else pats[-2]
                        got = _call(L.wdmpnn_head_stack_partial, pr, p, seed, want)
                        ref = _reference(pr, p, seed)
                        for k, v in got.items():
                            if k == 'dslope' and not (act == 'PReLU' and n > 1):
                                assert float(v) == 0.0
                                continue
                            e = golden_io.normwise(v.cpu().numpy(), ref[k])
                            assert e <= 1e-5, (name, k, e)
    assert checked >= 3 * 3 * 2 * (2 * 5 + 2)


@pytest.mark.parametrize('n,act,bias', [(4, 'PReLU', True), (1, 'ReLU', True), (3, 'tanh', False)])
def test_partial_head_writes_nothing_but_what_it_is_asked_for(n, act, bias):
    """One allocation holds every output buffer and the scratch, each between guard bands of a sentinel value:
    after the call every guard band is intact, for each want-pattern."""
    L = _native.lib()
    pr = _problem(n, act, 2, bias, 37)
    for name, want in _patterns(n, bias):
        block = torch.full((1 << 18,), SENTINEL, dtype=torch.float32, device=DEV)
        spans, pos = [], [GUARD]

        def arena(label, k, block=block, spans=spans, pos=pos):
            k4 = (k + 3) // 4 * 4  # (16-byte aligned buffers: the scratch must be)
            lo = pos[0]
            pos[0] = lo + k4 + GUARD
            assert pos[0] <= block.numel()
            spans.append((lo, lo + k))
            return block[lo:lo + k]

        got = _call(L.wdmpnn_head_stack_partial, pr, 0.25, 99, want, arena)
        assert torch.isfinite(got['loss']).all()
        inside = torch.zeros(block.numel(), dtype=torch.bool, device=DEV)
        for lo, hi in spans:
            inside[lo:hi] = True
        assert bool((block[~inside] == SENTINEL).all()), name
        for k, v in got.items():  # (and what was asked for was written)
            assert bool((v != SENTINEL).all()), (name, k)


# ---------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------
def _model(layers, dataset='regression', act='ReLU', freeze='a', dropout=0.0, **kw):
    """hidden 32, depth 3; ``freeze``: 'a' encoder and first FFN layer, 'b' encoder only, 'c' first FFN layer with a
    trainable encoder, '' nothing."""
    args = TrainArgs(hidden_size=32, depth=3, activation=act, ffn_num_layers=layers, dropout=dropout, device=DEV,
                     dataset_type=dataset, multiclass_num_classes=3, bias=True, num_tasks=2, **kw)
    torch.manual_seed(0)
    m = MoleculeModel(args)
    initialize_weights(m)
    with torch.no_grad():  # (initialize_weights zeroes every 1-D parameter: give slopes and biases values)
        g = torch.Generator().manual_seed(5)
        for mod in m.modules():
            if isinstance(mod, torch.nn.PReLU):
                mod.weight.fill_(0.25)
        for mod in m.ffn:
            if isinstance(mod, torch.nn.Linear):
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
    if freeze in ('a', 'b'):
        cli.apply_freezing(m, frzn_encoder=True, frzn_ffn_layers=1 if freeze == 'a' else 0)
    elif freeze == 'c':
        for q in m.ffn[1].parameters():
            q.requires_grad_(False)
    return m.to(DEV)


def _targets(dataset, b, tasks, seed):
    rng = np.random.default_rng(seed)

    def one():
        if rng.random() < 0.15:
            return None
        if dataset == 'regression':
            return float(rng.normal())
        return float(rng.random() < 0.5) if dataset == 'classification' else float(rng.integers(3))
    return [[one() for _ in range(tasks)] for _ in range(b)]


MOLS = [synthetic.make_batch('polymer', 8, 40 + i) for i in range(3)]


def _run(model, dataset, mode, steps=3, encodings=None, before=None):
    """Three HipAdam steps on the three batches; mode 'direct', 'autograd' or 'torch'.  Returns (losses,
    parameters by name, the optimizer)."""
    from chemprop_amd.train import HipAdam, build_optimizer, get_loss_func, train_step
    lf = get_loss_func(dataset)
    opt = build_optimizer(model, 1e-3)
    assert isinstance(opt, HipAdam)
    losses = []
    for i in range(steps):
        if before is not None:
            before(i)
        kw = dict(encodings=encodings[i]) if encodings is not None else {}
        losses.append(float(train_step(model, None if encodings is not None else [BatchMolGraph(MOLS[i])],
                                       _targets(dataset, 8, 2, 20 + i), lf, opt, dataset_type=dataset,
                                       direct=mode == 'direct', fused_head=mode != 'torch', **kw)))
    assert all(math.isfinite(v) for v in losses)
    return losses, {k: v.detach().clone() for k, v in model.named_parameters()}, opt


@pytest.mark.parametrize('dataset', ['regression', 'classification', 'multiclass'])
@pytest.mark.parametrize('layers', [2, 3])
def test_frozen_direct_step_equals_the_autograd_and_torch_steps(layers, dataset):
    """Patterns (a) encoder and first layer frozen, (b) encoder frozen, (c) first layer frozen under a trainable
    encoder: three steps of the direct step are bitwise the autograd step (``direct=False``: the same encoder
    call -- the inference forward on the same device graph and config for a frozen encoder, the training forward
    and backward otherwise -- and the same stack head with the same gradients left out), and within 1e-5 (losses)
    / 1e-4 normwise (parameters) of the torch-op step.  Frozen parameters keep their initial bits, have no
    gradient and no optimizer state."""
    from chemprop_amd.train import _fusable_head, _frozen_plan, get_loss_func
    for freeze in 'abc':
        res = {}
        for mode in ('direct', 'autograd', 'torch'):
            m = _model(layers, dataset, freeze=freeze).train()
            if mode == 'direct':
                plan = _frozen_plan(m, [BatchMolGraph(MOLS[0])], None, _fusable_head(m, get_loss_func(dataset), dataset))
                assert plan is not None and plan.enc_frozen == (freeze != 'c')
            init = {k: v.detach().clone() for k, v in m.named_parameters()}
            losses, params, opt = _run(m, dataset, mode)
            res[mode] = (losses, params)
            for k, q in m.named_parameters():
                if not q.requires_grad:
                    assert torch.equal(q, init[k]), (freeze, mode, k)
                    assert q.grad is None, (freeze, mode, k)
                    assert q not in opt.state or not opt.state[q], (freeze, mode, k)
                else:
                    assert not torch.equal(q, init[k]), (freeze, mode, k)
        assert res['direct'][0] == res['autograd'][0], freeze
        for k in res['direct'][1]:
            assert torch.equal(res['direct'][1][k], res['autograd'][1][k]), (freeze, k)
        for a, b in zip(res['direct'][0], res['torch'][0]):
            assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (freeze, a, b)
        for k in res['direct'][1]:
            e = golden_io.normwise(res['direct'][1][k].cpu().numpy(), res['torch'][1][k].cpu().numpy())
            assert e <= 1e-4, (freeze, k, e)


def test_a_stale_gradient_on_a_frozen_parameter_moves_nothing():
    m = _model(3, freeze='a').train()
    frozen = {k: q for k, q in m.named_parameters() if not q.requires_grad and 'cached_zero_vector' not in k}
    init = {k: q.detach().clone() for k, q in frozen.items()}

    def stale(i):
        if i == 0:
            for q in frozen.values():
                q.grad = torch.ones_like(q)

    ref = _run(_model(3, freeze='a').train(), 'regression', 'direct')
    losses, params, opt = _run(m, 'regression', 'direct', before=stale)
    for k, q in frozen.items():
        assert torch.equal(q, init[k]) and q.grad is None and (q not in opt.state or not opt.state[q]), k
    assert losses == ref[0] and all(torch.equal(params[k], ref[1][k]) for k in params)


def test_frozen_encoder_packs_its_weights_once(monkeypatch):
    """Three steps with a frozen encoder enqueue ONE weight pack (the pack's key has no optimizer-step count);
    ``invalidate_packed_params()`` drops it, and so does unfreezing."""
    L = _native.lib()
    real = L.wdmpnn_pack_params
    calls = []

    def counting(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(L, 'wdmpnn_pack_params', counting)
    for mode in ('direct', 'autograd'):
        m = _model(3, freeze='a').train()
        del calls[:]
        _run(m, 'regression', mode)
        assert len(calls) == 1, mode
        m.encoder.encoder[0].invalidate_packed_params()
        _run(m, 'regression', mode, steps=1)
        assert len(calls) == 2, mode
        _run(m, 'regression', mode, steps=1)
        assert len(calls) == 2, mode
    m.load_state_dict(m.state_dict())
    _run(m, 'regression', 'direct', steps=1)
    assert len(calls) == 3
    for _, q in m.encoder.encoder[0]._direct_names():  # unfrozen: the optimizer writes the weights, every step packs
        q.requires_grad_(True)
    del calls[:]
    _run(m, 'regression', 'autograd', steps=2)
    assert len(calls) >= 2


def test_steps_from_cached_encodings_are_bitwise_the_steps_that_run_the_encoder():
    from chemprop_amd.train import frozen_encodings, get_loss_func, train_step
    ref = _run(_model(3, freeze='a').train(), 'regression', 'direct')
    m = _model(3, freeze='a').train()
    rows = frozen_encodings(m, [g for mols in MOLS for g in mols], 8)
    assert rows.shape == (24, 32) and rows.device.type == 'cuda' and not rows.requires_grad
    with torch.no_grad():
        for i in range(3):
            assert torch.equal(rows[8 * i:8 * i + 8], m.encoder([BatchMolGraph(MOLS[i])]))
    other = frozen_encodings(m, [g for mols in MOLS for g in mols], 5)  # (another batching: the same rows)
    assert torch.equal(other, rows)
    got = _run(m, 'regression', 'direct', encodings=[rows[8 * i:8 * i + 8] for i in range(3)])
    assert got[0] == ref[0]
    for k in ref[1]:
        assert torch.equal(got[1][k], ref[1][k]), k
    assert frozen_encodings(m, [], 8).shape == (0, 32)
    with pytest.raises(ValueError, match='trainable'):
        frozen_encodings(_model(3, freeze='c'), MOLS[0], 8)
    with pytest.raises(ValueError, match='dropout'):
        frozen_encodings(_model(3, freeze='a', dropout=0.1), MOLS[0], 8)
    # encodings are for the direct step of a frozen encoder only
    lf = get_loss_func('regression')
    from chemprop_amd.train import build_optimizer
    for bad, kw in ((_model(3, freeze='c'), {}), (_model(3, freeze='a'), dict(direct=False)),
                    (_model(3, freeze='a', dropout=0.1), {})):
        with pytest.raises(ValueError, match='encodings'):
            train_step(bad, None, _targets('regression', 8, 2, 1), lf, build_optimizer(bad, 1e-3), encodings=rows[:8],
                       **kw)


def test_fallbacks_still_train():
    """model.py:118-121's ``parameters()[0:2N]`` slice on a PReLU FFN freezes W1, b1, the slope and W2 but not
    b2 (it splits a layer): any subset of the FFN is a frozen plan, so the direct step runs it.  A partly frozen
    encoder is no plan and keeps the autograd path.  Both match the torch-op step."""
    from chemprop_amd.train import _fusable_head, _frozen_plan, get_loss_func

    def sliced():
        m = _model(3, act='PReLU', freeze='', checkpoint_frzn='pretrained.pt', frzn_ffn_layers=2)
        frozen = {k for k, q in m.named_parameters() if not q.requires_grad and k.startswith('ffn.')}
        assert frozen == {'ffn.1.weight', 'ffn.1.bias', 'ffn.2.weight', 'ffn.4.weight'}
        return m.train()

    def partly():
        m = _model(3, act='PReLU', freeze='')
        m.encoder.encoder[0].W_i.weight.requires_grad_(False)
        m.ffn[1].weight.requires_grad_(False)
        return m.train()

    lf = get_loss_func('regression')
    batch = [BatchMolGraph(MOLS[0])]
    m = sliced()
    plan = _frozen_plan(m, batch, None, _fusable_head(m, lf, 'regression'))
    assert plan is not None and plan.enc_frozen and len(plan.frozen) == 4 + len(m.encoder.encoder[0]._direct_names())
    m = partly()
    assert _frozen_plan(m, batch, None, _fusable_head(m, lf, 'regression')) is None
    for make in (sliced, partly):
        init = {k: v.detach().clone() for k, v in make().named_parameters()}
        got, ref = _run(make(), 'regression', 'direct'), _run(make(), 'regression', 'torch')
        for a, b in zip(got[0], ref[0]):
            assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (a, b)
        for k in got[1]:
            assert golden_io.normwise(got[1][k].cpu().numpy(), ref[1][k].cpu().numpy()) <= 1e-4, k
        moved = {k for k in init if not torch.equal(init[k], got[1][k])}
        assert moved == {k for k, q in make().named_parameters() if q.requires_grad}


# ---------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------
def test_chemprop_train_finetunes_from_a_checkpoint(tmp_path):
    """24 synthetic polymers: a short pretraining run, then two epochs from its best checkpoint with
    ``--frzn_ffn_layers 1 --train_frac 0.5``: the encoder and ffn.1 keep the pretrained bits, the later layers
    move, half of the training split is used, and the run without the encoding cache ends in the same bits."""
    rng = np.random.default_rng(5)
    rows, graphs = [], []
    for k in range(24):
        fa = float(rng.choice([0.25, 0.5, 0.75]))
        xn = float(rng.choice([1, 10, 100, 1000]))
        s = f'[*:1]c1ccc([*:2])cc1.[*:3]CC[*:4]|{fa}|{1 - fa}|<1-3:0.5:0.5<2-4:0.5:0.5<1-2:0.5:0.5~{xn:g}'
        rows.append([s, 2.0 * fa - 0.5 * np.log10(xn)])
        graphs.append(polymer.synthetic_polymer_graph(s, seed=k))
    csv_path, npz_path = str(tmp_path / 'p.csv'), str(tmp_path / 'p.npz')
    with open(csv_path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['smiles', 'y'])
        w.writerows(rows)
    save_graphs(npz_path, graphs)
    base = ['--data_path', csv_path, '--graphs_path', npz_path, '--polymer', '--epochs', '2', '--hidden_size', '32',
            '--ffn_num_layers', '3', '--batch_size', '4', '--save_dir']
    cli.chemprop_train(base + [str(tmp_path / 'pre')])
    pre = torch.load(tmp_path / 'pre' / 'best_model.pt', weights_only=True)['state_dict']
    tune = ['--checkpoint_frzn', str(tmp_path / 'pre' / 'best_model.pt'), '--frzn_ffn_layers', '1', '--train_frac',
            '0.5', '--weight_decay', '0.01', '--optimizer', 'adamw']
    cli.chemprop_train(base + [str(tmp_path / 'ft')] + tune)
    cli.chemprop_train(base + [str(tmp_path / 'ft_nocache')] + tune + ['--no_encoding_cache'])
    out = torch.load(tmp_path / 'ft' / 'model.pt', weights_only=True)
    sd = out['state_dict']
    assert out['args']['frzn_encoder'] is True and out['args']['frzn_ffn_layers'] == 1
    assert sd.keys() == pre.keys()
    for k in sd:
        if k.startswith('encoder.') or k.startswith('ffn.1.'):
            assert torch.equal(sd[k], pre[k]), k
        else:
            assert not torch.equal(sd[k], pre[k]), k
    split = json.load(open(tmp_path / 'ft' / 'split_indices.json'))
    full = cli.random_split(24, (0.8, 0.1, 0.1), 0)
    n_train = len(full[0])
    assert len(split['train']) == int(n_train * 0.5) and set(split['train']) <= set(full[0])
    assert split['train'] == [full[0][k] for k in cli.subsample_train(n_train, 0.5, 0)]
    assert split['val'] == full[1] and split['test'] == full[2]
    for f in ('test_scores.json', 'test_scores.csv', 'test_preds.csv', 'train_val_loss_log.csv', 'best_model.pt'):
        assert (tmp_path / 'ft' / f).exists(), f
    assert math.isfinite(json.load(open(tmp_path / 'ft' / 'test_scores.json'))['rmse'][0])
    other = torch.load(tmp_path / 'ft_nocache' / 'model.pt', weights_only=True)['state_dict']
    for k in sd:
        assert torch.equal(sd[k], other[k]), k
