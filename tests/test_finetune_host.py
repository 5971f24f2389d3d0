"""Fine-tuning from a pretrained checkpoint with frozen layers: the host side.

The partial stack head's export and refusals (``wdmpnn_head_stack_partial``), the frozen-plan recogniser of the
direct step (``train._frozen_plan``), ``--checkpoint_frzn`` loading, the freezing rules of ``--frzn_encoder`` /
``--frzn_ffn_layers`` and the ``--train_frac`` subsample.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from chemprop_amd import MoleculeModel, TrainArgs, _native, cli, synthetic
from chemprop_amd.featurization import BatchMolGraph
from chemprop_amd.train import _direct_encoder, _frozen_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wdmpnn.h')
ERR_ARG, ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -1000, -1001, -1002, -1003
CPU = torch.device('cpu')


def test_partial_head_is_declared_bound_and_exported():
    text = open(HEADER).read()
    assert '#define WDMPNN_ABI_VERSION 12' in text
    assert re.search(r'\bint\s+wdmpnn_head_stack_partial\s*\(\s*const\s+WdHeadStack\s*\*', text)
    assert 'wdmpnn_head_stack_partial' in _native.EXPORTED_SYMBOLS
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r'\bT wdmpnn_head_stack_partial\b', out)
    L = _native.lib()
    assert L.wdmpnn_abi_version() == 12 and _native.ABI_VERSION == 12
    assert L.wdmpnn_head_stack_partial.argtypes[0]._type_ is _native.WdHeadStack


def _fake_stack(L=3, T=6, kind=2, n_classes=3, p=0.25, ld_table=None, B=4, scratch=4096, F=32, Hf=16, grads=True):
    """A WdHeadStack of made-up addresses (never dereferenced: every call below is refused on the host or has no
    rows).  ``grads=False``: every gradient pointer NULL."""
    a = 4096
    h = _native.WdHeadStack()
    h.x, h.ld_x, h.B, h.F, h.Hf, h.T, h.L = a, F, B, F, Hf, T, L
    for i in range(min(max(L, 0), _native.HEAD_MAX_LAYERS)):
        h.W[i], h.b[i] = a, a
        if grads:
            h.dW[i], h.db[i] = a, a
    tasks = T // n_classes if n_classes > 0 and T % n_classes == 0 else T
    h.slope, h.table, h.ld_table, h.inv_n, h.act = a, a, 2 * tasks if ld_table is None else ld_table, 1.0, 2
    h.p, h.seed, h.loss_kind, h.n_classes = p, 7, kind, n_classes
    h.scratch, h.scratch_bytes = scratch, 1 << 30
    h.loss = a
    if grads:
        h.dx, h.dslope = a, a
    return h


@pytest.mark.parametrize('grads', [True, False])
@pytest.mark.parametrize('kw,rc', [(dict(L=0), ERR_SHAPE),
                                   (dict(L=7), ERR_UNSUPPORTED),
                                   (dict(T=65, n_classes=5), ERR_UNSUPPORTED),
                                   (dict(F=4097), ERR_UNSUPPORTED),
                                   (dict(Hf=4097), ERR_UNSUPPORTED),
                                   (dict(p=-0.1), ERR_ARG),
                                   (dict(p=1.0), ERR_ARG),
                                   (dict(p=float('nan')), ERR_ARG),
                                   (dict(ld_table=3), ERR_SHAPE),
                                   (dict(scratch=0), ERR_ARG)])
def test_partial_head_keeps_the_refusals_of_the_full_head(kw, rc, grads):
    L = _native.lib()
    h = _fake_stack(grads=grads, **kw)
    got = L.wdmpnn_head_stack_partial(ctypes.byref(h), None)
    assert got == rc, (got, L.wdmpnn_last_error().decode())
    assert L.wdmpnn_last_error().decode()


def test_partial_head_refuses_null_inputs_and_a_small_scratch():
    L = _native.lib()
    for field in ('loss', 'x', 'table'):
        h = _fake_stack(grads=False)
        setattr(h, field, 0)
        assert L.wdmpnn_head_stack_partial(ctypes.byref(h), None) == ERR_ARG, field
    h = _fake_stack(grads=False)
    h.W[1] = 0
    assert L.wdmpnn_head_stack_partial(ctypes.byref(h), None) == ERR_ARG
    h = _fake_stack(grads=False, L=3, B=5, F=40, Hf=37, T=6)
    h.scratch_bytes = _native.head_stack_scratch_bytes(5, 40, 37, 6, 3) - 4
    assert L.wdmpnn_head_stack_partial(ctypes.byref(h), None) == ERR_WORKSPACE


def test_null_gradients_are_accepted_by_the_partial_head_only():
    """No rows: nothing is launched, so made-up addresses do.  Every gradient pointer NULL is a valid request
    (the loss alone) for the partial head, and still a refusal for wdmpnn_head_stack."""
    L = _native.lib()
    h = _fake_stack(B=0, grads=False)
    assert L.wdmpnn_head_stack_partial(ctypes.byref(h), None) == 0
    assert L.wdmpnn_head_stack(ctypes.byref(h), None) == ERR_ARG
    assert 'null gradient' in L.wdmpnn_last_error().decode()
    g = _fake_stack(B=4, grads=True)
    g.dx = 0
    assert L.wdmpnn_head_stack(ctypes.byref(g), None) == ERR_ARG  # (dx is required there once there are rows)


# ---------------------------------------------------------------------------------------------------
# the frozen plan
# ---------------------------------------------------------------------------------------------------
def _cpu_model(layers=3, **kw):
    return MoleculeModel(TrainArgs(hidden_size=32, depth=3, ffn_num_layers=layers, device=CPU, **kw))


def _head(model):
    """What ``_fusable_head`` gives on the GPU for a regression model (the recogniser does not look at devices)."""
    from chemprop_amd.train import _ffn_structure
    if len(model.ffn) == 5:
        return model.ffn[1], model.ffn[4], 0, 0, 1
    return _ffn_structure(model.ffn, True).with_kind(0, 1)


@pytest.mark.parametrize('layers', [2, 3])
def test_frozen_plan_recognition(layers):
    batch = [BatchMolGraph(synthetic.make_batch('polymer', 2, 0))]
    enc_of = lambda m: m.encoder.encoder[0]  # noqa: E731

    # nothing frozen: _direct_encoder's business, not a frozen plan
    m = _cpu_model(layers)
    assert _direct_encoder(m, batch, None, _head(m)) is enc_of(m)
    assert _frozen_plan(m, batch, None, _head(m)) is None

    # encoder and first layer frozen
    m = _cpu_model(layers)
    cli.apply_freezing(m, frzn_ffn_layers=1)
    assert _direct_encoder(m, batch, None, _head(m)) is None  # (unchanged: any frozen parameter stops it)
    plan = _frozen_plan(m, batch, None, _head(m))
    assert plan is not None and plan.enc is enc_of(m) and plan.enc_frozen
    assert len(plan.head.linears) == layers and plan.head.kind == 0  # (the two-layer head as a stack head too)
    assert {id(p) for p in plan.frozen} == {id(p) for p in m.parameters()
                                            if not p.requires_grad and p is not enc_of(m).cached_zero_vector}
    assert any(p is m.ffn[1].weight for p in plan.frozen) and plan.grad_of(m.ffn[1].weight) is None
    assert _frozen_plan(m, None, None, _head(m), cached=True) is not None  # (a step from cached encodings has no batch)
    assert _frozen_plan(m, None, None, _head(m)) is None

    # encoder trainable, one bias frozen
    m = _cpu_model(layers)
    m.ffn[1].bias.requires_grad_(False)
    plan = _frozen_plan(m, batch, None, _head(m))
    assert plan is not None and not plan.enc_frozen and [id(p) for p in plan.frozen] == [id(m.ffn[1].bias)]
    assert _direct_encoder(m, batch, None, _head(m)) is None

    # a partly frozen encoder, a parameter outside encoder and FFN, two molecules, extra features: not a plan
    m = _cpu_model(layers)
    enc_of(m).W_i.weight.requires_grad_(False)
    assert _frozen_plan(m, batch, None, _head(m)) is None
    m = _cpu_model(layers)
    cli.apply_freezing(m, frzn_encoder=True)
    assert _frozen_plan(m, batch, None, _head(m)) is not None
    assert _frozen_plan(m, batch + batch, None, _head(m)) is None
    assert _frozen_plan(m, batch, [np.zeros(3)], _head(m)) is None
    assert _frozen_plan(m, batch, None, None) is None
    m.extra = torch.nn.Parameter(torch.zeros(3))
    assert _frozen_plan(m, batch, None, _head(m)) is None
    m.extra.requires_grad_(False)
    assert _frozen_plan(m, batch, None, _head(m)) is None
    assert _direct_encoder(m, batch, None, _head(m)) is None


# ---------------------------------------------------------------------------------------------------
# --checkpoint_frzn, --frzn_encoder, --frzn_ffn_layers, --train_frac
# ---------------------------------------------------------------------------------------------------
def _two_models():
    torch.manual_seed(1)
    src = _cpu_model(3)
    with torch.no_grad():
        for p in src.parameters():
            if p.requires_grad:
                p.copy_(torch.randn(p.shape))
    torch.manual_seed(2)
    return src, _cpu_model(3)


@pytest.mark.parametrize('key', ['state_dict', 'model_state_dict'])
def test_checkpoint_frzn_accepts_both_spellings_and_old_names(tmp_path, key):
    src, dst = _two_models()
    sd = {k.replace('encoder.encoder.0.', 'encoder.encoder.'): v for k, v in src.state_dict().items()}
    assert any(k.startswith('encoder.encoder.W_i') for k in sd)
    path = str(tmp_path / 'pre.pt')
    torch.save({key: sd, 'epoch': 3}, path)
    msgs = []
    loaded, skipped = cli.load_frzn_checkpoint(dst, path, msgs.append)
    assert sorted(loaded) == sorted(src.state_dict()) and skipped == []
    for (k, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a, b), k
    assert any('loaded' in m for m in msgs)
    assert all(p.requires_grad for n, p in dst.named_parameters() if 'cached_zero_vector' not in n)  # nothing frozen


def test_checkpoint_frzn_skips_what_does_not_fit_and_refuses_an_empty_match(tmp_path):
    src, dst = _two_models()
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    sd = dict(src.state_dict())
    sd['ffn.7.weight'] = torch.zeros(5, 32)          # another number of outputs (the pretraining task's)
    sd['ffn.7.bias'] = torch.zeros(5)
    sd['ssl_head.weight'] = torch.zeros(4, 4)        # a name the model does not have
    path = str(tmp_path / 'pre.pt')
    torch.save({'state_dict': sd}, path)
    msgs = []
    loaded, skipped = cli.load_frzn_checkpoint(dst, path, msgs.append)
    assert sorted(skipped) == ['ffn.7.bias', 'ffn.7.weight', 'ssl_head.weight']
    assert 'ffn.7.weight' not in loaded and 'ffn.1.weight' in loaded
    for name in ('ffn.7.bias', 'ffn.7.weight', 'ssl_head.weight'):
        assert any(name in m and 'skipped' in m for m in msgs), name
    now = dst.state_dict()
    assert torch.equal(now['ffn.7.weight'], before['ffn.7.weight'])
    assert torch.equal(now['ffn.1.weight'], src.state_dict()['ffn.1.weight'])
    torch.save({'state_dict': {'other.weight': torch.zeros(2), 'ffn.1.weight': torch.zeros(3, 3)}}, path)
    with pytest.raises(ValueError, match='no tensor matches'):
        cli.load_frzn_checkpoint(dst, path, msgs.append)
    torch.save({'weights': {}}, path)
    with pytest.raises(ValueError, match='not a checkpoint'):
        cli.load_frzn_checkpoint(dst, path, msgs.append)


def _frozen_names(m):
    return {n for n, p in m.named_parameters() if not p.requires_grad and 'cached_zero_vector' not in n}


def test_freezing_rules():
    m = _cpu_model(3, activation='PReLU')
    cli.apply_freezing(m)
    assert _frozen_names(m) == set()
    cli.apply_freezing(m, frzn_encoder=True)
    assert _frozen_names(m) == {n for n, _ in m.named_parameters()
                                if n.startswith('encoder.') and 'cached_zero_vector' not in n}
    # the FIRST N Linear layers, weight and bias, whatever sits between them (here the PReLU slope, ffn.2.weight),
    # and the encoder with them
    m = _cpu_model(3, activation='PReLU')
    cli.apply_freezing(m, frzn_ffn_layers=1)
    ffn = {n for n in _frozen_names(m) if n.startswith('ffn.')}
    assert ffn == {'ffn.1.weight', 'ffn.1.bias'}
    assert all(not p.requires_grad for p in m.encoder.parameters())
    m = _cpu_model(3, activation='PReLU')
    cli.apply_freezing(m, frzn_ffn_layers=2)
    assert {n for n in _frozen_names(m) if n.startswith('ffn.')} == {'ffn.1.weight', 'ffn.1.bias', 'ffn.4.weight',
                                                                   'ffn.4.bias'}
    for n in (3, 4):
        with pytest.raises(ValueError, match='frzn_ffn_layers'):
            cli.apply_freezing(_cpu_model(3), frzn_ffn_layers=n)
    with pytest.raises(ValueError):
        cli.apply_freezing(_cpu_model(3), frzn_ffn_layers=-1)
    assert TrainArgs(device=CPU).frzn_encoder is False


def test_cli_flags_parse():
    base = ['--data_path', 'd.csv', '--graphs_path', 'g.npz', '--save_dir', 'o']
    a = cli.parse_args(base)
    assert (a.checkpoint_frzn, a.frzn_encoder, a.frzn_ffn_layers, a.train_frac, a.weight_decay, a.optimizer,
            a.no_encoding_cache) == (None, False, 0, 1.0, 0.0, 'adam', False)
    a = cli.parse_args(base + ['--checkpoint_frzn', 'p.pt', '--frzn_encoder', '--frzn_ffn_layers', '1', '--train_frac',
                               '0.5', '--weight_decay', '0.01', '--optimizer', 'adamw', '--no_encoding_cache'])
    assert (a.checkpoint_frzn, a.frzn_encoder, a.frzn_ffn_layers, a.train_frac, a.weight_decay, a.optimizer,
            a.no_encoding_cache) == ('p.pt', True, 1, 0.5, 0.01, 'adamw', True)


@pytest.mark.parametrize('seed', [0, 1])
def test_train_frac_follows_the_reference_rule(seed):
    got = cli.subsample_train(20, 0.5, seed)
    assert got == np.random.default_rng(seed).choice(20, 10, replace=False).tolist()
    assert len(set(got)) == 10 and all(0 <= i < 20 for i in got)
    assert len(cli.subsample_train(19, 0.5, seed)) == 9  # int(n_train * F)
    with pytest.raises(ValueError):
        cli.subsample_train(20, 0.0, seed)
