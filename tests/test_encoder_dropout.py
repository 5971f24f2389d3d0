"""Encoder dropout, forward and backward, against an fp64 reference that applies the same masks.

The native encoder stores no mask: every kernel that needs one derives it again from (seed, site, row, col) with
``dropout_scale`` (csrc/common.hpp), whose contract is ``chemprop_amd.nn_utils.dropout_mask``.  The tests build
the masks from that contract with the encoder's site numbering (``dropout_ref``; DESIGN.md "Dropout sites"), hand
them to ``oracle.mpn_ref.encoder_forward(drop=...)`` and ask the project's bar of the HIP path: 1e-5 normwise per
tensor, outputs against the fp32 oracle, gradients against the fp64 evaluation that shares the HIP forward's kink
decisions (``test_gpu_parity._oracle_vs_hip``'s recipe).  A wrong site number, a block-local row in place of the
natural row, a wrong 1 / (1 - p), a backward that disagrees with its forward, or an fp16 pair scale taken before the
mask (p >= 0.5 then overflows fp16) all fail them.

The seed of a forward: ``torch.manual_seed(s); seed = mpn._dropout_seed()``, then ``torch.manual_seed(s)`` again and
the forward draws the same seed (asserted on the grad-enabled path through ``out.grad_fn.cfg.seed``).
"""
import ctypes

import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import TrainArgs, mpn, synthetic
from chemprop_amd.featurization import BatchMolGraph, get_atom_fdim, get_bond_fdim
from chemprop_amd.mpn import MPNEncoder
from chemprop_amd.nn_utils import dropout_mask
from dropout_ref import graph_masks, ones_like_masks
from oracle import mpn_ref

TOL = 1e-5
MATTER = 1e-2  # the masked and the unmasked reference must differ by more than this
DEV = torch.device('cuda:0')
SEED = 0x9C0FFEE123456789  # the CPU tests' mask seed (any 64-bit value)


# (batch kind, batch size, hidden, depth, encoder options, p, descriptor size); batches are
# synthetic.make_batch('polymer', b, 700 + b), 'edge' the edge-case batch with a 130-leaf hub
A_CASES = [
    ('polymer', 16, 64, 3, dict(activation='ReLU', bias=True), 0.25, 0),
    ('polymer', 12, 300, 4, dict(activation='LeakyReLU'), 0.5, 0),   # fp16-pair backward GEMMs restage masked M
    ('polymer', 8, 300, 3, dict(activation='PReLU', bias=True, aggregation='norm'), 0.75, 0),  # dslope sums
    ('polymer', 8, 96, 3, dict(atom_messages=True, activation='ELU'), 0.3, 0),
    ('polymer', 8, 70, 3, dict(undirected=True, activation='tanh', aggregation='sum'), 0.1, 0),  # scalar epilogues
    ('polymer', 8, 48, 3, dict(atom_descriptors='descriptor', atom_descriptors_size=12), 0.25, 12),  # site depth + 1
    ('polymer', 8, 64, 2, {}, 0.25, 0),                               # site 1 feeds W_o directly
    ('edge', 9, 64, 3, dict(bias=True), 0.4, 0),
    ('polymer', 3, 2624, 2, {}, 0.2, 0),                              # Hk 2624 > RO_ACT_MAXLD: unfused readout backward
]


def _case(kind, b, hidden, depth, extra, p, desc_size):
    """(graph, args, descriptors or None) of one case-table row."""
    mols = synthetic.edge_case_batch(b, star_leaves=130) if kind == 'edge' else synthetic.make_batch(kind, b, 700 + b)
    args = TrainArgs(hidden_size=hidden, depth=depth, dropout=p, **extra)
    desc = synthetic.random_descriptors(mols, desc_size, 3) if desc_size else None
    return BatchMolGraph(mols), args, desc


def _encoder(args, fill_seed):
    enc = MPNEncoder(args, get_atom_fdim(), get_bond_fdim(atom_messages=args.atom_messages))
    synthetic.fill_parameters(enc, fill_seed)
    cpu = {n: t.detach().clone() for n, t in enc.named_parameters()}
    trainable = {n for n, t in enc.named_parameters() if t.requires_grad}
    return enc, cpu, trainable


def _out_grad(graph, args, desc_size, seed):
    return torch.randn((len(graph.a_scope), args.hidden_size + desc_size), generator=torch.Generator().manual_seed(seed))


def _ref_grads(cpu, trainable, graph, args, desc, R, dtype, kinks, drop):
    """(output, {name: gradient of sum(output * R)}) of the oracle in ``dtype``, as numpy."""
    p = {n: t.detach().clone().to(dtype).requires_grad_(n in trainable) for n, t in cpu.items()}
    out = mpn_ref.encoder_forward(p, graph, args, desc, dtype=None if dtype == torch.float32 else dtype, masks=kinks,
                                  drop=drop)
    (out * R.to(dtype)).sum().backward()
    return out.detach().numpy(), {n: t.grad.numpy() for n, t in p.items() if t.grad is not None}


def _show(tag, errs):
    print(f'\n{tag}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))


# ---------------------------------------------------------------------------------------------------
# E. CPU: the reference itself
# ---------------------------------------------------------------------------------------------------
@pytest.fixture
def one_thread():
    """torch's multithreaded CPU backward sums in an order that varies from call to call (the oracle's own fp32
    gradients then differ between two identical runs): bitwise comparisons run on one thread."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_all_ones_masks_are_bitwise_no_dropout(one_thread):
    graph, args, desc = _case(*A_CASES[5])
    _, cpu, trainable = _encoder(args, 3)
    R = _out_grad(graph, args, 12, 3)
    ones = ones_like_masks(graph_masks(SEED, 0.25, graph, args, 12))
    assert set(ones) == {'M', 'o', 'd'} and len(ones['M']) == args.depth - 1
    for dtype in (torch.float32, torch.float64):
        o0, g0 = _ref_grads(cpu, trainable, graph, args, desc, R, dtype, None, None)
        o1, g1 = _ref_grads(cpu, trainable, graph, args, desc, R, dtype, None, ones)
        assert np.array_equal(o0, o1)
        assert g0.keys() == g1.keys() and all(np.array_equal(g0[n], g1[n]) for n in g0)


def test_reference_rejects_masks_of_the_wrong_shape():
    graph, args, _ = _case(*A_CASES[0])
    _, cpu, _ = _encoder(args, 3)
    drop = graph_masks(SEED, 0.25, graph, args)
    with pytest.raises(ValueError):
        mpn_ref.encoder_forward(cpu, graph, args, drop=dict(drop, M=drop['M'][:1]))
    with pytest.raises(ValueError):
        mpn_ref.encoder_forward(cpu, graph, args, drop=dict(drop, o=drop['o'][:-1]))


@pytest.mark.parametrize('case', [0, 1, 3])
def test_fp32_reference_with_masks_is_well_inside_the_bar(case):
    """The fp32 oracle with masks against the fp64 one, outputs and gradients: within 2e-6 normwise, so the
    reference's own rounding sits a factor of five or more inside the 1e-5 bar (measured: <= 1.1e-6)."""
    graph, args, desc = _case(*A_CASES[case])
    p = A_CASES[case][5]
    _, cpu, trainable = _encoder(args, 5)
    R = _out_grad(graph, args, 0, 5)
    drop = graph_masks(SEED + case, p, graph, args)
    assert all(0 < int((m == 0).sum()) < m.numel() for m in drop['M'] + [drop['o']])
    o32, g32 = _ref_grads(cpu, trainable, graph, args, desc, R, torch.float32, None, drop)
    o64, g64 = _ref_grads(cpu, trainable, graph, args, desc, R, torch.float64, None, drop)
    errs = {'output': golden_io.normwise(o32, o64)}
    errs.update({n: golden_io.normwise(g32[n], g64[n]) for n in g64})
    _show(f'fp32 vs fp64 reference, case {case + 1}', errs)
    assert g32.keys() == g64.keys()
    assert all(e <= 2e-6 for e in errs.values()), errs
    o_plain, g_plain = _ref_grads(cpu, trainable, graph, args, desc, R, torch.float64, None, None)
    assert golden_io.normwise(o_plain, o64) > MATTER
    assert all(golden_io.normwise(g_plain[n], g64[n]) > MATTER for n in g64)


def test_dropout_seed_follows_manual_seed_and_rank(monkeypatch):
    G, M = 0x9E3779B97F4A7C15, (1 << 64) - 1
    torch.manual_seed(11)
    draw = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(11)
    a, b = mpn._dropout_seed(), mpn._dropout_seed()
    assert a == draw and b != a  # (no process group: the draw itself; the next call draws afresh)
    torch.manual_seed(11)
    assert (mpn._dropout_seed(), mpn._dropout_seed()) == (a, b)
    seeds = []
    monkeypatch.setattr(torch.distributed, 'is_available', lambda: True)
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    for rank in (0, 1):
        monkeypatch.setattr(torch.distributed, 'get_rank', lambda rank=rank: rank)
        torch.manual_seed(11)
        seeds.append(mpn._dropout_seed())
        assert seeds[-1] == draw ^ ((rank + 1) * G & M)
        assert 0 <= seeds[-1] <= M
    assert seeds[0] != seeds[1]


# ---------------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------------
def _seeded(s):
    """The seed the next training-mode forward draws; leaves torch's generator where that forward needs it."""
    torch.manual_seed(s)
    seed = mpn._dropout_seed()
    torch.manual_seed(s)
    return seed


def _ws_bytes(enc, g, variant=None, n_blocks=None):
    """wdmpnn_workspace_bytes of ``enc``'s no-grad forward on ``g``, optionally under another gemm_variant or
    with the graph's molecule blocks withheld (``n_blocks=0``).  Draws a dropout seed: call it before
    :func:`_seeded`."""
    from chemprop_amd import _native
    dg = g.device_graph(DEV, enc.atom_messages, enc.bond_fdim, not enc.bias)
    gs = _native.WdGraph.from_buffer_copy(enc._graph_struct(dg))
    if n_blocks is not None:
        gs.n_blocks = n_blocks
    old = enc._gemm_variant
    if variant is not None:
        enc._gemm_variant = variant
    cfg = enc._config(False)
    enc._gemm_variant = old
    params = tuple(t.detach().float() if t is not None else None for t in enc._param_tuple())
    pstruct, _ = enc._packed_params(gs, cfg, params, DEV)
    n = ctypes.c_size_t()
    _native.check(_native.lib().wdmpnn_workspace_bytes(ctypes.byref(gs), ctypes.byref(pstruct), ctypes.byref(cfg),
                                                       ctypes.byref(n)), 'workspace')
    return n.value


def _runs_blocked(enc, g):
    """The no-grad forward takes the molecule-blocked fused path: its workspace differs from the same graph's
    with the blocks withheld (as test_gpu_parity._runs_blocked)."""
    return _ws_bytes(enc, g) != _ws_bytes(enc, g, n_blocks=0)


def _lays_out_pairs(enc, g):
    """The workspace holds fp16 pair tiles unless the register-staged variant is asked for (as
    test_early_copies_gpu._selects_pairs)."""
    from chemprop_amd import _native
    return _ws_bytes(enc, g, _native.VARIANT_PAIRS) != _ws_bytes(enc, g, _native.VARIANT_STAGED)


# ---------------------------------------------------------------------------------------------------
# A. training forward + native backward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('kind,b,hidden,depth,extra,p,desc_size', A_CASES,
                         ids=[f'case{i + 1}' for i in range(len(A_CASES))])
def test_training_forward_and_backward_vs_fp64(kind, b, hidden, depth, extra, p, desc_size):
    graph, args, desc = _case(kind, b, hidden, depth, extra, p, desc_size)
    enc, cpu, trainable = _encoder(args, b)
    R = _out_grad(graph, args, desc_size, b)
    enc = enc.to(DEV).train()
    seed = _seeded(1000 + b)
    out = enc(graph, desc)
    assert out.grad_fn.cfg.seed == seed and out.grad_fn.cfg.dropout == pytest.approx(p)
    saved = mpn.saved_preactivations(out)
    kinks = {'Z': [z.cpu() > 0 for z in saved['Z']], 'Zo': saved['Zo'].cpu() > 0}
    (out * R.to(DEV)).sum().backward()
    hip = {'output': out.detach().cpu().numpy()}
    hip.update({n: t.grad.cpu().numpy() for n, t in enc.named_parameters() if t.grad is not None})
    drop = graph_masks(seed, p, graph, args, desc_size)
    with torch.no_grad():
        ref32 = mpn_ref.encoder_forward(cpu, graph, args, desc, drop=drop).numpy()
    _, ref64 = _ref_grads(cpu, trainable, graph, args, desc, R, torch.float64, kinks, drop)
    errs = {'output': golden_io.normwise(hip['output'], ref32)}
    for n, r in ref64.items():
        assert n in hip, f'missing gradient {n}'
        errs[n] = golden_io.normwise(hip[n], r)
    _show(f'A case H{hidden} d{depth} p{p} {extra}', errs)
    assert all(np.isfinite(v).all() for v in hip.values())
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    assert not bad, bad
    # the masks matter: the same references without them are far away
    with torch.no_grad():
        plain32 = mpn_ref.encoder_forward(cpu, graph, args, desc).numpy()
    _, plain64 = _ref_grads(cpu, trainable, graph, args, desc, R, torch.float64, kinks, None)
    assert golden_io.normwise(plain32, ref32) > MATTER
    for n, r in ref64.items():
        assert golden_io.normwise(plain64[n], r) > MATTER, n


# ---------------------------------------------------------------------------------------------------
# B. no-grad forward in .train(): the molecule-blocked fused forward and its fallbacks
# ---------------------------------------------------------------------------------------------------
def _hub():
    return synthetic.edge_case_batch(9, star_leaves=130)


B_CASES = [
    # (molecules, hidden, depth, options, gemm_variant, path)
    pytest.param(('polymer', 8), 300, 3, {}, 13, 'pairs', id='pairs-d3'),
    pytest.param(('polymer', 8), 300, 4, {}, 13, 'pairs', id='pairs-d4'),
    pytest.param(('polymer', 8), 300, 3, {}, 12, 'staged', id='staged-d3'),
    pytest.param(('polymer', 8), 300, 4, {}, 12, 'staged', id='staged-d4'),
    pytest.param(('polymer', 8), 64, 3, {}, 0, 'blocked', id='h64'),
    pytest.param(('polymer', 8), 64, 3, dict(atom_messages=True), 0, 'blocked', id='atom-blocked'),
    pytest.param(('polymer', 8), 64, 3, dict(atom_messages=True, bias=True), 0, 'unblocked', id='atom-bias-unblocked'),
    pytest.param(('hub', 9), 64, 3, dict(bias=True), 0, 'unblocked', id='hub-fallback'),
    pytest.param(('qm9', 32), 300, 3, {}, 0, 'small', id='qm9-off-one-launch'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('mols,hidden,depth,extra,variant,path', B_CASES)
def test_no_grad_training_forward_vs_fp64(mols, hidden, depth, extra, variant, path):
    kind, b = mols
    graph = BatchMolGraph(_hub() if kind == 'hub' else synthetic.make_batch(kind, b, 800 + b),
                          device_bond_features=not extra.get('atom_messages', False))
    for p in (0.25, 0.5):
        args = TrainArgs(hidden_size=hidden, depth=depth, dropout=p, **extra)
        enc, cpu, _ = _encoder(args, 12)
        enc = enc.to(DEV).train()
        enc._gemm_variant = variant
        # the intended path
        assert _runs_blocked(enc, graph) == (path != 'unblocked')
        if not args.atom_messages:
            assert _lays_out_pairs(enc, graph) == (path in ('pairs', 'staged', 'small'))
        if path == 'small':  # inside the one-launch forward's domain but for the dropout
            st = graph.device_graph(DEV, False, enc.bond_fdim).struct
            assert 0 < st.blk_max_bonds <= 32 and st.blk_max_atoms <= 32
        seed = _seeded(2000 + b)
        with torch.no_grad():
            out = enc(graph)
        assert out.grad_fn is None and torch.isfinite(out).all()
        p64 = {n: t.double() for n, t in cpu.items()}
        with torch.no_grad():
            ref = mpn_ref.encoder_forward(p64, graph, args, dtype=torch.float64,
                                          drop=graph_masks(seed, p, graph, args)).numpy()
            plain = mpn_ref.encoder_forward(p64, graph, args, dtype=torch.float64).numpy()
        err = golden_io.normwise(out.cpu().numpy(), ref)
        _show(f'B {kind}{b} H{hidden} d{depth} v{variant} {extra} p{p}', {'output': err})
        assert err <= TOL, (p, err)
        assert golden_io.normwise(plain, ref) > MATTER  # (a forward that dropped nothing would be this far off)


@pytest.mark.gpu
@pytest.mark.parametrize('frozen', [False, True])
def test_frozen_forward_is_bitwise_the_no_grad_forward(frozen):
    """``_frozen_forward`` (the forward of a frozen encoder inside a fine-tuning step) draws the same seed and
    runs the same launches as the no-grad forward."""
    args = TrainArgs(hidden_size=300, depth=3, dropout=0.25)
    graph = BatchMolGraph(synthetic.make_batch('polymer', 8, 808), device_bond_features=True)
    enc, _, _ = _encoder(args, 12)
    enc = enc.to(DEV).train()
    if frozen:
        enc.requires_grad_(False)
    _seeded(31)
    with torch.no_grad():
        a = enc(graph)
    _seeded(31)
    b = enc._frozen_forward(graph)
    _seeded(32)
    c = enc._frozen_forward(graph)
    assert torch.equal(a, b) and not torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------
# C. exact mask placement at the W_o site
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('leaves', [20, 130])  # the hub fits a block / exceeds it (unblocked no-grad fallback)
def test_single_atom_molecules_show_the_w_o_mask_exactly(leaves):
    """A single-atom molecule's encoding is its atom's dropout(tanh(Zo)) row times positive factors, and tanh of
    a biased pre-activation is never 0: the output is 0 exactly where the W_o site's mask is, on the
    grad-enabled and on the no-grad path."""
    rng = np.random.default_rng(3)
    mols = synthetic.edge_case_batch(9, star_leaves=leaves) + [synthetic.single_atom_graph(rng) for _ in range(2)]
    graph = BatchMolGraph(mols)
    singles = [(i, a0) for i, (a0, n) in enumerate(graph.a_scope) if n == 1]
    assert len(singles) == 3
    H, depth, p = 64, 3, 0.4
    args = TrainArgs(hidden_size=H, depth=depth, dropout=p, activation='tanh', bias=True)
    enc, _, _ = _encoder(args, 5)
    enc = enc.to(DEV).train()
    assert _runs_blocked(enc, graph) == (leaves == 20)
    for no_grad in (False, True):
        seed = _seeded(77)
        with torch.set_grad_enabled(not no_grad):
            out = enc(graph).detach().cpu().numpy()
        mask = dropout_mask(seed, depth, graph.n_atoms, H, p)
        for i, atom in singles:
            assert 0 < (mask[atom] == 0).sum() < H
            assert np.array_equal(out[i] == 0, mask[atom] == 0), (no_grad, i)


# ---------------------------------------------------------------------------------------------------
# D. one whole step: encoder and head masks, the order of the draws
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_step_with_encoder_and_head_dropout_vs_fp64():
    from chemprop_amd.model import MoleculeModel
    from chemprop_amd.train import _StackHead, _fusable_head, get_loss_func, head_loss
    B, H, depth, Hf, tasks, p = 8, 64, 3, 40, 2, 0.2
    args = TrainArgs(hidden_size=H, depth=depth, ffn_num_layers=3, ffn_hidden_size=Hf, dropout=p, device=DEV,
                     dataset_type='regression')
    args.num_tasks = tasks
    graph = BatchMolGraph(synthetic.make_batch('polymer', B, 39))
    rng = np.random.default_rng(B)
    targets = [[None if rng.random() < 0.25 else float(rng.normal()) for _ in range(tasks)] for _ in range(B)]
    targets[0][0], targets[1][1] = None, 0.5  # (at least one missing, at least one present)
    tw = list(rng.uniform(0.5, 1.5, tasks))
    dw = list(rng.uniform(0.5, 1.5, B))
    m = MoleculeModel(args)
    synthetic.fill_parameters(m, 17)
    cpu = {n: t.detach().clone() for n, t in m.named_parameters()}
    m = m.to(DEV).train()
    head = _fusable_head(m, get_loss_func('regression'), 'regression')
    assert isinstance(head, _StackHead) and head.p == pytest.approx(p) and len(head.linears) == 3

    torch.manual_seed(5)
    s_enc, s_head = mpn._dropout_seed(), mpn._dropout_seed()  # the encoder draws first, then the head
    torch.manual_seed(5)
    emb = m.encoder([graph])
    assert emb.grad_fn.cfg.seed == s_enc
    saved = mpn.saved_preactivations(emb)
    kinks = {'Z': [z.cpu() > 0 for z in saved['Z']], 'Zo': saved['Zo'].cpu() > 0}
    loss = head_loss(emb, head, targets, tw, dw)
    loss.backward()
    hip = {n: t.grad.cpu().numpy() for n, t in m.named_parameters() if t.grad is not None}

    pre = 'encoder.encoder.0.'
    p64 = {n: t.double().requires_grad_(t.dtype.is_floating_point and n != pre + 'cached_zero_vector')
           for n, t in cpu.items()}
    a = mpn_ref.encoder_forward({n[len(pre):]: t for n, t in p64.items() if n.startswith(pre)}, graph, args,
                                dtype=torch.float64, masks=kinks, drop=graph_masks(s_enc, p, graph, args))
    lin = sorted({int(n.split('.')[1]) for n in p64 if n.startswith('ffn.')})
    assert len(lin) == 3
    for site, i in enumerate(lin):  # head site l masks the input of Linear l + 1
        a = a * torch.from_numpy(dropout_mask(s_head, site, B, a.shape[1], p)).double()
        a = torch.nn.functional.linear(a, p64[f'ffn.{i}.weight'], p64[f'ffn.{i}.bias'])
        if site < len(lin) - 1:
            a = torch.relu(a)
    y = torch.tensor([[0.0 if v is None else v for v in row] for row in targets], dtype=torch.float64)
    present = np.array([[v is not None for v in row] for row in targets])
    w = torch.from_numpy((np.asarray(tw)[None, :] * np.asarray(dw)[:, None] * present).astype(np.float32)).double()
    ref_loss = ((a - y.float().double()) ** 2 * w).sum() / float(present.sum())
    ref_loss.backward()
    ref = {n: t.grad.numpy() for n, t in p64.items() if t.grad is not None}

    errs = {'loss': abs(float(loss.detach()) - float(ref_loss.detach())) / abs(float(ref_loss.detach()))}
    assert ref.keys() == hip.keys(), sorted(set(ref) ^ set(hip))
    errs.update({n: golden_io.normwise(hip[n], ref[n]) for n in ref})
    _show('D whole step', errs)
    assert all(np.isfinite(v).all() for v in hip.values())
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    assert not bad, bad
