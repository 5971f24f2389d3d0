"""GPU: bond weights, atom weights and Xn at their special values (0, 1, above 1) and the block edges of the
one-launch dispatch, on every forward path of the encoder (tests/weight_cases.py ``PATHS``), on the family
``synthetic.weight_case_batch`` (14 molecules, each within the one-launch forward's 32 bond rows / 32 atoms).

The bar is the project's parity bar applied PER MOLECULE: max|out - ref64| <= 1e-5 max|ref64| on every row,
against ``mpn_ref.encoder_forward(dtype=float64)`` -- a whole-batch normwise error hides one molecule's
dropped tail term behind the other rows.  The fp32 oracle itself (the reference's own arithmetic) stays
1.9e-7 .. 4.9e-7 from the fp64 one on its worst row over the ten paths x three aggregations
(test_weight_paths_ref.py asserts <= 2e-6), so the bar leaves the kernels 20x the reference's own error.

Exact properties need no reference: doubling one molecule's float32 Xn doubles exactly its row; doubling
its atom weights leaves its row alone under ``mean`` and doubles it under ``sum`` / ``norm`` (fmaf chains
and lane trees scale exactly by 2); a rule pair with weights (0, 0) is inert for bond messages.

Arithmetic-only mutations of a scratch build that these tests caught (each with no index change): coefficient
1.0 in the CSR tail of the one-launch atom sums (small_fwd.hpp ``sf_atom_sum``); ``w`` stored in place of
``w - 1`` for the reverse bond by the device graph builder (graph_build.hpp ``build_structure``); Xn read as
1 in the one-launch readout.
"""
import copy

import pytest
import torch

import weight_cases as wc
from chemprop_amd import TrainArgs, synthetic
from chemprop_amd.featurization import BatchMolGraph, get_atom_fdim, get_bond_fdim
from chemprop_amd.mpn import MPNEncoder
from test_gpu_parity import _check, _oracle_vs_hip, _runs_blocked

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
_ENCODERS = {}


def _encoder(path, agg=None):
    """The encoder of ``path`` (and aggregation) on the device, made once."""
    enc = _ENCODERS.get((path, agg))
    if enc is None:
        args, variant, _ = wc.path_args(path, agg)
        enc = wc.new_encoder(args).to(DEV).eval()
        enc._gemm_variant = variant
        _ENCODERS[(path, agg)] = enc
    return enc


def _forward(path, g, agg=None):
    with torch.set_grad_enabled(wc.PATHS[path][4]):
        out = _encoder(path, agg)(g)
    return out.detach().cpu()


def _one_launch_domain(g):
    s = g.device_graph(DEV, False, get_bond_fdim()).struct
    return 0 < s.blk_max_bonds <= 32 and s.blk_max_atoms <= 32


@pytest.mark.parametrize('path', sorted(wc.PATHS))
def test_per_molecule_accuracy_on_every_forward_path(path):
    g = BatchMolGraph(wc.family())
    enc = _encoder(path)
    if enc.atom_messages:
        assert _runs_blocked(enc, g) == (path == 'atom_nobias')
    else:
        assert _one_launch_domain(g)
        assert g.device_graph(DEV, False, get_bond_fdim()).built_on_device
    err = wc.row_errors(_forward(path, g), wc.family_ref64(path))
    print(path, 'per-molecule errors', ' '.join(f'{e:.1e}' for e in err))
    assert max(err) <= wc.ROW_TOL, err


@pytest.mark.parametrize('target,reverse', [(None, False), (16, True)])
@pytest.mark.parametrize('agg', ['mean', 'sum', 'norm'])
def test_one_launch_is_bitwise_the_register_staged_forward(agg, target, reverse):
    """The one-launch forward equals the four-launch forward with register-staged layers (variant 12)
    bitwise on the family.  The family's largest molecule has 32 bond rows, so every plan of at least 8
    blocks fills blocks to 32 rows: the default plan already has molecules 0 - 4 in one full block
    (32 rows, 17 atoms, 5 molecules); block_target=16 on the reversed batch groups other molecules."""
    mols = wc.family()[::-1] if reverse else wc.family()
    g = BatchMolGraph(mols) if target is None else BatchMolGraph(mols, block_target=target)
    blocks = g.molecule_blocks()
    assert blocks[:, 1].max() == 32 and blocks[:, 3].max() <= 32 and (blocks[:, 5] - blocks[:, 4]).max() >= 3
    if not reverse:
        assert blocks[0].tolist()[:6] == [1, 32, 1, 17, 0, 5]
    assert _one_launch_domain(g)
    one, four = _forward('one_launch', g, agg), _forward('staged_v12', g, agg)
    assert torch.equal(one, four), float((one - four).abs().max())
    ref = wc.family_ref64('one_launch', agg)
    err = wc.row_errors(one, ref.flip(0) if reverse else ref)
    assert max(err) <= wc.ROW_TOL, err


@pytest.mark.parametrize('name', sorted(wc.block_edge_batches()))
def test_block_edges_of_the_one_launch_dispatch(name):
    """Blocks on either side of each limit of the one-launch forward: the plan has the named shape; shapes
    inside the limits equal variant 12 bitwise, shapes outside take the four-launch path; all meet the
    per-molecule bar (the fp32 oracle with room)."""
    mols, target, shape, one_launch = wc.block_edge_batches()[name]
    g = BatchMolGraph(mols, block_target=target)
    blocks = g.molecule_blocks()
    assert shape in [(int(b[1]), int(b[3]), int(b[5] - b[4])) for b in blocks]
    assert _one_launch_domain(g) == one_launch
    s = g.device_graph(DEV, False, get_bond_fdim()).struct
    assert (s.blk_max_bonds, s.blk_max_atoms) == (int(blocks[:, 1].max()), int(blocks[:, 3].max()))
    args = wc.path_args('one_launch')[0]
    ref64 = wc.oracle(args, mols, torch.float64)
    assert max(wc.row_errors(wc.oracle(args, mols), ref64)) <= wc.ORACLE_ROOM
    out = _forward('one_launch', g)
    err = wc.row_errors(out, ref64)
    print(name, f'worst row {max(err):.1e}')
    assert max(err) <= wc.ROW_TOL, err
    if one_launch:
        assert torch.equal(out, _forward('staged_v12', g))


@pytest.mark.parametrize('hidden,depth,extra', [
    (300, 3, dict(bias=True)),
    (64, 4, dict(activation='PReLU', aggregation='norm')),
    (64, 2, dict(undirected=True, aggregation='sum')),
])
def test_gradients_on_the_weight_cases(hidden, depth, extra):
    """Training forward and backward on the family (mp_layer_kernel, wo_readout_kernel and the backward's
    gather8_kernel walk the zero / unit-weight rows): every weight gradient within 1e-5 normwise of the
    fp64 evaluation."""
    args = TrainArgs(hidden_size=hidden, depth=depth, **extra)
    _check(_oracle_vs_hip(BatchMolGraph(wc.family()), args, seed=wc.PARAM_SEED))


@pytest.mark.parametrize('path', sorted(wc.PATHS))
def test_doubling_xn_doubles_exactly_that_row(path):
    mols = wc.family()
    base = _forward(path, BatchMolGraph(mols))
    for m in (0, 7):  # a molecule of the shared first block, and a hub alone in its block
        out = _forward(path, BatchMolGraph(wc.double_xn(mols, m)))
        others = [i for i in range(len(mols)) if i != m]
        assert torch.equal(out[m], 2 * base[m]), (m, float((out[m] - 2 * base[m]).abs().max()))
        assert torch.equal(out[others], base[others]), m


@pytest.mark.parametrize('agg', ['mean', 'sum', 'norm'])
@pytest.mark.parametrize('path', sorted(wc.PATHS))
def test_doubling_atom_weights(path, agg):
    """Molecule 0 (one atom weight exactly 0, block mates) and molecule 10 (17 atoms: three readout passes of
    eight lanes): the row is unchanged under mean and doubled under sum / norm, bitwise; no other row moves."""
    mols = wc.family()
    base = _forward(path, BatchMolGraph(mols), agg)
    for m in (0, 10):
        out = _forward(path, BatchMolGraph(wc.double_w_atoms(mols, m)), agg)
        want = base.clone()
        if agg != 'mean':
            want[m] *= 2
        assert torch.equal(out, want), (m, float((out - want).abs().max()))


@pytest.mark.parametrize('path', wc.BOND_PATHS)
def test_zero_weight_rule_pair_is_inert_in_the_forward(path):
    """The (0, 0) rule pair of the three-atom molecule, cut from the built graph: no other molecule's row
    changes at all (the block plan is the same, test_weight_paths_ref.py) and the molecule's own row moves
    by rounding only (1e-6 of its maximum: the bond rows after the cut move up by two, into other tiles and
    lanes).  Bond messages only: atom messages sum their neighbours unweighted (mpn.py:104-108)."""
    mols = wc.family()
    base = _forward(path, BatchMolGraph(mols))
    out = _forward(path, BatchMolGraph(wc.drop_last_pair(mols, wc.TRI)))
    others = [i for i in range(len(mols)) if i != wc.TRI]
    assert torch.equal(out[others], base[others])
    err = float((out[wc.TRI] - base[wc.TRI]).abs().max() / base[wc.TRI].abs().max())
    assert err <= 1e-6, err


def test_zero_weight_rule_pair_is_inert_in_the_gradients():
    """The same cut through the training path: every weight gradient agrees to 1e-6 normwise."""
    import golden_io
    mols = wc.family()
    args = wc.path_args('grad')[0]
    R = torch.randn((len(mols), args.hidden_size), generator=torch.Generator().manual_seed(3)).to(DEV)
    grads = []
    for batch in (mols, wc.drop_last_pair(mols, wc.TRI)):
        enc = wc.new_encoder(args).to(DEV)
        (enc(BatchMolGraph(batch)) * R).sum().backward()
        grads.append({n: t.grad.cpu().numpy() for n, t in enc.named_parameters() if t.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) >= 6
    err = {n: golden_io.normwise(grads[1][n], grads[0][n]) for n in grads[0]}
    assert max(err.values()) <= 1e-6, err


def test_prepare_in_training_mode_leaves_inference_without_dropout():
    """``prepare`` on a training-mode encoder with dropout caches inference plans; after ``.eval()`` a
    no-grad forward on the prepared graph must be the forward of a never-prepared copy, bitwise (the plan key
    has no training flag: the cached config must not carry the dropout)."""
    args = TrainArgs(hidden_size=300, depth=3, dropout=0.2)
    enc = MPNEncoder(args, get_atom_fdim(), get_bond_fdim())
    synthetic.fill_parameters(enc, 4)
    enc = enc.to(DEV).train()
    fresh = copy.deepcopy(enc).eval()
    g = BatchMolGraph(wc.family())
    enc.prepare([g])
    enc.eval()
    with torch.no_grad():
        out = enc(g)
        want = fresh(BatchMolGraph(wc.family()))
    assert torch.equal(out, want), float((out - want).abs().max())
