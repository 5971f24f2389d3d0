"""Extra atom / bond features against the REAL reference: tests/golden/extra_features/enc_extra_features.npz
(tools/make_goldens.py ``enc_extra_features``: the reference's BatchMolGraph and MPNEncoder with
``set_extra_atom_fdim(3)`` / ``set_extra_bond_fdim(2)`` on widened synthetic graphs).  CPU: the oracle, unchanged,
reproduces the reference on widened rows, and the host packing equals the reference's.  GPU: the native forward
and gradients on the device-built graph meet the reference's own numbers."""
import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import synthetic
from chemprop_amd.mpn import MPNEncoder
from oracle import mpn_ref

NAME = 'extra_features/enc_extra_features'
TOL = 1e-5


@pytest.fixture(scope='module')
def case():
    return golden_io.load(NAME)


def _module(case):
    enc = MPNEncoder(case.args, 136, 152)
    synthetic.fill_parameters(enc, case.seed)
    return enc.eval()


def test_fixture_is_the_widened_case(case):
    z = np.load(golden_io.GOLDEN_DIR + '/' + NAME + '.npz', allow_pickle=False)
    assert z['extra_dims'].tolist() == [3, 2] and case.level == 'encoder'
    g = case.graphs[0]
    assert len(case.mol_lists[0]) == 4 and g.f_atoms.shape[1] == 136 and g.f_bonds.shape[1] == 152
    assert (case.args.hidden_size, case.args.depth, case.args.bias) == (32, 3, True)
    assert g._compact is not None and g._compact_extra[2:] == (3, 2), g._compact_why
    x = np.concatenate([g.f_atoms.numpy()[:, 133:].ravel(), g.f_bonds.numpy()[:, 150:].ravel()])
    assert (x < 0).any() and (np.abs(x) == 1e3).any() and ((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)).any()
    ref = case.packed[0]
    np.testing.assert_array_equal(g.a2b.numpy(), ref['a2b'])
    np.testing.assert_array_equal(g.b2a.numpy(), ref['b2a'])
    np.testing.assert_array_equal(g.b2revb.numpy(), ref['b2revb'])
    assert [n for n, _ in _module(case).named_parameters()] == case.param_names


def test_oracle_matches_the_reference_on_widened_rows(case):
    enc = _module(case)
    p = {n: t.detach().clone().requires_grad_(t.requires_grad) for n, t in enc.named_parameters()}
    out = mpn_ref.encoder_forward(p, case.graphs[0], case.args)
    assert out.shape == case.output.shape
    assert golden_io.normwise(out.detach().numpy(), case.output) <= TOL
    (out * torch.from_numpy(case.R)).sum().backward()
    assert set(case.grads) >= {'W_i.weight', 'W_h.weight', 'W_o.weight'} and case.grads['W_i.weight'].shape == (32, 152)
    for n, g in case.grads.items():
        err = golden_io.normwise(p[n].grad.numpy(), g)
        assert err <= TOL, (n, err)


@pytest.mark.gpu
def test_native_forward_and_gradients_match_the_reference(case):
    dev = torch.device('cuda:0')
    enc = _module(case).to(dev)
    g = case.graphs[0]
    with torch.no_grad():
        out = enc(g)
    assert g.device_graph(dev, False, 152).built_on_device
    assert golden_io.normwise(out.cpu().numpy(), case.output) <= TOL
    out = enc.train()(g)
    assert golden_io.normwise(out.detach().cpu().numpy(), case.output) <= TOL
    (out * torch.from_numpy(case.R).to(dev)).sum().backward()
    for n, t in enc.named_parameters():
        if n in case.grads:
            err = golden_io.normwise(t.grad.cpu().numpy(), case.grads[n])
            assert err <= TOL, (n, err)
