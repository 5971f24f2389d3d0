"""CPU: what tests/test_weight_paths_gpu.py relies on.  The fp32 oracle itself meets the per-molecule bar
(max|out - ref64| <= 1e-5 max|ref64| per row) with room on ``synthetic.weight_case_batch`` in every
configuration the GPU tests run, the block plans have the shapes those tests name, and the edits of the
exact-property tests leave the block plan alone."""
import numpy as np
import pytest
import torch

import weight_cases as wc
from chemprop_amd.featurization import BatchMolGraph


@pytest.mark.parametrize('path', sorted(wc.PATHS))
def test_fp32_oracle_meets_the_per_molecule_bar_with_room(path):
    for agg in (None, 'sum', 'norm'):
        args = wc.path_args(path, agg)[0]
        err = wc.row_errors(wc.oracle(args, wc.family()), wc.family_ref64(path, agg))
        print(path, agg, f'worst row {max(err):.2e}')
        assert max(err) <= wc.ORACLE_ROOM, (agg, err)


def test_family_block_plans():
    """The default plan: no block above 32 bond rows / 32 atoms, molecules 0 - 4 in one full block; the
    reversed batch groups other molecules together."""
    mols = wc.family()
    assert len(mols) == 14
    for order in (mols, mols[::-1]):
        blocks = BatchMolGraph(order).molecule_blocks()
        assert blocks[:, 1].max() == 32 and blocks[:, 3].max() <= 32
        assert (blocks[:, 5] - blocks[:, 4]).max() >= 3
    blocks = BatchMolGraph(mols).molecule_blocks()
    assert blocks[0].tolist()[:6] == [1, 32, 1, 17, 0, 5]


def test_property_edits_keep_the_block_plan():
    mols = wc.family()
    base = BatchMolGraph(mols).molecule_blocks()
    cut = BatchMolGraph(wc.drop_last_pair(mols, wc.TRI))
    assert cut.n_bonds == BatchMolGraph(mols).n_bonds - 2
    assert np.array_equal(cut.molecule_blocks()[:, 4:6], base[:, 4:6])
    assert mols[wc.TRI].w_bonds[-2:] == [0.0, 0.0] and mols[wc.TRI].n_bonds == 10
    g2 = BatchMolGraph(wc.double_xn(wc.double_w_atoms(mols, 0), 6))
    assert np.array_equal(g2.molecule_blocks(), base)
    a0, n0 = g2.a_scope[0]
    assert torch.equal(g2.w_atoms[a0:a0 + n0], 2 * BatchMolGraph(mols).w_atoms[a0:a0 + n0])


@pytest.mark.parametrize('name', sorted(wc.block_edge_batches()))
def test_block_edge_batches_have_the_named_shape(name):
    mols, target, (rows, atoms, n_mols), one_launch = wc.block_edge_batches()[name]
    blocks = BatchMolGraph(mols, block_target=target).molecule_blocks()
    shapes = [(int(b[1]), int(b[3]), int(b[5] - b[4])) for b in blocks]
    assert (rows, atoms, n_mols) in shapes, shapes
    assert (0 < blocks[:, 1].max() <= 32 and blocks[:, 3].max() <= 32) == one_launch, shapes
