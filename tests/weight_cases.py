"""Shared by test_weight_paths_ref.py (CPU) and test_weight_paths_gpu.py: the encoder configurations of
every forward path, the per-molecule error against the fp64 oracle, and the edits of one molecule of
``synthetic.weight_case_batch`` that the exact-property tests make."""
import copy
import functools

import numpy as np
import torch

from chemprop_amd import TrainArgs, synthetic
from chemprop_amd.featurization import BatchMolGraph, get_atom_fdim, get_bond_fdim
from chemprop_amd.mpn import MPNEncoder
from oracle import mpn_ref

SEED = 33       # the family's seed (tests/golden/enc_weights_h300_t3.npz holds the same batch)
PARAM_SEED = 17
ROW_TOL = 1e-5  # the parity bar, applied per molecule: max|out - ref64| <= 1e-5 max|ref64| per row
ORACLE_ROOM = 2e-6  # what the fp32 oracle itself must meet per row (measured: see test_weight_paths_ref.py)
TRI = 1         # the three-atom molecule whose last rule pair has weights (0, 0)

# path -> (hidden, depth, TrainArgs extras, WdConfig.gemm_variant, grad-enabled call)
PATHS = {
    'one_launch': (300, 3, dict(bias=True), 0, False),                      # small_fwd.hpp
    'staged_v12': (300, 3, dict(bias=True), 12, False),                     # four launches, register-staged layers
    'pairs_v13': (300, 4, dict(activation='LeakyReLU'), 13, False),         # four launches, fp16 pair tiles
    'f32_mfma_v9': (300, 2, dict(activation='tanh', bias=True), 9, False),
    'hidden64': (64, 3, dict(activation='ELU', bias=True), 0, False),       # 64-column tiles
    'grad': (300, 3, dict(activation='PReLU', bias=True), 0, True),         # the training forward (unblocked)
    'depth1': (300, 1, dict(), 0, False),
    'undirected': (300, 3, dict(undirected=True, activation='SELU'), 0, False),
    'atom_nobias': (64, 3, dict(atom_messages=True), 0, False),             # molecule-blocked atom messages
    'atom_bias': (64, 3, dict(atom_messages=True, bias=True), 0, False),    # unblocked atom messages
}
BOND_PATHS = [k for k, v in PATHS.items() if not v[2].get('atom_messages')]


def path_args(path, aggregation=None):
    hidden, depth, extra, variant, grad = PATHS[path]
    extra = dict(extra, **({'aggregation': aggregation} if aggregation else {}))
    return TrainArgs(hidden_size=hidden, depth=depth, **extra), variant, grad


def new_encoder(args):
    enc = MPNEncoder(args, get_atom_fdim(), get_bond_fdim(atom_messages=args.atom_messages))
    synthetic.fill_parameters(enc, PARAM_SEED)
    return enc


def family():
    return synthetic.weight_case_batch(SEED)


def oracle(args, mols, dtype=None):
    """mpn_ref.encoder_forward on the CPU with the parameters of ``new_encoder`` (fp32, or ``dtype``)."""
    p = {n: t.detach().clone() if dtype is None else t.detach().to(dtype) for n, t in new_encoder(args).named_parameters()}
    with torch.no_grad():
        return mpn_ref.encoder_forward(p, BatchMolGraph(mols), args, dtype=dtype)


@functools.lru_cache(maxsize=None)
def family_ref64(path, aggregation=None):
    """The fp64 oracle's output of ``path``'s configuration on the family: computed once, never written."""
    return oracle(path_args(path, aggregation)[0], family(), torch.float64)


def row_errors(out, ref64):
    """max|out - ref64| / max|ref64| per molecule."""
    ref64 = ref64.double()
    return ((out.double() - ref64).abs().max(dim=1).values / ref64.abs().max(dim=1).values).tolist()


def double_xn(mols, m):
    """A copy of ``mols`` with molecule m's float32 degree_of_polym doubled."""
    mols = list(mols)
    mols[m] = copy.copy(mols[m])
    mols[m].degree_of_polym = 2.0 * float(np.float32(mols[m].degree_of_polym))
    return mols


def double_w_atoms(mols, m):
    """A copy of ``mols`` with the float32 atom weights of molecule m doubled."""
    mols = list(mols)
    mols[m] = copy.copy(mols[m])
    mols[m].w_atoms = [2.0 * float(np.float32(w)) for w in mols[m].w_atoms]
    return mols


def drop_last_pair(mols, m):
    """A copy of ``mols`` without the last bond pair of molecule m, cut from the built graph's arrays: no
    new random draws, the same f_atoms, no other bond renumbered."""
    g = copy.copy(mols[m])
    last = {g.n_bonds - 2, g.n_bonds - 1}
    assert {g.b2revb[b] for b in last} == last
    g.f_bonds, g.w_bonds, g.b2a, g.b2revb = g.f_bonds[:-2], g.w_bonds[:-2], g.b2a[:-2], g.b2revb[:-2]
    g.a2b = [[b for b in row if b not in last] for row in g.a2b]
    g.n_bonds -= 2
    mols = list(mols)
    mols[m] = g
    return mols


def chain(rng, n_atoms, k):
    """n_atoms in a chain of RULE pairs (2 (n_atoms - 1) bond rows) with fractional weights, distinct atom
    weights and Xn != 1; ``k`` tells the molecules of a batch apart."""
    rules = [(i, i + 1, 0.2 + 0.013 * ((7 * i + k) % 53), 1.0 if (i + k) % 4 == 0 else 0.9 - 0.011 * ((5 * i + k) % 47))
             for i in range(n_atoms - 1)]
    w_atoms = [0.15 + 0.017 * ((3 * i + 11 * k) % 41) for i in range(n_atoms)]
    return synthetic._build(rng, n_atoms, set(), rules, w_atoms, 1.25 + 0.0625 * (k % 23))


def block_edge_batches():
    """name -> (molecules, block_target, (bond rows, atoms, molecules) of the block in question, one launch?):
    the block shapes on either side of every limit of the one-launch dispatch (32 bond rows, 32 atoms, one
    and two 16-row groups, a block without bond rows)."""
    rng = np.random.default_rng(91)
    single = lambda k: chain(rng, 1, k)  # noqa: E731
    pairs16 = [chain(rng, 2, k) for k in range(16)]
    return {
        # 64 molecules fill a block (20 single atoms, 44 empty molecules): no bond rows; the chain follows
        'no_bond_rows': ([single(k) for k in range(20)] + [synthetic.empty_graph() for _ in range(44)] + [chain(rng, 5, 0)],
                         64, (0, 20, 64), True),
        'rows16': ([chain(rng, 9, 1), single(2)], 64, (16, 10, 2), True),
        'rows18': ([single(3), chain(rng, 10, 2)], 64, (18, 11, 2), True),
        'rows32_atoms17': ([chain(rng, 17, 3)], 64, (32, 17, 1), True),
        'rows32_atoms32': (pairs16, 1, (32, 32, 16), True),
        'rows32_atoms33': (pairs16 + [single(4)], 1, (32, 33, 17), False),
        'rows34': ([chain(rng, 18, 5)], 64, (34, 18, 1), False),
    }
