"""Molecules shared by the resident graph table's host and GPU tests: a pool with the block-limit and
bond-weight edge cases, built once."""
import functools

import numpy as np

from chemprop_amd import synthetic

# named positions of the pool
ONE_ATOM, ATOMS_64, BONDS_128, WEIGHTS, EMPTY = 0, 1, 2, 3, 4


@functools.lru_cache(maxsize=None)
def pool():
    """0: one atom, no bonds.  1: a chain of exactly 64 atoms (126 directed bonds).  2: 40 atoms and exactly 128
    directed bonds, the rule pairs' weights cycling through 0, 1 and 0.37 in both directions.  3: a small hub whose
    rule pairs carry the nine (w12, w21) combinations of 0, 1 and 0.37.  4: the empty molecule (host tests only).
    Then 12 polymers, 8 QM9-like molecules and the non-empty molecules of ``synthetic.weight_case_batch``."""
    rng = np.random.default_rng(77)
    vals = (0.0, 1.0, 0.37)
    chain64 = synthetic._build(rng, 64, {(i, i + 1) for i in range(63)}, [], [1.0] * 64, 2.5)
    rules = [(k % 40, (7 * k + 3) % 40, vals[k % 3], vals[(k // 3) % 3]) for k in range(25)]
    full = synthetic._build(rng, 40, {(i, i + 1) for i in range(39)}, rules,
                            [0.25 + 0.01 * i for i in range(40)], 1.75)
    assert chain64.n_atoms == 64 and full.n_bonds == 128
    nine = synthetic._build(rng, 10, {(0, 1)}, [(0, 1 + k, vals[k % 3], vals[k // 3]) for k in range(9)],
                            [0.1 * (i + 1) for i in range(10)], 3.0)
    mols = [synthetic.single_atom_graph(rng), chain64, full, nine, synthetic.empty_graph()]
    mols += synthetic.make_batch('polymer', 12, 5) + synthetic.make_batch('qm9', 8, 6)
    mols += [g for g in synthetic.weight_case_batch(12) if g.n_atoms]
    return mols


def gpu_pool():
    """The pool without the empty molecule (position 4 then holds the first polymer)."""
    return [g for g in pool() if g.n_atoms]
