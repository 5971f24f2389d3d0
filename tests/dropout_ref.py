"""The encoder's dropout masks for ``oracle.mpn_ref.encoder_forward(drop=...)``, built from the contract
``chemprop_amd.nn_utils.dropout_mask`` with the encoder's site numbering (DESIGN.md "Dropout sites"):
site t masks the t-th W_h update (t = 1 .. depth - 1), site depth the W_o output, site depth + 1 the
descriptor layer; rows are natural rows including the pad row 0, columns the hidden column."""
import torch

from chemprop_amd.nn_utils import dropout_mask


def encoder_masks(seed: int, p: float, depth: int, rows: int, n_atoms: int, H: int, desc: int = 0) -> dict:
    """``rows`` = message rows (bond rows, or atom rows in atom-message mode), ``n_atoms`` = atom rows, both with
    the pad row; ``desc`` = atom descriptor size (0: no descriptor layer, no 'd' mask)."""
    drop = {'M': [torch.from_numpy(dropout_mask(seed, t, rows, H, p)) for t in range(1, depth)],
            'o': torch.from_numpy(dropout_mask(seed, depth, n_atoms, H, p))}
    if desc:
        drop['d'] = torch.from_numpy(dropout_mask(seed, depth + 1, n_atoms, H + desc, p))
    return drop


def graph_masks(seed: int, p: float, graph, args, desc: int = 0) -> dict:
    """:func:`encoder_masks` for ``graph`` under the encoder arguments ``args``."""
    rows = graph.n_atoms if args.atom_messages else graph.n_bonds
    return encoder_masks(seed, p, args.depth, rows, graph.n_atoms, args.hidden_size, desc)


def ones_like_masks(drop: dict) -> dict:
    return {k: [torch.ones_like(m) for m in v] if isinstance(v, list) else torch.ones_like(v) for k, v in drop.items()}
