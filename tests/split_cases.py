"""Inputs, references and bounds shared by the split-operand term tests (test_split_ref.py on the CPU,
test_split_terms_gpu.py on the GPU): the same batches, probe weights, layerwise fp64 reference and elementwise
bound, so that what the CPU emulation shows about the bound -- the complete schemes stay under it, a scheme that
lost one product does not -- holds for the very numbers the GPU tests feed the kernels.

Probe weights.  W_h (and W_o[:, Fa:]) is a signed permutation matrix with full-mantissa nonzeros of magnitude
4 .. 16: every dot product of the GEMM is ONE product, nothing averages out, and the product dominates the
residual Z_0 it is added to.  W_i stays dense and random, so the messages carry full mantissas.  Then

    Z_t[r, i] = Z_0[r, i] + w_i * sum_j c_j M_j[pi(i)],   M = relu(Z_{t-1}),  j over row r's gather entries.

The gather entries of a row are those of the form its path evaluates: the unblocked path gathers the packer's
merged list (``bond_message_gather``), the molecule-blocked fused layers the reference's own form, all in-bonds
of the source atom minus the reverse bond (``fused_message_gather``).

Reference and bound.  The reference of layer t is that formula in float64 from the kernel's own Z_0 and
Z_{t-1} (errors do not travel from layer to layer, and the kink decisions are the kernel's).  The bound is
2^-21 (|Z_0| + |w_i| sum_j |c_j| |M_j|) per element.  For fp16-pair operands csrc/planes.hpp adds an absolute
term: where lo goes subnormal the representation error of a value is no longer relative but at most 2^-25 in
scaled units (half the fp16 subnormal spacing 2^-24), that is 2^-25 / s with s the scale of the value's tile.
A message M_j then carries at most 2^-25 / s_M more error and a weight 2^-25 / s_W, which the product and the
gather turn into  |w_i| sum_j |c_j| 2^-25 / s_M  +  2^-25 / s_W  sum_j |c_j| |M_j|.  s_M is taken from the
maximum over the whole molecule block of row j: no tile of the block has a smaller scale, so the term covers
whichever tiling the producer used.
"""
import numpy as np
import torch

from oracle import split_ref

REL = 2.0 ** -21


def full_mantissa(rng, shape, lo_exp, hi_exp):
    """fp32 values with random sign, exponent in [lo_exp, hi_exp) and all 23 mantissa bits random."""
    n = int(np.prod(shape))
    bits = (rng.integers(0, 2, n, dtype=np.uint64) << 31) | \
        ((rng.integers(lo_exp, hi_exp, n).astype(np.uint64) + 127) << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint64)
    return bits.astype(np.uint32).view(np.float32).reshape(shape)


def signed_permutation(rng, n):
    """(W [n][n] fp32, pi, w): row i of W holds the single nonzero w[i] at column pi[i]; |w| in [4, 16) with
    full mantissas, one in four negative.  Among such values the probe keeps those whose fp16 pair (scale 2^11: the
    maximum lies in [8, 16)) has a lo half below 2^-13 |w s|.  The complete pair scheme drops lo_a lo_b and
    carries both operands' representation errors, each up to 2^-22 of the product: with an arbitrary weight they
    alone can fill the 2^-21 bound (emulated worst element 0.8 to 1.06 of it over eight seeds), leaving nothing
    for the roundings of the gather and of the add to Z_0.  With this choice the weight's share is below 2^-24
    while its lo half stays 2^8 times the bound, so a product that lost it is as visible as before."""
    pi = rng.permutation(n)
    w = np.zeros(0, np.float32)
    while len(w) < n:
        c = np.abs(full_mantissa(rng, (16 * n,), 2, 4))
        hi = (c.astype(np.float64) * 2.0 ** 11).astype(np.float16).astype(np.float64)
        lo = c.astype(np.float64) * 2.0 ** 11 - hi
        w = np.concatenate([w, c[(np.abs(lo) < 2.0 ** -13 * c * 2.0 ** 11) & (lo != 0)]])
    w = w[:n].copy()
    w[0] = max(w[0], np.float32(8.0) + w[0] / 4)  # (the maximum in [8, 16): the scale the choice assumed)
    # one weight in four negative: behind the ReLU a negative weight mostly zeroes its column for the next layer,
    # where those elements then test nothing
    w = (w * rng.choice(np.array([-1.0, 1.0, 1.0, 1.0], np.float32), n)).astype(np.float32)
    W = np.zeros((n, n), np.float32)
    W[np.arange(n), pi] = w
    return W, pi, w


def probe_parameters(hidden, atom_fdim, in_dim, seed, wh_extra=0, layers=True, quantised_wi=False):
    """Encoder parameters (state_dict names -> fp32 tensors, no biases but W_o's zero one) and the probe's
    description.  ``layers=False`` zeroes W_h: the messages reaching W_o are relu(Z_0), W_o alone is probed.
    ``wh_extra``: extra zero input columns of W_h (atom messages: the bond-feature half).  ``quantised_wi``:
    W_i in multiples of 2^-10 from (0, 1): a Z_0 row is then an exact sum plus the one full-mantissa product of
    the mass column, every message still has a full mantissa and is positive, and a reference that starts from
    the features (the paths that expose only their output) is not charged for cancellation in the input layer."""
    rng = np.random.default_rng(seed)
    if quantised_wi:
        wi = (rng.integers(1, 1 << 10, (hidden, in_dim)) / float(1 << 10)).astype(np.float32)
    else:
        wi = (rng.standard_normal((hidden, in_dim)) * 0.25 + 0.1).astype(np.float32)
    Wh, pi_h, w_h = signed_permutation(rng, hidden)
    Wo, pi_o, w_o = signed_permutation(rng, hidden)
    if not layers:
        Wh[:] = 0
    p = {'W_i.weight': wi,
         'W_h.weight': np.concatenate([Wh, np.zeros((hidden, wh_extra), np.float32)], axis=1),
         'W_o.weight': np.concatenate([np.zeros((hidden, atom_fdim), np.float32), Wo], axis=1),
         'W_o.bias': np.zeros(hidden, np.float32), 'cached_zero_vector': np.zeros(hidden, np.float32)}
    return {n: torch.from_numpy(a) for n, a in p.items()}, dict(pi_h=pi_h, w_h=w_h, pi_o=pi_o, w_o=w_o)


def load_parameters(enc, params):
    with torch.no_grad():
        for n, t in enc.named_parameters():
            t.copy_(params[n])


def gather_sums(csr, M):
    """(sum_j c_j M_j, sum_j |c_j| |M_j|) per gather row, float64; M [source rows][H]."""
    n = len(csr.ptr) - 1
    row = np.repeat(np.arange(n), np.diff(csr.ptr))
    idx, coef = csr.idx[:len(row)].astype(np.int64), csr.coef[:len(row)].astype(np.float64)
    M = np.asarray(M, np.float64)
    S, Sabs = np.zeros((n, M.shape[1])), np.zeros((n, M.shape[1]))
    np.add.at(S, row, coef[:, None] * M[idx])
    np.add.at(Sabs, row, np.abs(coef)[:, None] * np.abs(M[idx]))
    return S, Sabs


def fused_message_gather(g):
    """The bond-message gather in the form the molecule-blocked fused layers (and mpn.py:112-120 itself)
    evaluate it: X_b = sum over ALL in-bonds j of b's source atom of w_j M_j, minus M_rev(b) -- the atom
    aggregate's row of b2a[b] followed by the entry (b2revb[b], -1).  ``bond_message_gather`` is the same sum with
    the reverse bond's two contributions merged into one coefficient w_rev - 1 (dropped when 0), which the
    unblocked path gathers; the unmerged form cancels w_rev M_rev against M_rev in fp32, so its rounding error
    scales with sum |w_j| |M_j| + |M_rev|, and that is the sum its bound takes."""
    from chemprop_amd.featurization import Csr
    agg = g.atom_aggregate_gather()
    b2a, rev = g.b2a.numpy(), g.b2revb.numpy()
    rows, idx, coef = [], [], []
    for b in range(1, g.n_bonds):
        e = slice(agg.ptr[b2a[b]], agg.ptr[b2a[b] + 1])
        n = e.stop - e.start
        rows += [b] * (n + 1)
        idx += list(agg.idx[e]) + [int(rev[b])]
        coef += list(agg.coef[e]) + [-1.0]
    return Csr.from_rows(np.array(rows, np.int64), np.array(idx, np.int32), np.array(coef, np.float32), g.n_bonds)


def gather_weight(csr, v):
    """sum_j |c_j| v_j per gather row for a per-source-row quantity v."""
    n = len(csr.ptr) - 1
    row = np.repeat(np.arange(n), np.diff(csr.ptr))
    out = np.zeros(n)
    np.add.at(out, row, np.abs(csr.coef[:len(row)].astype(np.float64)) * v[csr.idx[:len(row)]])
    return out


def block_scales(M, blocks, col=0):
    """Per source row the pair scale of its molecule block: h2_scale of the bits of max |M| over the block's
    rows (``blocks[:, col]`` = first row, ``blocks[:, col + 1]`` = count); rows outside every block: inf."""
    s = np.full(M.shape[0], np.inf)
    for b in blocks:
        r0, n = int(b[col]), int(b[col + 1])
        if n:
            s[r0:r0 + n] = split_ref.h2_scale(split_ref.abs_bits(np.abs(M[r0:r0 + n]).max(initial=0.0)))
    return s


def layer_reference(Z0, M, csr, pi, w, pairs_scales=None):
    """(reference, bound) of Z = Z_0 + (gather of M) W^T for the signed permutation (pi, w), float64.
    ``pairs_scales`` = (per-source-row scale of M, scale of W) adds the fp16-pair floor."""
    S, Sabs = gather_sums(csr, M)
    w = w.astype(np.float64)
    Z0 = np.asarray(Z0, np.float64)
    ref = Z0 + w[None, :] * S[:, pi]
    bound = REL * (np.abs(Z0) + np.abs(w)[None, :] * Sabs[:, pi])
    if pairs_scales is not None:
        s_m, s_w = pairs_scales
        bound = bound + np.abs(w)[None, :] * gather_weight(csr, 2.0 ** -25 / s_m)[:, None] + \
            2.0 ** -25 / s_w * Sabs[:, pi]
    return ref, bound


def worst(Z, ref, bound, rows):
    """(largest |Z - ref| / bound, fraction of elements over the bound) over ``rows`` (elements whose bound is 0
    must be exact)."""
    d = np.abs(np.asarray(Z, np.float64)[rows] - ref[rows])
    b = bound[rows]
    ratio = np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(ratio.max(initial=0.0)), float((ratio > 1.0).mean())


def relu(z):
    return np.maximum(np.asarray(z), 0)


def dev_read(dg, ptr, nbytes):
    """``nbytes`` of device memory at ``ptr``, which must lie inside one of a DeviceGraph's own allocations."""
    for t in [dg.buffer] + [v for v in dg.views.values() if v is not None]:
        base, size = t.data_ptr(), t.numel() * t.element_size()
        if base <= ptr and ptr + nbytes <= base + size:
            flat = t.reshape(-1)
            flat = flat if flat.dtype == torch.uint8 else flat.view(torch.uint8)
            return flat[ptr - base:ptr - base + nbytes].cpu().numpy()
    raise AssertionError('pointer outside the device graph')


# ---------------------------------------------------------------------------------------------------
# CPU emulation of one layer with a (possibly degraded) scheme
# ---------------------------------------------------------------------------------------------------
def emulate_layer(Z0, M, csr, W, scheme, terms, blocks=None):
    """fp32 Z = Z_0 + X W^T with X the gather of M, the GEMM emulated by ``split_ref``:
    'x6': the gathered rows (rounded to fp32) times W on bf16x3 planes;
    'h2': M as fp16 pairs with its block's scale times W's pairs, the products gathered afterwards (the pair
    layers multiply the messages and gather the products)."""
    M = np.asarray(M, np.float32)
    if scheme == 'x6':
        X = gather_sums(csr, M)[0].astype(np.float32)
        acc = split_ref.mm_x6(X, W, terms)
    else:
        s_m = block_scales(M, blocks)
        s_m = np.where(np.isfinite(s_m), s_m, 1.0)[:, None]
        s_w = split_ref.h2_scale(split_ref.abs_bits(np.abs(W).max()))
        P = split_ref.mm_h2(M, W, s_m, s_w, terms)
        acc = gather_sums(csr, P)[0].astype(np.float32)
    return (np.asarray(Z0, np.float32) + acc).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
# layerwise cases (kind, molecules, hidden, depth): the training forward's saved pre-activations and the
# no-grad forward's debug stops.  H 300 / 257: Hk 320, five 64-column chunks, 80-column tiles, pair tiles laid
# out; H 70: Hk 128 with 58 padding columns
LAYER_CASES = {'h300': ('polymer', 6, 300, 3), 'h70': ('polymer', 6, 70, 3), 'h257': ('polymer', 5, 257, 3)}

# paths that expose only their output: depth 2 with W_h = 0 (the blocked paths need depth >= 2; the one layer
# adds nothing to Z_0), W_o a positive permutation (the messages are positive, so a negative weight would only
# zero its whole output column behind the ReLU), W_i quantised (probe_parameters)
OUTPUT_CASES = {
    'blocked-h64': dict(kind='tiny', b=24, hidden=64, path='blocked'),
    'h70': dict(kind='tiny', b=24, hidden=70, path='blocked'),
    'pairs-h257': dict(kind='tiny', b=16, hidden=257, path='blocked', pairs=True),
    'atom-blocked': dict(kind='tiny', b=24, hidden=64, atom=True, path='blocked'),
    'atom-unblocked': dict(kind='tiny', b=24, hidden=64, atom=True, bias=True, path='unblocked'),
    'hub-fallback': dict(kind='hub', b=12, hidden=64, path='unblocked'),
    'qm9-one-launch': dict(kind='tiny-qm9', b=24, hidden=300, path='small'),
}


def case_seed(name):
    return 7000 + sum(ord(c) for c in name)


def make_graph(kind, b, **kw):
    """The batch of a case.  'tiny' / 'tiny-qm9': molecules of 4 to 6 / 2 to 4 atoms, packed into full molecule
    blocks: the readout of the output-only paths is a mean over a molecule's atoms, which averages the rounding
    errors of its terms away while the bound adds up; with few atoms per molecule a lost product still shows.
    'hub': the edge-case batch with a 130-leaf hub (no molecule blocks: the unblocked fallback) plus ``b`` tiny
    polymers."""
    from chemprop_amd import synthetic
    from chemprop_amd.featurization import BatchMolGraph
    rng = np.random.default_rng(4200 + b)
    if kind == 'tiny':
        return BatchMolGraph([synthetic.polymer_graph(rng, 2, 3) for _ in range(b)], block_target=2, **kw)
    if kind == 'tiny-qm9':
        return BatchMolGraph([synthetic.molecule_graph(rng, 2, 4) for _ in range(b)], **kw)
    if kind == 'hub':
        mols = synthetic.edge_case_batch(9, star_leaves=130) + [synthetic.polymer_graph(rng, 2, 3) for _ in range(b)]
        return BatchMolGraph(mols, **kw)
    return BatchMolGraph(synthetic.make_batch(kind, b, 4200 + b), **kw)


def output_args(case):
    from chemprop_amd import TrainArgs
    return TrainArgs(hidden_size=case['hidden'], depth=2, atom_messages=bool(case.get('atom')),
                     bias=bool(case.get('bias')))


def output_graph(case):
    return make_graph(case['kind'], case['b'])


def output_parameters(case):
    from chemprop_amd.featurization import get_atom_fdim, get_bond_fdim
    atom = bool(case.get('atom'))
    Fa, Fb = get_atom_fdim(), get_bond_fdim(atom_messages=atom)
    H = case['hidden']
    name = next(n for n, c in OUTPUT_CASES.items() if c is case)
    params, info = probe_parameters(H, Fa, Fa if atom else Fb, case_seed(name), wh_extra=Fb if atom else 0,
                                    layers=False, quantised_wi=True)
    wo = params['W_o.weight']
    wo[:, Fa:] = wo[:, Fa:].abs()
    info['w_o'] = np.abs(info['w_o'])
    if case.get('bias'):  # (zero biases: the same function on the path a biased model takes)
        params['W_i.bias'] = torch.zeros(H)
        params['W_h.bias'] = torch.zeros(H)
    return params, info


def readout(g, hid, weights=None):
    """mpn.py:146-171 with the default mean aggregation, float64: per molecule xn * sum_a w_a hid_a / sum_a w_a."""
    w_atoms = g.w_atoms.numpy().astype(np.float64)
    out = np.zeros((len(g.a_scope), hid.shape[1]))
    for i, (a0, n) in enumerate(g.a_scope):
        if n:
            w = w_atoms[a0:a0 + n]
            out[i] = float(g.degree_of_polym[i]) * (w[:, None] * hid[a0:a0 + n]).sum(axis=0) / w.sum()
    return out


def output_messages(g, params, case):
    """(M = relu(Z_0) as fp32 from a float64 input layer, the atom aggregate gather, W_o[:, Fa:])."""
    atom = bool(case.get('atom'))
    f = (g.f_atoms if atom else g.f_bonds).numpy().astype(np.float64)
    Z0 = (f @ params['W_i.weight'].numpy().astype(np.float64).T).astype(np.float32)
    Fa = g.f_atoms.shape[1]
    return relu(Z0), g.atom_aggregate_gather(atom), params['W_o.weight'].numpy()[:, Fa:]


def output_reference(g, params, info, case, pair_floor=True):
    """(fp64 reference of the encoder output from the features, elementwise bound).  The bound is the layer
    bound of W_o carried through the readout -- a positively weighted mean of non-negative terms, no
    cancellation -- and widened by n_atoms 2^-24 for the readout's own sums: (2^-21 + n_atoms 2^-24) times the
    readout of |w_i| sum_j |c_j| |M_j|, plus, on a path whose W_o multiplies fp16 pairs, the readout of the pair
    floor (the aggregate A in pairs with its block's scale, W_o[:, Fa:] with its own)."""
    from oracle import mpn_ref
    args = output_args(case)
    p64 = {n: t.double() for n, t in params.items()}
    with torch.no_grad():
        ref = mpn_ref.encoder_forward(p64, g, args, dtype=torch.float64).numpy()
    M, agg, Wo = output_messages(g, params, case)
    S, Sabs = gather_sums(agg, M)
    w = info['w_o'].astype(np.float64)
    base = np.abs(w)[None, :] * Sabs[:, info['pi_o']]
    n_at = np.zeros(g.n_atoms)
    for a0, n in g.a_scope:
        n_at[a0:a0 + n] = n
    per_atom = (REL + n_at[:, None] * 2.0 ** -24) * base
    if case.get('pairs') and pair_floor:
        s_a = block_scales(S, g.molecule_blocks(), col=2)
        s_w = split_ref.h2_scale(split_ref.abs_bits(np.abs(Wo).max()))
        per_atom = per_atom + np.abs(w)[None, :] * (2.0 ** -25 / s_a)[:, None] + 2.0 ** -25 / s_w * Sabs[:, info['pi_o']]
    return ref, readout(g, per_atom)
