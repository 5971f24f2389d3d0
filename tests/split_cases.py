"""Inputs, references and bounds shared by the split-operand term tests (test_split_ref.py and
test_split_bwd_ref.py on the CPU, test_split_terms_gpu.py and test_split_bwd_gpu.py on the GPU): the same batches,
probe weights, stagewise fp64 reference and elementwise bound, so that what the CPU emulation shows about the
bound -- the complete schemes stay under it, a scheme that lost one product does not -- holds for the very numbers
the GPU tests feed the kernels.  The forward comes first; the backward's cases, references and emulation follow
under "the backward".

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
    from chemprop_amd.featurization import BatchMolGraph
    if kind == 'tiny':
        kw = dict(block_target=2, **kw)
    return BatchMolGraph(make_mols(kind, b), **kw)


def make_mols(kind, b):
    """The molecules of ``make_graph``'s batch."""
    from chemprop_amd import synthetic
    rng = np.random.default_rng(4200 + b)
    if kind == 'tiny':
        return [synthetic.polymer_graph(rng, 2, 3) for _ in range(b)]
    if kind == 'tiny-qm9':
        return [synthetic.molecule_graph(rng, 2, 4) for _ in range(b)]
    if kind == 'hub':
        return synthetic.edge_case_batch(9, star_leaves=130) + [synthetic.polymer_graph(rng, 2, 3) for _ in range(b)]
    return synthetic.make_batch(kind, b, 4200 + b)


def full_mantissa_mols(mols, seed, lo_exp=-20, hi_exp=20):
    """``mols`` with atom feature rows and bond feature tails replaced by full-mantissa floats in every column,
    exponents in [lo_exp, hi_exp) (bond rows stay source atom row + tail, as the reference lays them out)."""
    rng = np.random.default_rng(seed)
    for g in mols:
        if not g.n_atoms:
            continue
        fa = full_mantissa(rng, (g.n_atoms, len(g.f_atoms[0])), lo_exp, hi_exp)
        g.f_atoms = [[float(v) for v in row] for row in fa]
        tail_w = len(g.f_bonds[0]) - fa.shape[1] if g.n_bonds else 0
        tails = full_mantissa(rng, (g.n_bonds, tail_w), lo_exp, hi_exp)
        g.f_bonds = [g.f_atoms[int(g.b2a[j])] + [float(v) for v in tails[j]] for j in range(g.n_bonds)]
    return mols


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


# ---------------------------------------------------------------------------------------------------
# the backward: cases, stage references and bounds, CPU emulation (test_split_bwd_ref.py, test_split_bwd_gpu.py)
# ---------------------------------------------------------------------------------------------------
# The output gradient's columns are disjoint across molecules: dout[m, c] != 0 only for the columns c that
# molecule m owns.  With the probe weights (W_h, W_o[:, Fa:] signed permutations, ReLU) a column stays with one
# molecule all the way down, so every element of a weight gradient sums the products of ONE molecule's rows (two
# molecules' in dZ_0 at depth 2, where a column collects the residual and the layer), at any batch size: about a
# dozen products, and the elementwise bound 2^-21 sum |a| |b| shows a lost plane product.  Features are
# full-mantissa floats with exponents in [-1, 2) (host-built graphs), dout likewise.
#
# path: the loop of wdmpnn_backward the case must take ('blocked': the fused order with fp16-pair GEMMs for dM and
# dW_h; 'unblocked': bf16x3 throughout, X_t saved).  only: the stages a large case checks.
BWD_CASES = {
    'tiny-b24-h300': dict(kind='tiny', b=24, hidden=300, depth=2, path='blocked', bias=True),
    'tiny-b24-h70': dict(kind='tiny', b=24, hidden=70, depth=2, path='blocked'),
    'tiny-b96-h300': dict(kind='tiny', b=96, hidden=300, depth=2, path='blocked', only=('dW', 'db', 'words', 'mwords')),
    'tiny-b24-h300-d3': dict(kind='tiny', b=24, hidden=300, depth=3, path='blocked'),
    'hub-h64': dict(kind='hub', b=12, hidden=64, depth=2, path='unblocked'),
    'atom-h64': dict(kind='tiny', b=24, hidden=64, depth=2, path='unblocked', atom=True),
    'undirected-h70': dict(kind='tiny', b=24, hidden=70, depth=2, path='blocked', undirected=True),
}
# Molecules of more than 32 bond rows own no columns: 32 rows are one chunk of the weight-gradient GEMM, so an owner's
# products meet in at most two chunks of one accumulator, and the bound 2^-21 sum |a| |b| keeps room for their fp32
# roundings next to the scheme's own error; the hub's 260-term sums stay out altogether.
OWNER_MAX_BONDS = 32
U24 = 2.0 ** -24


class Bag(dict):
    """A dict with attribute access."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def bwd_inputs(name):
    """Everything a backward case feeds the encoder: the host-built batch with full-mantissa features, the probe
    parameters (zero biases present when the case asks: the same function through the bias kernels), the training
    arguments and the column-owned output gradient."""
    from chemprop_amd import TrainArgs
    from chemprop_amd.featurization import BatchMolGraph, get_atom_fdim, get_bond_fdim
    case = BWD_CASES[name]
    atom, H, seed = bool(case.get('atom')), case['hidden'], case_seed(name)
    mols = full_mantissa_mols(make_mols(case['kind'], case['b']), seed, -1, 2)
    g = BatchMolGraph(mols, compact=False, **(dict(block_target=2) if case['kind'] == 'tiny' else {}))
    Fa, Fb = get_atom_fdim(), get_bond_fdim(atom_messages=atom)
    params, info = probe_parameters(H, Fa, Fa if atom else Fb, seed, wh_extra=Fb if atom else 0)
    if case.get('bias'):
        params['W_i.bias'] = torch.zeros(H)
        params['W_h.bias'] = torch.zeros(H)
    args = TrainArgs(hidden_size=H, depth=case['depth'], atom_messages=atom, bias=bool(case.get('bias')),
                     undirected=bool(case.get('undirected')))
    owners = np.array([i for i, (_, n) in enumerate(g.b_scope) if 0 < n <= OWNER_MAX_BONDS])
    owner = owners[np.arange(H) % len(owners)]
    dout = np.zeros((len(g.a_scope), H), np.float32)
    dout[owner, np.arange(H)] = full_mantissa(np.random.default_rng(seed + 1), (H,), -1, 2)
    R = g.n_atoms if atom else g.n_bonds
    Hk = -(-H // 64) * 64
    Fak, Fbk = -(-Fa // 32) * 32, -(-Fb // 32) * 32
    plan = Bag(blocked=case['path'] == 'blocked', bm=128, R=R, Rp=-(-R // 128) * 128, Va=g.n_atoms,
               Vap=-(-g.n_atoms // 128) * 128, Hk=Hk, ldx=Hk + Fbk if atom else Hk,
               o=tn_plan(Hk, Fak + Hk, g.n_atoms), h=tn_plan(Hk, Hk + Fbk if atom else Hk, R),
               i=tn_plan(Hk, Fak if atom else Fbk, R))
    f_in = (g.f_atoms if atom else g.f_bonds).numpy()
    f_tail = g.f_bonds.numpy()[:, -Fb:] if atom else None
    return Bag(name=name, case=case, g=g, params=params, info=info, args=args, dout=dout, owner=owner, atom=atom,
               undirected=bool(case.get('undirected')), H=H, T=case['depth'], Fa=Fa, Fb=Fb, plan=plan, f_in=f_in,
               f_tail=f_tail, only=case.get('only'))


def tn_plan(n_out, n_dense, m_rows, target=512):
    """(k_per_split, nsplit) of the weight-gradient GEMM's split-K plan (wdmpnn.hip tn_plan), restated so that
    the CPU emulation splits as the kernel does; the GPU tests compare it with the debug export."""
    tiles = -(-n_out // 64) * -(-n_dense // 64)
    chunks = -(-m_rows // 32)
    ns = max(1, min(target // tiles, chunks))
    kps = -(-chunks // ns) * 32
    return kps, max(1, -(-m_rows // kps))


def bwd_gathers(g, atom):
    """(msg, agg, msg_t, agg_t): the gather lists of the forward and their transposes, as device_graph packs them."""
    if atom:
        msg, agg = g.atom_message_gather()[0], g.atom_aggregate_gather(True)
        return msg, agg, msg.transpose(g.n_atoms), agg.transpose(g.n_atoms)
    return g._native_gathers()


def sym_compose(csr, rev):
    """The gather of (M + M[rev]) / 2 as one list: each entry (r, j, c) becomes (r, j, c/2), (r, rev j, c/2)."""
    from chemprop_amd.featurization import Csr
    n = len(csr.ptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(csr.ptr))
    idx, coef = csr.idx[:len(row)].astype(np.int64), csr.coef[:len(row)]
    return Csr.from_rows(np.concatenate([row, row]), np.concatenate([idx, rev[idx]]).astype(np.int32),
                         np.concatenate([coef, coef]).astype(np.float32) * np.float32(0.5), n)


def y_words(Y, plan):
    """act_bwd_kernel's scale words of Y [rows <= Rp][cols <= Hk] (zero padded): the largest absolute-value bits
    of every 256 consecutive float4 of the [Rp][Hk] buffer."""
    buf = np.zeros((plan.Rp, plan.Hk), np.float32)
    buf[:Y.shape[0], :Y.shape[1]] = Y
    return split_ref.abs_bits(buf).reshape(-1, 1024).max(axis=1)


def m_words(Z, plan):
    """The data-gradient GEMM's scale words of M = relu(Z): the largest |M| bits per bm x 64 tile of [Rp][Hk],
    tile (mt, nt) at mt * (Hk / 64) + nt; padding rows and columns hold zeros."""
    buf = np.zeros((plan.Rp, plan.Hk), np.float32)
    buf[:Z.shape[0], :Z.shape[1]] = relu(Z)
    return split_ref.abs_bits(buf).reshape(plan.Rp // plan.bm, plan.bm, plan.Hk // 64, 64).max(axis=(1, 3)).reshape(-1)


def split_pair_scales(words, mwords, plan):
    """[(s_Y, s_M)] per split of the pair weight-gradient GEMM (gemm_tn_x6_kernel<..., true>): one scale per operand
    from the words of the split's rows."""
    kps, nsplit = plan.h
    cv, tn = plan.Hk // 4, plan.Hk // 64
    out = []
    for z in range(nsplit):
        kbeg = z * kps
        ke = max(min(plan.R, kbeg + kps), kbeg + 1)
        wa0, wa1 = (kbeg * cv) >> 8, (ke * cv - 1) >> 8
        rb0, rb1 = kbeg // plan.bm, (ke - 1) // plan.bm
        out.append((float(split_ref.h2_scale(words[wa0:wa1 + 1].max())),
                    float(split_ref.h2_scale(mwords[rb0 * tn:(rb1 + 1) * tn].max()))))
    return out


def row_tile_scales(words, plan):
    """Per row of Y the scale the data-gradient GEMM (gemm_x6_kernel<H2>) gives its bm-row tile."""
    cv = plan.Hk // 4
    s = np.zeros(plan.Rp)
    for m0 in range(0, plan.Rp, plan.bm):
        s[m0:m0 + plan.bm] = split_ref.h2_scale(words[(m0 * cv) >> 8:(((m0 + plan.bm) * cv - 1) >> 8) + 1].max())
    return s


def max_scale(x):
    return float(split_ref.h2_scale(split_ref.abs_bits(np.float32(np.abs(x).max(initial=0.0)))))


# --- references and bounds, each from the buffers the stage read -------------------------------------------------
def readout_adjoint(inp, Zo):
    """dZo = (dout[i] xn_i / sum w) w_a relu'(Zo) (mean aggregation; readout_act_bwd_kernel), float64.  Four
    factors, each of the three operations rounded once, and the fp32 sum of a small molecule's weights carries up
    to three roundings more: (4 + 2) 2^-24 |ref|."""
    g = inp.g
    w = g.w_atoms.numpy().astype(np.float64)
    ref = np.zeros((g.n_atoms, inp.H))
    for i, (a0, n) in enumerate(g.a_scope):
        if n and inp.dout[i].any():
            gi = inp.dout[i].astype(np.float64) * float(np.float32(g.degree_of_polym[i])) / w[a0:a0 + n].sum()
            ref[a0:a0 + n] = gi[None, :] * w[a0:a0 + n, None]
    ref = ref * (np.asarray(Zo) > 0)
    return ref, 6 * U24 * np.abs(ref)


def perm_product(G, pi, w):
    """(ref, sum |a| |b|) of G W for the signed permutation (pi, w): C[:, pi[i]] = G[:, i] w[i], one product each."""
    G = np.asarray(G, np.float64)
    ref, ab = np.zeros_like(G), np.zeros_like(G)
    ref[:, pi] = G * w.astype(np.float64)[None, :]
    ab[:, pi] = np.abs(G) * np.abs(w.astype(np.float64))[None, :]
    return ref, ab


def gather_bwd(csr_t, G, keep=None, slack=None):
    """(ref, bound) of a transposed gather (act_bwd_kernel's CSR branch), masked by ``keep`` (relu'): an n-entry
    fp32 sum of products, (n + 1) 2^-24 sum |c| |x|.  ``slack``: the error bound G itself carries (a rebuilt
    buffer), gathered with |c| on top."""
    S, Sabs = gather_sums(csr_t, G)
    n = np.diff(csr_t.ptr)[:, None]
    bound = (n + 1) * U24 * Sabs
    if slack is not None:
        carried = gather_sums(csr_t, slack)[1]
        bound = bound + carried + (n + 1) * U24 * carried
    if keep is not None:
        S, bound = S * keep, bound * keep
    return S, bound


def symmetrise(S, bound, rev):
    """act_bwd_kernel's sym_rev branch on top of (S, bound): (a + b) / 2 rounds its add once."""
    ref = 0.5 * (S + S[rev])
    b = 0.5 * (bound + bound[rev])
    return ref, b + U24 * (0.5 * (np.abs(S) + np.abs(S[rev])) + b)


def tn_reference(A, B, plan_hw, pair_scales=None, slack_A=None):
    """(ref, bound) of the weight-gradient GEMM A^T B, A [rows][n], B [rows][k], float64: 2^-21 sum_r |a_r| |b_r|
    per element; for the pair GEMM plus the floor sum_r (2^-25 / s_Y |b_r| + 2^-25 / s_M |a_r|) over the rows whose
    product is not zero (a zero has an exact pair), with the scales of row r's split.  ``slack_A``: the error
    bound a rebuilt A carries.  No term for the fp32 accumulation and the slab sum: the emulated complete schemes
    stay under the bound without one (test_split_bwd_ref.py)."""
    kps, nsplit = plan_hw
    A64, B64 = np.asarray(A, np.float64), np.asarray(B, np.float64)
    aA, aB = np.abs(A64), np.abs(B64)
    ref, ab = A64.T @ B64, aA.T @ aB
    bound = REL * ab
    nzA, nzB = (A64 != 0).astype(np.float64), (B64 != 0).astype(np.float64)
    if pair_scales is not None:
        for z, (s_y, s_m) in enumerate(pair_scales):
            r = slice(z * kps, (z + 1) * kps)
            bound = bound + 2.0 ** -25 / s_y * (nzA[r].T @ aB[r]) + 2.0 ** -25 / s_m * (aA[r].T @ nzB[r])
    if slack_A is not None:
        bound = bound + np.asarray(slack_A).T @ aB
    return ref, bound


def bias_reference(G, nsplit, slack=None):
    """(ref, bound) of a bias gradient, the column sums of G: fp32 partial sums per thread, eight row groups and
    nsplit slabs; adding a zero is exact, so at most (nonzero terms + 8 + nsplit) roundings of at most
    2^-24 sum |x| each."""
    G = np.asarray(G, np.float64)
    ab = np.abs(G).sum(axis=0)
    bound = ((G != 0).sum(axis=0) + 8 + nsplit) * U24 * ab
    if slack is not None:
        bound = bound + np.asarray(slack).sum(axis=0)
    return G.sum(axis=0), bound


def bwd_stages(inp, fwd, b):
    """[(stage, what the backward wrote, float64 reference, elementwise bound)] in the order of wdmpnn_backward.
    ``fwd``: the saved forward (Z [T] of [R][H], Zo and A [n_atoms][H], on the unblocked path X [R][H] and for
    atom messages Xf [R][Fb]); ``b``: the backward's buffers in natural rows, padding cut off (dZo, dA, dZ_last =
    dZ_{T-1} where it survives, Y (blocked) or dX (unblocked), dZ0, dZ1 at depth 3, dRes, words, mwords) and the
    gradients W_i, W_h, W_o, b_*.  Every reference starts from the buffer the stage read."""
    g, info, plan, T, H = inp.g, inp.info, inp.plan, inp.T, inp.H
    _, _, msg_t, agg_t = bwd_gathers(g, inp.atom)
    rev = g.b2revb.numpy()
    Wh = inp.params['W_h.weight'].numpy()[:, :H]
    s_w = max_scale(Wh)
    keep = [np.asarray(z) > 0 for z in fwd.Z]
    M = [relu(z) for z in fwd.Z]
    out = []

    def y_of(G, slack=None):
        S, bound = gather_bwd(msg_t, G, slack=slack)
        return symmetrise(S, bound, rev) if inp.undirected else (S, bound)

    def dm_of(Y, keep_prev, res, slack_y=None):
        """dZ_{t-1} = relu'(Z_{t-1}) (Y W_h) + res on fp16 pairs: 2^-21 (|res| + |w| |Y|) plus the pair floor
        |w| 2^-25 / s_Y + 2^-25 / s_W |Y| where Y is not zero, s_Y from the largest |Y| of the whole buffer."""
        ref, ab = perm_product(Y, info['pi_h'], info['w_h'])
        s_y = max_scale(np.abs(Y).max(initial=0.0) + (0.0 if slack_y is None else np.max(slack_y)))
        nz = np.asarray(Y) != 0
        fl = perm_product(nz * (2.0 ** -25 / s_y), info['pi_h'], info['w_h'])[1] + \
            2.0 ** -25 / s_w * perm_product(np.abs(Y), info['pi_h'], np.ones(H))[1]
        bound = REL * ab + fl
        if slack_y is not None:
            bound = bound + perm_product(slack_y, info['pi_h'], info['w_h'])[1]
        res = np.zeros_like(ref) if res is None else np.asarray(res, np.float64)
        # (where the product is zero, masked or not there, the add returns the residual itself: exact)
        return ref * keep_prev + res, (bound + REL * np.abs(res) * (ab > 0)) * keep_prev

    ref, bound = readout_adjoint(inp, fwd.Zo)
    out.append(('dZo', b.dZo, ref, bound))
    ref, ab = perm_product(b.dZo, info['pi_o'], info['w_o'])
    out.append(('dA', b.dA, ref, REL * ab))
    last_ref, last_bound = gather_bwd(agg_t, b.dA, keep[T - 1])
    wh_ref = wh_bound = bh_ref = bh_bound = None
    if T == 2:
        out.append(('dZ1', b.dZ_last, last_ref, last_bound))
        out.append(('dRes', b.dRes, np.asarray(b.dZ_last, np.float64), np.zeros_like(last_bound)))
        dZ1 = b.dZ_last
        bh_ref, bh_bound = bias_reference(dZ1, plan.h[1])
    else:  # depth 3, blocked: dZ_2 and Y_2 are gone; rebuilt in float64 from dA, their fp32 slack charged
        y2, y2_slack = y_of(last_ref, last_bound)
        ref, bound = dm_of(y2, keep[1], None, y2_slack)
        out.append(('dZ1', b.dZ1, ref, bound))
        dZ1 = b.dZ1
        res = last_ref + np.asarray(dZ1, np.float64)
        out.append(('dRes', b.dRes, res, last_bound + U24 * np.abs(res)))
        sc2 = [(max_scale(np.abs(y2).max() + y2_slack.max()), s_m)
               for _, s_m in split_pair_scales(np.zeros(plan.Rp * plan.Hk // 1024, np.uint32), m_words(fwd.Z[1], plan), plan)]
        wh_ref, wh_bound = tn_reference(y2, M[1], plan.h, sc2, slack_A=y2_slack)
        wh_bound = wh_bound + U24 * np.abs(wh_ref) * plan.h[1]  # (the second layer's add into each slab)
        r2, b2 = bias_reference(last_ref, plan.h[1], last_bound)
        r1, b1 = bias_reference(dZ1, plan.h[1])
        bh_ref, bh_bound = r2 + r1, b2 + b1 + U24 * (np.abs(r2) + np.abs(r1)) * plan.h[1]
    if plan.blocked:
        ref, bound = y_of(dZ1)
        out.append(('Y1', b.Y, ref, bound))
        words, mwords = y_words(b.Y, plan), m_words(fwd.Z[0], plan)
        out.append(('words', b.words, words, np.zeros(len(words))))
        out.append(('mwords', b.mwords, mwords, np.zeros(len(mwords))))
        ref, bound = dm_of(b.Y, keep[0], b.dRes)
        out.append(('dZ0', b.dZ0, ref, bound))
        # (the floor's scales are the words the kernel wrote, which the stage above holds to the bytes)
        ref, bound = tn_reference(b.Y, M[0], plan.h, split_pair_scales(b.words, b.mwords, plan))
        if wh_ref is not None:
            ref, bound = ref + wh_ref, bound + wh_bound
        out.append(('dW_h', b.W_h, ref, bound))
    else:
        ref, bound = tn_reference(dZ1, fwd.X, plan.h)
        out.append(('dW_h', b.W_h[:, :H], ref, bound))
        if inp.atom:
            ref, bound = tn_reference(dZ1, fwd.Xf, plan.h)
            out.append(('dW_h[:, H:]', b.W_h[:, H:], ref, bound))
        ref, ab = perm_product(dZ1, info['pi_h'], info['w_h'])
        out.append(('dX', b.dX, ref, REL * ab))
        S, bound = gather_bwd(msg_t, b.dX)
        if inp.undirected:
            S, bound = symmetrise(S, bound, rev)
        res = np.asarray(b.dRes, np.float64)
        ref = S * keep[0] + res
        out.append(('dZ0', b.dZ0, ref, (bound + U24 * (np.abs(S) + np.abs(res)) * (bound > 0)) * keep[0]))
    if b.get('b_h') is not None:
        out.append(('db_h', b.b_h, bh_ref, bh_bound))
    Fa = inp.Fa
    ref, bound = tn_reference(b.dZo, g.f_atoms.numpy(), plan.o)
    out.append(('dW_o[:, :Fa]', b.W_o[:, :Fa], ref, bound))
    ref, bound = tn_reference(b.dZo, fwd.A, plan.o)
    out.append(('dW_o[:, Fa:]', b.W_o[:, Fa:], ref, bound))
    ref, bound = bias_reference(b.dZo, plan.o[1])
    out.append(('db_o', b.b_o, ref, bound))
    ref, bound = tn_reference(b.dZ0, inp.f_in, plan.i)
    out.append(('dW_i', b.W_i, ref, bound))
    if b.get('b_i') is not None:
        ref, bound = bias_reference(b.dZ0, plan.i[1])
        out.append(('db_i', b.b_i, ref, bound))
    if inp.only:
        out = [s for s in out if s[0].startswith(inp.only)]
    return out


def stage_worst(got, ref, bound):
    """(largest |got - ref| / bound, elements over their bound, the share of those among the elements whose bound
    is not zero) of a stage; an element whose bound is 0 must be exact."""
    got, ref, bound = (np.asarray(x, np.float64).reshape(-1) for x in (got, ref, bound))
    d = np.abs(got - ref)
    live = bound > 0
    ratio = np.where(live, d / np.where(live, bound, 1.0), np.where(d > 0, np.inf, 0.0))
    over = ratio > 1.0
    return float(ratio.max(initial=0.0)), int(over.sum()), float(over[live].mean()) if live.any() else 0.0


# --- CPU emulation -----------------------------------------------------------------------------------------------
def emulate_forward(inp):
    """The saved forward of a case, emulated with the complete bf16x3 scheme (fp32 Z_t, A, Zo, X_1)."""
    g, H, T = inp.g, inp.H, inp.T
    msg, agg, _, _ = bwd_gathers(g, inp.atom)
    p = {n: t.numpy() for n, t in inp.params.items()}
    Wh, Wo = p['W_h.weight'][:, :H], p['W_o.weight'][:, inp.Fa:]
    Z0 = (inp.f_in.astype(np.float64) @ p['W_i.weight'].astype(np.float64).T).astype(np.float32)
    csr = fused_message_gather(g) if inp.plan.blocked else msg
    if inp.undirected:
        csr = sym_compose(csr, g.b2revb.numpy())
    Z = [Z0]
    for _ in range(1, T):
        Z.append(emulate_layer(Z0, relu(Z[-1]), csr, Wh, 'x6', split_ref.X6_TERMS))
    A = gather_sums(agg, relu(Z[-1]))[0].astype(np.float32)
    fwd = Bag(Z=Z, A=A, Zo=split_ref.mm_x6(A, Wo))
    if not inp.plan.blocked:
        fwd.X = gather_sums(csr, relu(Z[0]))[0].astype(np.float32)
        if inp.atom:
            fwd.Xf = gather_sums(g.atom_message_gather()[1], inp.f_tail)[0].astype(np.float32)
    return fwd


def emulate_tn(A, B, plan_hw, scheme, terms, pair_scales=None, slabs=None):
    """The split-K slabs of A^T B as the weight-gradient GEMM forms them: per split one fp32 accumulator per
    element, the 32-row chunks added in order, each chunk's plane products from ``split_ref`` with the transposed
    operands (and, for pairs, the split's scales) under that module's contract: a plane product is the exactly
    rounded fp32 value of its sum over the chunk's rows.  ``slabs``: accumulated onto (the next layer of dW_h)."""
    kps, nsplit = plan_hw
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    out = []
    for z in range(nsplit):
        acc = np.zeros((A.shape[1], B.shape[1]), np.float32)
        for k0 in range(z * kps, min(A.shape[0], (z + 1) * kps), 32):
            k1 = min(A.shape[0], (z + 1) * kps, k0 + 32)
            a, bb = A[k0:k1].T, B[k0:k1].T
            if not a.any() or not bb.any():
                continue
            c = split_ref.mm_x6(a, bb, terms) if scheme == 'x6' else split_ref.mm_h2(a, bb, *pair_scales[z], terms)
            acc = (acc + c).astype(np.float32)
        out.append(acc if slabs is None else (slabs[z] + acc).astype(np.float32))
    return out


def slab_sum(slabs):
    acc = slabs[0]
    for s in slabs[1:]:
        acc = (acc + s).astype(np.float32)
    return acc


def f32_colsum(G):
    acc = np.zeros(G.shape[1], np.float32)
    for row in np.asarray(G, np.float32)[np.asarray(G).any(axis=1)]:
        acc = (acc + row).astype(np.float32)
    return acc


def bwd_gemms(inp):
    """{GEMM: (scheme, the stages it writes)} of a case's backward."""
    blocked = inp.plan.blocked
    d = {'dA': ('x6', ('dA',)), 'dW_o': ('x6', ('dW_o[:, :Fa]', 'dW_o[:, Fa:]')), 'dW_i': ('x6', ('dW_i',))}
    if blocked:
        d['dM'] = ('h2', ('dZ0',) + (('dZ1',) if inp.T == 3 else ()))
        d['dW_h'] = ('h2', ('dW_h',))
    else:
        d['dX'] = ('x6', ('dX',))
        d['dW_h'] = ('x6', ('dW_h',) + (('dW_h[:, H:]',) if inp.atom else ()))
    return d


def emulate_backward(inp, fwd, drop=None, base=None):
    """The backward's buffers (``bwd_stages``'s ``b``) in numpy: the elementwise stages in float64 rounded to
    fp32, the GEMMs emulated by ``split_ref``.  ``drop`` = (GEMM, product): that GEMM without that product; with
    ``base`` (a complete emulation) only that GEMM is computed again, from the buffers ``base`` holds."""
    g, info, plan, T, H = inp.g, inp.info, inp.plan, inp.T, inp.H
    _, _, msg_t, agg_t = bwd_gathers(g, inp.atom)
    rev = g.b2revb.numpy()
    p = {n: t.numpy() for n, t in inp.params.items()}
    Wh, Wo = p['W_h.weight'][:, :H], p['W_o.weight'][:, inp.Fa:]
    s_w = max_scale(Wh)
    keep = [np.asarray(z) > 0 for z in fwd.Z]
    M = [relu(z) for z in fwd.Z]
    gemms = bwd_gemms(inp)
    b = Bag() if base is None else Bag(base)

    def terms(name):
        full = split_ref.X6_TERMS if gemms[name][0] == 'x6' else split_ref.H2_TERMS
        return tuple(t for t in full if drop is None or drop != (name, t))

    def todo(name):
        return base is None or (drop is not None and drop[0] == name)

    def f32(x):
        return np.asarray(x, np.float64).astype(np.float32)

    def y_of(G):
        S = gather_sums(msg_t, G)[0]
        return f32(0.5 * (f32(S).astype(np.float64) + f32(S)[rev])) if inp.undirected else f32(S)

    def dm(Y, keep_prev, res):
        words = y_words(Y, plan)
        s_y = row_tile_scales(words, plan)[:Y.shape[0], None]
        C = split_ref.mm_h2(Y, Wh.T, s_y, s_w, terms('dM'))
        C = C * keep_prev
        return C if res is None else (C + res).astype(np.float32)

    if base is None:
        b.dZo = f32(readout_adjoint(inp, fwd.Zo)[0])
    if todo('dA'):
        b.dA = split_ref.mm_x6(b.dZo, Wo.T, terms('dA'))
    if base is None:
        dZl = f32(gather_bwd(agg_t, b.dA, keep[T - 1])[0])
        b.b_h = b.b_i = None
        if T == 2:
            b.dZ_last = b.dRes = dZl
        else:
            b.dZ_last, b._dZ2 = None, dZl
            b._Y2 = y_of(dZl)
    slabs_h = None
    if T == 3:
        if todo('dM'):
            b.dZ1 = dm(b._Y2, keep[1], None)
        if base is None:
            b.dRes = (b._dZ2 + b.dZ1).astype(np.float32)
        if todo('dW_h'):
            sc2 = split_pair_scales(y_words(b._Y2, plan), m_words(fwd.Z[1], plan), plan)
            slabs_h = emulate_tn(b._Y2, M[1], plan.h, 'h2', terms('dW_h'), sc2)
    dZ1 = b.dZ_last if T == 2 else b.dZ1
    if plan.blocked:
        if base is None:
            b.Y = y_of(dZ1)
            b.words, b.mwords = y_words(b.Y, plan), m_words(fwd.Z[0], plan)
        if todo('dM'):
            b.dZ0 = dm(b.Y, keep[0], b.dRes)
        if todo('dW_h'):
            b.W_h = slab_sum(emulate_tn(b.Y, M[0], plan.h, 'h2', terms('dW_h'),
                                        split_pair_scales(b.words, b.mwords, plan), slabs_h))
    else:
        if todo('dW_h'):
            X = np.concatenate([fwd.X, fwd.Xf], axis=1) if inp.atom else fwd.X
            b.W_h = slab_sum(emulate_tn(dZ1, X, plan.h, 'x6', terms('dW_h')))
        if todo('dX'):
            b.dX = split_ref.mm_x6(dZ1, Wh.T, terms('dX'))
        if base is None:
            S = gather_sums(msg_t, b.dX)[0]
            if inp.undirected:
                S = 0.5 * (S + S[rev])
            b.dZ0 = (f32(S * keep[0]) + b.dRes).astype(np.float32)
    if todo('dW_o'):
        b.W_o = slab_sum(emulate_tn(b.dZo, np.concatenate([g.f_atoms.numpy(), fwd.A], axis=1), plan.o, 'x6',
                                    terms('dW_o')))
    if todo('dW_i'):
        b.W_i = slab_sum(emulate_tn(b.dZ0, inp.f_in, plan.i, 'x6', terms('dW_i')))
    if base is None:
        b.b_o = f32_colsum(b.dZo)
        if inp.case.get('bias'):
            b.b_i = f32_colsum(b.dZ0)
            b.b_h = f32_colsum(dZ1) if T == 2 else (f32_colsum(b._dZ2) + f32_colsum(b.dZ1)).astype(np.float32)
    return b
