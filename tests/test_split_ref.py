"""CPU tests of oracle/split_ref.py, the numpy restatement of the split-operand formats (bf16x3 planes, fp16
hi / lo pairs), and of the bound the GPU term tests assert: on those tests' own inputs (split_cases.py) the
emulated complete schemes leave no element over it, and every scheme that lost one product puts at least a
quarter of the elements over it."""
import numpy as np
import pytest
import torch

import split_cases as sc
from chemprop_amd.featurization import get_atom_fdim, get_bond_fdim
from oracle import split_ref as sr


def _wide_values(n, seed):
    """fp32 values with random sign, exponent and mantissa, |x| in [2^-96, 2^100), then +0 and -0."""
    v = sc.full_mantissa(np.random.default_rng(seed), (n,), -96, 100)
    return np.concatenate([v, np.array([0.0, -0.0], np.float32)])


# ---------------------------------------------------------------------------------------------------
# bf16x3 planes
# ---------------------------------------------------------------------------------------------------
def test_bf16_rounding_is_nearest_even_and_agrees_with_torch():
    x = _wide_values(200000, 1)
    ties = np.array([0x3f808000, 0x3f818000, 0xbf808000, 0x3f808001, 0x3f807fff], np.uint32).view(np.float32)
    want = np.array([0x3f80, 0x3f82, 0xbf80, 0x3f81, 0x3f80], np.uint16)  # ties to the even neighbour
    assert np.array_equal(sr.bf16_bits(ties), want)
    t = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(sr.bf16_bits(x), t)


def test_three_planes_hold_every_value_exactly():
    x = _wide_values(200000, 2)
    h, m, l = sr.split3(x)
    for p in (h, m, l):
        assert not (p.view(np.uint32) & 0xffff).any()  # bf16 values
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    assert np.array_equal(np.signbit(h[-2:]), [False, True])  # +0 and -0 keep their sign in h
    assert (m.astype(np.float64) != 0).mean() > 0.9 and (l.astype(np.float64) != 0).mean() > 0.9


@pytest.mark.parametrize('br', sr.BLOCK_ROWS)
def test_plane_tiles_are_a_bijection_and_decode_inverts_encode(br):
    rows, kp = 2 * br, 96
    off = sr.plane_offset(np.arange(rows)[:, None], np.arange(kp)[None, :], kp, br)
    every = np.concatenate([(off + p * br * 64).reshape(-1) for p in range(3)])
    assert np.array_equal(np.sort(every), np.arange(0, rows * kp * 6, 2))
    # a block is contiguous: 3 * br * 64 bytes, plane after plane, rows of 64 bytes
    assert off[0, 0] == 0 and off[1, 0] == 64 and off[0, 1] == 2 and off[0, 32] == 3 * br * 64
    assert off[br, 0] == (kp // 32) * 3 * br * 64
    x = sc.full_mantissa(np.random.default_rng(br), (rows, kp), -40, 40)
    buf = sr.encode_planes(x, br)
    assert buf.dtype == np.uint8 and buf.size == rows * kp * 6
    h, m, l = sr.decode_planes(buf, rows, kp, br)
    H, M, L = sr.split3(x)
    assert np.array_equal(h.view(np.uint32), H.view(np.uint32)) and np.array_equal(m, M) and np.array_equal(l, L)


def test_plane_tiles_with_a_row_map():
    rng = np.random.default_rng(5)
    rows, out_rows, kp = 70, 128, 32
    row_map = np.full(rows, -1, np.int64)
    keep = rng.permutation(rows)[:50]
    row_map[keep] = rng.permutation(out_rows)[:50]
    x = sc.full_mantissa(rng, (rows, kp), -20, 20)
    h, m, l = sr.decode_planes(sr.encode_planes(x, 64, row_map, out_rows), out_rows, kp, 64)
    got = h.astype(np.float64) + m + l
    want = np.zeros((out_rows, kp))
    want[row_map[keep]] = x[keep]
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        sr.encode_planes(x, 64, np.full(rows, out_rows), out_rows)


# ---------------------------------------------------------------------------------------------------
# fp16 pairs
# ---------------------------------------------------------------------------------------------------
def test_scale_rule_and_its_clamps():
    x = np.abs(_wide_values(20000, 3)[:-2])
    s = sr.h2_scale(sr.abs_bits(x))
    assert ((x * s >= 2.0 ** 14) & (x * s < 2.0 ** 15)).all()
    assert np.array_equal(np.log2(s), 141.0 - (sr.abs_bits(x) >> 23))  # s = 2^(268 - e - 127)
    # maxima below 2^-112 (all-zero and subnormal ones among them) take the largest scale, 2^126, whose inverse
    # is still a normal float; the largest finite maximum takes 2^-113
    assert sr.h2_scale(0) == 2.0 ** 126 and sr.h2_scale(0x007fffff) == 2.0 ** 126
    assert sr.h2_scale(sr.abs_bits(np.float32(2.0 ** -113))) == 2.0 ** 126
    assert sr.h2_scale(sr.abs_bits(np.float32(2.0 ** -112))) == 2.0 ** 126
    assert sr.h2_scale(sr.abs_bits(np.float32(2.0 ** -111))) == 2.0 ** 125
    assert sr.h2_scale(0x7f7fffff) == 2.0 ** -113


def test_pairs_meet_the_stated_bound():
    """|x s - hi - lo| <= max(2^-22 |x s|, 2^-25) for values up to 2^40 below their tile's maximum."""
    rng = np.random.default_rng(4)
    x = sc.full_mantissa(rng, (200000,), -30, 11)
    x[0] = 1234.567  # the maximum (exponent 10)
    s = sr.h2_scale(sr.abs_bits(np.abs(x).max()))
    hi, lo = sr.split_h2(x, s)
    xs = x.astype(np.float64) * s
    r = np.abs(xs - hi.astype(np.float64) - lo.astype(np.float64))
    assert (r <= np.maximum(2.0 ** -22 * np.abs(xs), 2.0 ** -25)).all()
    assert (r > 2.0 ** -22 * np.abs(xs)).any()  # the absolute floor is needed: small values sit on it
    assert np.isfinite(hi.astype(np.float64)).all() and np.abs(hi.astype(np.float64)).max() <= 2.0 ** 15


@pytest.mark.parametrize('br', [64, 80, 128])
def test_pair_tiles_are_a_bijection_and_decode_inverts_encode(br):
    rows, kp = 2 * br, 64
    off = sr.pair_offset(np.arange(rows)[:, None], np.arange(kp)[None, :], kp, br)
    every = np.concatenate([off.reshape(-1), (off + br * 64).reshape(-1)])
    assert np.array_equal(np.sort(every), np.arange(0, rows * kp * 4, 2))
    r, k = np.arange(br)[:, None], np.arange(kp)[None, :]  # inside one molecule block
    assert np.array_equal(off[:br], (k // 32) * (2 * br * 64) + r * 64 + 2 * (k % 32))
    x = sc.full_mantissa(np.random.default_rng(br), (rows, kp), -6, 6)
    s = sr.h2_scale(sr.abs_bits(np.abs(x).max()))
    hi, lo = sr.decode_pairs(sr.encode_pairs(x, s, br), rows, kp, br)
    HI, LO = sr.split_h2(x, s)
    assert np.array_equal(hi.view(np.uint16), HI.view(np.uint16)) and np.array_equal(lo.view(np.uint16), LO.view(np.uint16))


# ---------------------------------------------------------------------------------------------------
# the emulated products and the bound of the GPU term tests
# ---------------------------------------------------------------------------------------------------
def test_single_products_of_24_bit_operands():
    """One product per output element: the complete schemes stay under 2^-21 relative, a scheme without one of
    its products does not (the figures the bound's factor rests on)."""
    rng = np.random.default_rng(6)
    n = 200000
    a = sc.full_mantissa(rng, (n, 1), 0, 4)
    b = sc.full_mantissa(rng, (n, 1), 0, 4)
    exact = a.astype(np.float64) * b.astype(np.float64)

    def rel(acc):
        return np.abs(acc - exact)[:, 0] / np.abs(exact)[:, 0]

    def x6(terms):
        pa, pb = sr.split3(a), sr.split3(b)
        acc = np.zeros((n, 1), np.float32)
        for t in terms:
            acc = (acc + (pa['hml'.index(t[0])].astype(np.float64) * pb['hml'.index(t[1])]).astype(np.float32)).astype(np.float32)
        return acc

    def h2(terms):
        pa, pb = sr.split_h2(a, 2.0 ** 11), sr.split_h2(b, 2.0 ** 11)
        acc = np.zeros((n, 1), np.float32)
        for t in terms:
            acc = (acc + (pa['hl'.index(t[0])].astype(np.float64) * pb['hl'.index(t[1])]).astype(np.float32)).astype(np.float32)
        return acc / 2.0 ** 22

    full = rel(x6(sr.X6_TERMS))
    print(f'\nx6 complete: worst {full.max():.2e}')
    assert full.max() <= sc.REL
    for drop in ('hm', 'mh', 'hl', 'lh', 'mm'):
        e = rel(x6([t for t in sr.X6_TERMS if t != drop]))
        print(f'x6 without {drop}: worst {e.max():.2e}, over 2^-21: {(e > sc.REL).mean():.2f}')
        assert (e > sc.REL).mean() >= 0.5
    full = rel(h2(sr.H2_TERMS))
    print(f'h2 complete: worst {full.max():.2e}')
    assert full.max() <= sc.REL
    for drop in ('hl', 'lh'):
        e = rel(h2([t for t in sr.H2_TERMS if t != drop]))
        print(f'h2 without {drop}: worst {e.max():.2e}, over 2^-21: {(e > sc.REL).mean():.2f}')
        assert (e > sc.REL).mean() >= 0.5
    # mm_x6 / mm_h2 are that arithmetic as matrix products
    A, B = a[:64].reshape(8, 8), b[:64].reshape(8, 8)
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    assert np.abs(sr.mm_x6(A, B) - ref).max() <= 4 * sc.REL * (np.abs(A).astype(np.float64) @ np.abs(B).T).max()
    assert np.abs(sr.mm_h2(A, B, 2.0 ** 11, 2.0 ** 11) - ref).max() <= 4 * sc.REL * (np.abs(A).astype(np.float64) @ np.abs(B).T).max()
    with pytest.raises(ValueError):
        sr.mm_x6(A, B, ('ll',))


X6_DROPS = ('hm', 'mh', 'hl', 'lh', 'mm')
H2_DROPS = ('hl', 'lh')


def _assert_discriminates(tag, Z0, M, csr, W, pi, w, rows, blocks, schemes):
    for scheme in schemes:
        all_terms = sr.X6_TERMS if scheme == 'x6' else sr.H2_TERMS
        scales = None
        if scheme == 'h2':
            scales = (sc.block_scales(np.asarray(M, np.float32), blocks),
                      sr.h2_scale(sr.abs_bits(np.abs(W).max())))
        ref, bound = sc.layer_reference(Z0, M, csr, pi, w, scales)
        top, over = sc.worst(sc.emulate_layer(Z0, M, csr, W, scheme, all_terms, blocks), ref, bound, rows)
        print(f'{tag} {scheme} complete: worst ratio {top:.3f}')
        assert over == 0.0 and top <= 1.0, (tag, scheme, top)
        for drop in (X6_DROPS if scheme == 'x6' else H2_DROPS):
            terms = [t for t in all_terms if t != drop]
            top, over = sc.worst(sc.emulate_layer(Z0, M, csr, W, scheme, terms, blocks), ref, bound, rows)
            print(f'{tag} {scheme} without {drop}: worst ratio {top:.1f}, over the bound {over:.2f}')
            assert over >= 0.25, (tag, scheme, drop, over)


@pytest.mark.parametrize('name', list(sc.LAYER_CASES))
def test_bound_discriminates_on_the_layer_cases(name):
    """The message layers and W_o of the layerwise GPU cases, emulated: Z_0 from the fp32 input layer, each
    layer from the complete scheme's previous one."""
    kind, b, hidden, depth = sc.LAYER_CASES[name]
    g = sc.make_graph(kind, b)
    params, info = sc.probe_parameters(hidden, get_atom_fdim(), get_bond_fdim(), sc.case_seed(name))
    fb = g.f_bonds.numpy().astype(np.float64)
    Z0 = (fb @ params['W_i.weight'].numpy().astype(np.float64).T).astype(np.float32)
    blocks = g.molecule_blocks()
    msg, agg = sc.fused_message_gather(g), g.atom_aggregate_gather()  # (the form the split layers gather in)
    Wh, Wo = params['W_h.weight'].numpy(), params['W_o.weight'].numpy()[:, get_atom_fdim():]
    rows = slice(1, g.n_bonds)
    schemes = ('x6', 'h2') if (-(-hidden // 64) * 64) % 80 == 0 else ('x6',)
    Z = Z0
    for t in range(1, depth):
        M = sc.relu(Z)
        _assert_discriminates(f'{name} layer {t}', Z0, M, msg, Wh, info['pi_h'], info['w_h'], rows, blocks, schemes)
        Z = sc.emulate_layer(Z0, M, msg, Wh, 'x6', sr.X6_TERMS)
    M = sc.relu(Z)
    zero = np.zeros((g.n_atoms, hidden), np.float32)
    _assert_discriminates(f'{name} W_o', zero, M, agg, Wo, info['pi_o'], info['w_o'], slice(1, g.n_atoms), blocks,
                          schemes)


@pytest.mark.parametrize('name', list(sc.OUTPUT_CASES))
def test_bound_discriminates_on_the_output_cases(name):
    """The paths that expose only their output: W_o alone (W_h = 0, depth 2), the reference from the features."""
    case = sc.OUTPUT_CASES[name]
    g = sc.output_graph(case)
    params, info = sc.output_parameters(case)
    ref, bound = sc.output_reference(g, params, info, case)
    M, agg, Wo = sc.output_messages(g, params, case)
    zero = np.zeros((g.n_atoms, case['hidden']), np.float32)
    real = ref != 0  # (a molecule without atoms gives the zero vector)
    schemes = ('x6', 'h2') if case.get('pairs') else ('x6',)
    for scheme in schemes:
        all_terms = sr.X6_TERMS if scheme == 'x6' else sr.H2_TERMS
        blocks = g.molecule_blocks()
        for drop in (None,) + (X6_DROPS if scheme == 'x6' else H2_DROPS):
            terms = [t for t in all_terms if t != drop]
            Zo = sc.emulate_layer(zero, M, agg, Wo, scheme, terms, blocks)
            out = sc.readout(g, sc.relu(Zo).astype(np.float64)).astype(np.float32)
            d = np.abs(out.astype(np.float64) - ref)
            over = float((d[real] > bound[real]).mean())
            print(f'{name} {scheme} without {drop}: worst ratio {(d[real] / bound[real]).max():.2f}, over {over:.2f}')
            assert (over == 0.0) if drop is None else (over >= 0.25), (name, scheme, drop, over)
