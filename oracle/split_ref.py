"""Test infrastructure (CPU checker, never imported by chemprop_amd): a numpy restatement of the two
split-operand formats the GEMMs multiply, written from their contracts (csrc/planes.hpp's header
comments), not from the kernels' code paths.

bf16x3 planes.  x = h + m + l with h = rne_bf16(x), m = rne_bf16(x - h), l = rne_bf16(x - h - m); both
residuals are exact in fp32, each piece carries 8 significant bits, so the planes hold every fp32 value to
its last bit (finite x, l not below the bf16 subnormals).  A plane-tile matrix [rows][kp] (rows % BR == 0,
kp % 32 == 0) is a row-major grid of blocks of BR rows x 32 columns; a block is 3 planes (h, m, l) of
BR x 32 bf16, row-major: BR * 64 bytes per plane, 3 * BR * 64 per block, rows * kp * 6 in all.  BR = 64 is
the natural-row layout, 80 the fused kernels' weight layout, 128 the molecule-blocked bond layout.

fp16 hi / lo pairs.  With the power-of-two scale s = 2^(141 - e), e the biased exponent of max |x| (so
max |x| s lies in [2^14, 2^15)), x s = hi + lo + r with hi = rne_f16(x s), lo = rne_f16(x s - hi) and
|r| <= 2^-22 |x s|, or, where lo goes subnormal, |r| <= 2^-25 (half the fp16 subnormal spacing 2^-24) in
scaled units.  A pair-tile matrix has the plane-tile layout with two planes (hi, lo): 2 * BR * 64 bytes
per block; inside one molecule block (one block row) the offset is (k / 32) (2 BR 64) + 64 r + 2 (k % 32).

Emulated products.  ``mm_x6`` / ``mm_h2`` keep one fp32 accumulator per output element and add whole-plane
products (each the exactly rounded fp32 value of the plane product, summed over K in float64) in a fixed
order; ``terms`` may leave any product out: the degraded schemes a test bound has to tell from the
complete one.
"""
import numpy as np

X6_TERMS = ('hh', 'hm', 'mh', 'hl', 'lh', 'mm')  # the six products of the bf16x3 scheme (ml, lm, ll dropped)
H2_TERMS = ('hh', 'hl', 'lh')                    # the three of the fp16-pair scheme (lo lo dropped)
BLOCK_ROWS = (64, 80, 128)


# ---------------------------------------------------------------------------------------------------
# bf16x3 planes
# ---------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """Round-to-nearest-even bf16 of finite fp32 values, as uint16, by integer arithmetic on the fp32 bits:
    add 0x7fff plus the lowest kept bit, keep the upper half."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_value(bits):
    """The fp32 value of bf16 bit patterns."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_rne(x):
    return bf16_value(bf16_bits(x))


def split3(x):
    """(h, m, l) fp32 arrays of bf16-representable values with h + m + l == x (finite fp32 x).  The residuals
    are formed in float64 and must fit fp32 unchanged (the contract's "exact in fp32")."""
    x = np.ascontiguousarray(x, np.float32)
    h = bf16_rne(x)
    r1 = x.astype(np.float64) - h
    r1f = r1.astype(np.float32)
    m = bf16_rne(r1f)
    r2 = r1 - m
    r2f = r2.astype(np.float32)
    if not (np.array_equal(r1f.astype(np.float64), r1) and np.array_equal(r2f.astype(np.float64), r2)):
        raise ValueError('a split residual is not an fp32 value')
    return h, m, bf16_rne(r2f)


def plane_offset(r, k, kp, br=64):
    """Byte offset of (row r, column k) in plane 0 of a plane-tile matrix with ``br``-row blocks and kp columns;
    plane p lies p * br * 64 bytes further."""
    r, k = np.asarray(r, np.int64), np.asarray(k, np.int64)
    return ((r // br) * (kp // 32) + k // 32) * (3 * br * 64) + (r % br) * 64 + 2 * (k % 32)


def _check_tile(rows, kp, br):
    if br not in BLOCK_ROWS or rows % br or kp % 32:
        raise ValueError(f'plane tiles need rows % BR == 0, kp % 32 == 0, BR in {BLOCK_ROWS} (rows {rows}, kp {kp}, BR {br})')


def encode_planes(x, br=64, row_map=None, out_rows=None):
    """uint8 [out_rows * kp * 6]: the plane tiles of fp32 ``x`` [rows][kp].  ``row_map`` (int, one entry per
    source row): row r goes to tile row row_map[r], skipped when negative; tile rows nothing maps to are zero."""
    x = np.ascontiguousarray(x, np.float32)
    rows, kp = x.shape
    if row_map is None:
        row_map = np.arange(rows, dtype=np.int64)
        out_rows = rows if out_rows is None else out_rows
    row_map = np.asarray(row_map, np.int64)
    _check_tile(out_rows, kp, br)
    if len(row_map) != rows or (row_map >= out_rows).any():
        raise ValueError('row_map must hold one tile row < out_rows (or a negative value) per source row')
    keep = row_map >= 0
    if len(np.unique(row_map[keep])) != int(keep.sum()):
        raise ValueError('row_map sends two rows to one tile row')
    out = np.zeros(out_rows * kp * 3, np.uint16)
    off = plane_offset(row_map[keep][:, None], np.arange(kp)[None, :], kp, br) // 2
    for p, plane in enumerate(split3(x[keep])):
        out[off + p * br * 32] = bf16_bits(plane)
    return out.view(np.uint8)


def decode_planes(buf, rows, kp, br=64):
    """(h, m, l): the three planes of a plane-tile matrix [rows][kp], each an fp32 array, separately."""
    _check_tile(rows, kp, br)
    t = np.ascontiguousarray(buf, np.uint8)[:rows * kp * 6].view(np.uint16)
    off = plane_offset(np.arange(rows)[:, None], np.arange(kp)[None, :], kp, br) // 2
    return tuple(bf16_value(t[off + p * br * 32]) for p in range(3))


# ---------------------------------------------------------------------------------------------------
# fp16 hi / lo pairs
# ---------------------------------------------------------------------------------------------------
def h2_scale(word):
    """The scale of a maximum given as the bits of its absolute value (a scale word): 2^(se - 127) with
    se = 268 - (word >> 23) clamped to [1, 253]: the scale and its inverse stay normal floats.  The upper
    clamp holds every maximum below 2^-112 (zero and subnormal ones among them) at 2^126; the lower one is out of
    reach of any fp32 word (a finite maximum gives se >= 14)."""
    se = np.clip(268 - (np.asarray(word).astype(np.int64) >> 23), 1, 253)
    return np.ldexp(1.0, se - 127)


def abs_bits(x):
    """The scale word of one value: the bits of |x| (fp32)."""
    a = np.asarray(x, np.float32)
    return (a.reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)).reshape(a.shape)


def split_h2(x, s):
    """(hi, lo) float16 arrays: hi = rne_f16(x s), lo = rne_f16(x s - hi); ``s`` a power of two (scalar or
    broadcastable).  x s and the residual are exact in float64, so each piece is rounded once."""
    xs = np.asarray(x, np.float32).astype(np.float64) * s
    with np.errstate(over='raise'):
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float64)).astype(np.float16)
    return hi, lo


def pair_offset(r, k, kp, br):
    """Byte offset of (row r, column k) in the hi plane of a pair-tile matrix with ``br``-row blocks; the lo
    plane lies br * 64 bytes further.  Within one block row: (k / 32) (2 br 64) + 64 r + 2 (k % 32)."""
    r, k = np.asarray(r, np.int64), np.asarray(k, np.int64)
    return ((r // br) * (kp // 32) + k // 32) * (2 * br * 64) + (r % br) * 64 + 2 * (k % 32)


def encode_pairs(x, s, br):
    """uint8 [rows * kp * 4]: the pair tiles of fp32 ``x`` [rows][kp] scaled by ``s``."""
    x = np.ascontiguousarray(x, np.float32)
    rows, kp = x.shape
    if rows % br or kp % 32:
        raise ValueError('pair tiles need rows % BR == 0 and kp % 32 == 0')
    out = np.zeros(rows * kp * 2, np.uint16)
    off = pair_offset(np.arange(rows)[:, None], np.arange(kp)[None, :], kp, br) // 2
    hi, lo = split_h2(x, s)
    out[off] = hi.view(np.uint16)
    out[off + br * 32] = lo.view(np.uint16)
    return out.view(np.uint8)


def decode_pairs(buf, rows, kp, br):
    """(hi, lo) float16 arrays [rows][kp] of a pair-tile matrix (still in scaled units)."""
    if rows % br or kp % 32:
        raise ValueError('pair tiles need rows % BR == 0 and kp % 32 == 0')
    t = np.ascontiguousarray(buf, np.uint8)[:rows * kp * 4].view(np.uint16)
    off = pair_offset(np.arange(rows)[:, None], np.arange(kp)[None, :], kp, br) // 2
    return t[off].view(np.float16), t[off + br * 32].view(np.float16)


# ---------------------------------------------------------------------------------------------------
# emulated products: C = A B^T, A [M][K], B [N][K]
# ---------------------------------------------------------------------------------------------------
def _accumulate(planes_a, planes_b, terms, known):
    acc = None
    for t in terms:
        if t not in known:
            raise ValueError(f'unknown product {t!r} (known: {known})')
        prod = (planes_a[t[0]] @ planes_b[t[1]].T).astype(np.float32)
        acc = prod if acc is None else (acc + prod).astype(np.float32)
    return acc


def mm_x6(A, B, terms=X6_TERMS):
    """fp32 [M][N]: the bf16x3 product of fp32 A and B with the listed plane products, added in that order."""
    pa = dict(zip('hml', (p.astype(np.float64) for p in split3(A))))
    pb = dict(zip('hml', (p.astype(np.float64) for p in split3(B))))
    return _accumulate(pa, pb, terms, X6_TERMS)


def mm_h2(A, B, sa, sb, terms=H2_TERMS):
    """fp32 [M][N]: the fp16-pair product of fp32 A (scale ``sa``, a scalar or broadcastable to A) and B (scale
    ``sb``).  The pieces are divided by their power-of-two scales first (exact), so scales that vary along K --
    one word per column tile of a molecule block -- need no special case."""
    pa = dict(zip('hl', (p.astype(np.float64) / sa for p in split_h2(A, sa))))
    pb = dict(zip('hl', (p.astype(np.float64) / sb for p in split_h2(B, sb))))
    return _accumulate(pa, pb, terms, H2_TERMS)
