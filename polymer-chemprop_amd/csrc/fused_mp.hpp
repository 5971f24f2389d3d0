// fused_mp.hpp — molecule-blocked fused message passing (inference forward, bond messages).
//
// Molecules are independent (block-diagonal batches, featurization.py:782-800), so a workgroup that
// owns whole molecules needs no other workgroup's rows.  The host packer groups consecutive molecules
// into blocks of <= 128 bond rows and <= 64 atom rows (WdGraph.blocks).  Intermediates live in
// molecule-blocked plane tiles (planes.hpp, BR = 128 for bond rows, BR = 64 for atom rows), and
// every stage after W_i is ONE launch per (block, 64- or 80-column tile):
//
//   mp_layer_kernel   P = M_{t-1} W_hᵀ (bf16x6 split-plane GEMM on the block's 128 rows; the first layer
//                       stages M_0 = act(inp) from the fp32 inp rows itself), then the CSR gather of P
//                       inside the block (GEMM first, gather second: X_t W_hᵀ = (G M_{t-1}) W_hᵀ =
//                       G (M_{t-1} W_hᵀ), column-separable, mpn.py:110-124), bias, residual inp and
//                       activation: M_t = act(inp + G P (+ b_h)) -> plane tiles of the next layer.  The last layer also forms the atom aggregate
//                       A = Σ_{b into a} w_b M_t[b] (mpn.py:126-131) for its columns -> atom plane tiles.
//   wo_readout_kernel   h = act([f_atoms | A] W_oᵀ + b_o) (mpn.py:132-134) on the block's atoms, then the
//                       molecule readout (mpn.py:145-171) of those columns straight to out[mol].
//
// So the forward is W_i + (T - 1) layer launches + 1, with no gather kernels, no M_0 round trip through
// HBM and no separate readout.  Arithmetic per output element: the P and h GEMMs
// are fp32-accurate (gemm_x6.hpp), the gathers add in CSR order (the reference's slot order).
#pragma once
#include "gemm_x6.hpp"
#include "kernels.hpp"
#include "wdmpnn.h"

namespace wd {


constexpr int BLK_BONDS = 128, BLK_ATOMS = 64;  // block capacity (rows of the blocked layouts)
constexpr int BLK_MOLS = 64;                     // molecules per block (empty molecules have no rows)
// gather entries per row in the block-local ELL form (WdGraph.*_ell_*, WDMPNN_ELL_WIDTH; 12 measured
// no faster than 8 on the polymer benchmark, whose longest rows have 9 entries)
constexpr int ELLW = 8;
static_assert(ELLW % 4 == 0, "ELL rows of whole 4-byte index words and float4 weight groups");

// one prefetched ELL row: ELLW uint8 indices (bit 7 of the last = "more entries in the CSR list") and
// ELLW weights (0 = empty slot)
struct EllRow {
    uint32_t ix[ELLW / 4];
    float w[ELLW];
};
__device__ __forceinline__ EllRow ell_zero() {
    EllRow e;
    for (int k = 0; k < ELLW / 4; ++k) e.ix[k] = 0;
    for (int k = 0; k < ELLW; ++k) e.w[k] = 0.f;
    return e;
}
__device__ __forceinline__ EllRow ell_load(const uint8_t *idx, const float *coef, size_t row) {
    EllRow e;
    const uint32_t *ip = reinterpret_cast<const uint32_t *>(idx + ELLW * row);
    const float *cp = coef + ELLW * row;
#pragma unroll
    for (int q = 0; q < ELLW / 4; ++q) {
        e.ix[q] = ip[q];
        const float4 w = ld4(cp + 4 * q);
        e.w[4 * q] = w.x; e.w[4 * q + 1] = w.y; e.w[4 * q + 2] = w.z; e.w[4 * q + 3] = w.w;
    }
    return e;
}
__device__ __forceinline__ int ell_idx(const EllRow &e, int k) { return (e.ix[k >> 2] >> (8 * (k & 3))) & 0x7f; }
__device__ __forceinline__ bool ell_more(const EllRow &e) { return e.ix[ELLW / 4 - 1] & 0x80000000u; }

// WdGraph.blocks row: {bond_start, bond_count, atom_start, atom_count, mol_lo, mol_hi, -, -}
struct BlockRow { int bs, bn, as, an, ml, mh; };
__device__ __forceinline__ BlockRow load_block(const int32_t *blocks, int i) {
    const int4 a = *reinterpret_cast<const int4 *>(blocks + 8 * i);
    const int2 b = *reinterpret_cast<const int2 *>(blocks + 8 * i + 4);
    return BlockRow{a.x, a.y, a.z, a.w, b.x, b.y};
}

// The same row through the constant address space: a scalar load whatever the compiler can prove about the
// pointer (the pair kernels' loader waves got a vector load, whose vmcnt(0) wait also waited for every copy
// issued before it).  `blocks` is written by an earlier launch and i is workgroup-uniform.
__device__ __forceinline__ BlockRow load_block_s(const int32_t *blocks, int i) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef int v2i __attribute__((ext_vector_type(2)));
    const auto *q = (const __attribute__((address_space(4))) int32_t *)(blocks + 8 * i);
    const v4i a = *reinterpret_cast<const __attribute__((address_space(4))) v4i *>(q);
    const v2i b = *reinterpret_cast<const __attribute__((address_space(4))) v2i *>(q + 4);
    return BlockRow{a.x, a.y, a.z, a.w, b.x, b.y};
}
// ... and its atom and molecule fields alone (W_o + readout: loaded whole, the two unused registers of the
// 16-byte load were reused at once, and the write-after-write wait for them stood ahead of the role branch)
__device__ __forceinline__ BlockRow load_block_atoms_s(const int32_t *blocks, int i) {
    typedef int v2i __attribute__((ext_vector_type(2)));
    const auto *q = reinterpret_cast<const __attribute__((address_space(4))) v2i *>(
        (const __attribute__((address_space(4))) int32_t *)(blocks + 8 * i));
    const v2i a = q[1], b = q[2];
    return BlockRow{0, 0, a.x, a.y, b.x, b.y};
}

// s += w * T[j][c .. c+7] (LDS tile, row stride LDC)
template <int LDC>
__device__ __forceinline__ void lds_term(const float *T, int j, int c, float w, float4 &s0, float4 &s1) {
    fma4(s0, w, ld4(T + j * LDC + c));
    fma4(s1, w, ld4(T + j * LDC + c + 4));
}

struct MpLayerP {
    // The entry head: what the pair layers read before their main loop, adjacent and first, so that the entry
    // copies it with one batch of scalar loads and one wait (mp_layer_kernel; 15 dwords).  Everything after it
    // is first touched by the loaders' hook or the epilogue.
    const uint8_t *ain;         // (pair-operand layers, below)
    const uint8_t *wh;          // W_h h2 plane tiles [Hk][Hk] with BN-row blocks
    const int32_t *blocks;
    const uint32_t *amax_in;    // the scale words of M_{t-1} (planes.hpp h2): [nblk][amax_in_n] maxima of |M_{t-1}|,
    const uint32_t *wh_amax;    // W_h's scale word (max |W_h|, wdmpnn_pack_params)
    int kp;                     // Hk
    int n_tiles;                // Hk / BN
    uint32_t tmagic;            // tile_magic(n_tiles): tile -> (block, column tile) without a division (common.hpp)
    int amax_in_n;              // published per (block, tile) by the embed or by layer t - 1; amax_rt > 0:
    int ain_g;                  // (pair-operand layers, below)
    const float *zin;           // Z_{t-1}: fp32 natural bond rows [Rp][kp] (the first layer: inp, mpn.py:95); the
                                // GEMM operand is M_{t-1} = dropout(act(Z_{t-1})) (mpn.py:97, 123-124), formed
                                // while staging
    int amax_rt;                // amax_in: per (amax_rt-row tile of zin, column tile) by the input GEMM (gemm_x6g's
                                //   Epi.amax): the words of the row tiles the block's rows overlap
    int ldz, ldr;               // row strides of zin and of the residual inp (Hk, or wider for column slices)
    float p_drop_in;            // the dropout of M_{t-1} (0 for M_0: mpn.py:97 drops nothing)
    float *zout;                // Z_t, same layout (null in the last layer)
    uint32_t *amax_out;         // [nblk][n_tiles]: max |dropout(act(Z_t))| of each workgroup (not the last layer)
    const float *inp;           // fp32 [Rp][Hk] natural rows (mpn.py:95 input)
    const float *bias;          // b_h (padded) or null
    const int32_t *rev;         // b2revb (natural bond ids)
    const uint8_t *src_blk;     // per natural bond row: block-local source atom (b2a)
    int undirected;             // mpn.py:101-102
    int act; const float *slope; float p_drop; uint64_t seed; uint32_t layer;
    const int32_t *aptr, *aidx; const float *acoef;  // atom gather (natural atom rows -> natural bond rows)
    const uint8_t *aell_idx; const float *aell_coef; // its first ELLW entries per row, block-local (WdGraph)
    uint8_t *aplanes;           // A: blocked atom plane tiles [nblk * 64][kp] (the last layer)
    // training forward (save_for_backward) or null, the last layer only (the others' Z_t is zout): its
    // pre-activation Z_t (mpn.py:123) as fp32 natural bond rows [Rp][kp] and the atom aggregate A
    // (mpn.py:126-131) as fp32 natural atom rows [Vap][kp] (the backward's operands)
    float *zsave, *asave;
    // atom-message mode (mpn.py:47-53, 93-94, 104-108; the template's ATOM): the message rows are the
    // block's atoms, inp is the residual inp + (sum over a2b of the bond features) W_h[:, H:]^T, and the
    // gather is the a2a neighbour sum X[a] = sum_{a' in nbr(a)} P[a'] (no reverse term), from these lists
    // (block-local ELL over atom rows); aptr / aell above stay the final
    // aggregate (mpn.py:126-131).  The ELL lists drop the a2a pad slots (atom 0, whose message is zero
    // without biases); rows longer than the ELL width continue in the CSR list msg_gather, whose pad-slot
    // entry (atom 0, outside every block) is skipped
    const uint8_t *mell_idx; const float *mell_coef;
    const int32_t *mptr, *midx; const float *mcoef;
    // pair-operand layers (the template's PAIRS, round 6): M_{t-1} comes as fp16 hi / lo pair tiles of the
    // molecule blocks ([nblk][Hk / 32 chunks][2 planes][128 rows][64 B]), scaled per group of ain_g columns
    // by the words amax_in [nblk][amax_in_n] (the embed: 32-column groups; a layer: its BN-column tiles),
    // and the layer writes M_t the same way into aout (not the last layer), scaled by its tile's max
    // (ain, ain_g: in the entry head)
    uint8_t *aout;
    // ... and the last layer writes the atom aggregate A as pair tiles of the blocks' atom rows ([nblk][Hk / 32]
    // [2][64][64 B], W_o's A operand: wo_readout_kernel<..., PAIRS>), scaled by its tile's max, published in
    // amax_out [nblk][n_tiles]
    uint8_t *apairs;
};

// The GEMM operand M_{t-1} = dropout(act(Z_{t-1})), formed while staging from the fp32 Z rows (the
// producer waves of h2_mainloop_ws), so that no message tensor goes through HBM in split form: producer
// thread t (0..255) stages rows t / 4 and t / 4 + 64 of the block, columns 8 (t % 4) .. +7 of each
// 32-column chunk, applies the activation and dropout, scales and splits into fp16 hi / lo.  The rows are
// read through a buffer resource that ends at the block's last bond: rows past it come back as zeros
// without touching memory (a QM9 block holds ~14 of the 128 rows), with the same instruction stream in
// every wave, so the compiler's vmcnt waits stay exact; only the 16-row tiles the consumers multiply are
// converted and stored.  (8 lanes per row, one 16-byte load each, measured +0.5 us per launch.)
template <int BM, int AACT>
struct H2Prod {
    static constexpr int U = BM / 64;                    // rows per producer thread
    static constexpr int SETS = 3;                       // register sets (chunks in flight)
    __amdgpu_buffer_rsrc_t rs;              // the block's Z rows
    int off[U];                             // byte offset of this thread's columns in row r0 + 64 i
    uint32_t grow[U];                       // natural bond row (dropout counter)
    int r0, u, live16;                      // live16: rows of the 16-row tiles holding bonds
    float slope, scale, pd;
    uint64_t seed;
    uint32_t layer;
    uint32_t wv;                            // this lane's scale word (lane_word, loaded by the caller)
    u32x4 v[SETS][U][2];                    // register sets (raw fp32 bits)
    __device__ __forceinline__ void init() { scale = h2_scale(wave_max_u32(wv)); }
    // rows rs .. rs + rn - 1 of zin (the block's bonds, or its atoms in atom-message mode)
    __device__ __forceinline__ H2Prod(const MpLayerP &P, int rs0, int rn, uint32_t words) {
        const int t = threadIdx.x & 255;
        r0 = t >> 2; u = t & 3;
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.zin + (size_t)rs0 * P.ldz), 0,
                                               rn > 0 ? ((rn - 1) * P.ldz + P.kp) * 4 : 0, 0x00020000);
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int r = r0 + 64 * i;
            grow[i] = r < rn ? rs0 + r : 0;
            off[i] = (r * P.ldz + 8 * u) * 4;
        }
        live16 = (rn + 15) & ~15;
        slope = AACT == ACT_PRELU ? P.slope[0] : 0.f;
        wv = words;
        scale = 1.f;
        pd = P.p_drop_in;
        seed = P.seed;
        layer = P.layer - 1;
    }
    template <typename S>
    __device__ __forceinline__ void load(S, int kc) {
#pragma unroll
        for (int i = 0; i < U; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                v[S::value][i][h] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off[i] + 128 * kc + 16 * h, 0, 0));
    }
    template <typename S>
    __device__ __forceinline__ void store(S, int kc, uint8_t *st) {
        // (a use of every register of the set outside the row branch below: the compiler otherwise sank
        // the first set's second-row loads into that branch, right in front of their use)
#pragma unroll
        for (int i = 0; i < U; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) asm volatile("" ::"v"(v[S::value][i][h]));
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int r = r0 + 64 * i;
            if (r >= live16) continue;  // (the consumers skip those 16-row tiles)
            float x[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const u32x4 a = v[S::value][i][h];
                x[4 * h] = __uint_as_float(a.x); x[4 * h + 1] = __uint_as_float(a.y);
                x[4 * h + 2] = __uint_as_float(a.z); x[4 * h + 3] = __uint_as_float(a.w);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = act_fwd(AACT, x[q], slope);
            if (pd > 0.f)
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] *= dropout_scale(seed, layer, grow[i], 32 * kc + 8 * u + q, pd);
            uint32_t hh[4], ll[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) split_h2(x[2 * q], x[2 * q + 1], scale, hh[q], ll[q]);
            uint8_t *d = st + x6_slot(r, u);
            *reinterpret_cast<u32x4 *>(d) = u32x4{hh[0], hh[1], hh[2], hh[3]};
            *reinterpret_cast<u32x4 *>(d + BM * 64) = u32x4{ll[0], ll[1], ll[2], ll[3]};
        }
    }
};

// The fused layer kernel runs 512 threads, warp-specialised: 4 MFMA waves of 32 rows x all BN columns and
// their 4 staging partners (gemm_x6.hpp h2_mainloop_ws); the epilogue runs on all 512.  80-column tiles
// give 4 tiles for Hk = 320 and so exactly one workgroup per CU at the benchmark size (64 blocks x 4 =
// 256): a grid of 1.25 workgroups per CU left a quarter of the CUs with twice the bytes to stream.
constexpr int MP_THREADS = 512;

// mp_layer epilogue: the gather G applied to the P = M_{t-1} W_h^T tile in LDS in the reference's two
// steps (mpn.py:110-120), then bias, residual and the fp32 stores of Z_t (with the maximum of
// dropout(act(Z_t)) published for the next layer's scale) -- or, in the last layer, activation, dropout
// and the atom aggregate of M_t (mpn.py:126-131):
//     (undirected: P <- (P + P[rev]) / 2, mpn.py:101-102)
//     A[a] = sum_{b into a} w_b P[b]      (the block's atoms, slot order, into LDS)
//     X[b] = A[src(b)] - P[rev(b)]
// Only the atom gather lists and the rows' source / reverse ids are prefetched during the GEMM (a few
// registers: with <= 128 VGPRs two layer workgroups co-reside on a CU -- one's epilogue beside the
// other's GEMM when batches are in flight on two streams); the residual rows are loaded when the
// epilogue starts and land behind the atom sums.
template <int BN, int NT, bool LAST, bool ATOM = false, bool POUT = false>
struct MpEpilogue {
    static constexpr int BM = BLK_BONDS, LDC = BN + 4;
    static constexpr int UPR = BN / 8, UNITS = BM * UPR, UPT = (UNITS + NT - 1) / NT;  // 8-column units
    static constexpr int AUNITS = BLK_ATOMS * UPR, AUPT = (AUNITS + NT - 1) / NT;
    static constexpr int LDS_FLOATS = (BM + BLK_ATOMS) * LDC;  // P tile, then the atom sums
    static constexpr int YPT = ATOM ? AUPT : UPT;              // units of M_t per thread (rows: atoms | bonds)
    EllRow aell[AUPT];               // bond mode: the atom gather; atom mode: the a2a neighbour lists
    EllRow gell[ATOM && LAST ? AUPT : 1];  // atom mode, last layer: the final aggregate's lists
    int32_t rv[ATOM ? 1 : UPT];
    uint32_t sa[ATOM ? 1 : UPT];

    // The gather rows of the block's atoms (unit v = tid + NT i: atom v / UPR) and, in bond mode, the source /
    // reverse ids of its bond rows (unit v: row v / UPR), handed over through LDS: the staging waves, done one
    // chunk before the MFMA waves, load them for the whole block while the last chunk is multiplied (fill_pre),
    // and every thread reads its units' rows from LDS after the barrier (take_pre) -- no memory latency after
    // the GEMM.
    static constexpr int PRE_ELL = BLK_ATOMS * (int)sizeof(EllRow);
    static constexpr int PRE_BYTES = PRE_ELL * (ATOM && LAST ? 2 : 1) + (ATOM ? 0 : BM * 8);
    // one staging thread's share of the lists: loaded into registers (plain loads, nothing computed on what
    // they return), then stored into the `pre` area
    struct Pre {
        EllRow e, f;  // (f: ATOM && LAST only)
        int2 q;
    };
    __device__ __forceinline__ void load_pre(const MpLayerP &P, const BlockRow &B, Pre &R) {
        const int t = threadIdx.x - MP_THREADS / 2;  // (staging threads 0 .. 255)
        R.e = ell_zero();
        if (t < B.an) R.e = ATOM ? ell_load(P.mell_idx, P.mell_coef, (size_t)B.as + t)
                                 : ell_load(P.aell_idx, P.aell_coef, (size_t)B.as + t);
        if constexpr (ATOM && LAST) {
            R.f = ell_zero();
            if (t < B.an) R.f = ell_load(P.aell_idx, P.aell_coef, (size_t)B.as + t);
        }
        if constexpr (!ATOM) {
            R.q = make_int2(0, 0);
            if (t < B.bn) R.q = make_int2(P.rev[B.bs + t], (int)P.src_blk[B.bs + t]);
        }
    }
    __device__ __forceinline__ void store_pre(const Pre &R, uint8_t *pre) {
        const int t = threadIdx.x - MP_THREADS / 2;
        if (t < BLK_ATOMS) {
            reinterpret_cast<EllRow *>(pre)[t] = R.e;
            if constexpr (ATOM && LAST) reinterpret_cast<EllRow *>(pre + PRE_ELL)[t] = R.f;
        }
        if constexpr (!ATOM)
            if (t < BM) reinterpret_cast<int2 *>(pre + PRE_ELL)[t] = R.q;
    }
    __device__ __forceinline__ void fill_pre(const MpLayerP &P, const BlockRow &B, uint8_t *pre) {
        Pre R;
        load_pre(P, B, R);
        store_pre(R, pre);
    }
    __device__ __forceinline__ void take_pre(const BlockRow &B, const uint8_t *pre) {
        const int tid = threadIdx.x;
#pragma unroll
        for (int i = 0; i < AUPT; ++i) {
            const int v = tid + NT * i, la = min(v / UPR, BLK_ATOMS - 1);
            aell[i] = reinterpret_cast<const EllRow *>(pre)[la];
            if constexpr (ATOM && LAST) gell[i] = reinterpret_cast<const EllRow *>(pre + PRE_ELL)[la];
        }
        if constexpr (!ATOM)
#pragma unroll
            for (int i = 0; i < UPT; ++i) {
                const int v = tid + NT * i, lr = min(v / UPR, BM - 1);
                const int2 q = reinterpret_cast<const int2 *>(pre + PRE_ELL)[lr];
                rv[i] = q.x;
                sa[i] = (uint32_t)q.y;
            }
    }

    // s = sum over the row's entries (ELL slots, then the CSR rest: natural ids, base = the block's first
    // row of the gathered kind; entries below it -- the atom-message pad slot -- skipped) of w * T[entry][c .. c + 7]
    __device__ __forceinline__ void row_sum(const int32_t *ptr, const int32_t *idx, const float *coef, int row, int base,
                                            const EllRow &E, int c, const float *T, float4 &s0, float4 &s1) {
        s0 = s1 = f4zero();
#pragma unroll
        for (int k = 0; k < ELLW; ++k)
            if (E.w[k] != 0.f) lds_term<LDC>(T, ell_idx(E, k), c, E.w[k], s0, s1);
        if (ell_more(E))
            for (int q = ptr[row] + ELLW; q < ptr[row + 1]; ++q) {
                const int li = idx[q] - base;
                if (li >= 0) lds_term<LDC>(T, li, c, coef ? coef[q] : 1.0f, s0, s1);
            }
    }
    // A[la][c..c+7] = sum over the atom's in-bonds of w * T[bond] (bond mode's atom gather)
    __device__ __forceinline__ void atom_sum(const MpLayerP &P, const BlockRow &B, const EllRow &E, int la, int c,
                                             const float *T, float4 &s0, float4 &s1) {
        row_sum(P.aptr, P.aidx, P.acoef, B.as + la, ATOM ? B.as : B.bs, E, c, T, s0, s1);
    }

    // Pt: the P tile [BM][LDC] fp32 in LDS (every write of it done and synchronised); At = Pt + BM * LDC
    template <int ACT>
    __device__ __forceinline__ void run(const MpLayerP &P, const BlockRow &B, int blk, int n0, float *Pt) {
        const int tid = threadIdx.x;
        float *At = Pt + BM * LDC;
        // message rows of this block: bonds, or atoms in atom-message mode
        const int rs = ATOM ? B.as : B.bs, rn = ATOM ? B.an : B.bn;
        constexpr int NU = ATOM ? AUNITS : UNITS, PT = ATOM ? AUPT : UPT;
        // residual rows (mpn.py:123 input): issued now, consumed after the gathers
        float4 res[PT][2];
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int v = tid + NT * i, lr = v / UPR, c = 8 * (v % UPR);
            res[i][0] = res[i][1] = f4zero();
            if (v < NU && lr < rn) {
                const float *s = P.inp + (size_t)(rs + lr) * P.ldr + n0 + c;
                res[i][0] = ld4(s);
                res[i][1] = ld4(s + 4);
            }
        }
        if constexpr (!ATOM) {
            if (P.undirected) {  // P <- (P + P[rev]) / 2, one thread per reverse pair (the lower row)
#pragma unroll
                for (int i = 0; i < UPT; ++i) {
                    const int v = tid + NT * i, lr = v / UPR, c = 8 * (v % UPR);
                    const int rl = rv[i] - B.bs;
                    if (v < UNITS && lr < B.bn && lr < rl) {
                        float4 p0 = ld4(Pt + lr * LDC + c), p1 = ld4(Pt + lr * LDC + c + 4);
                        const float4 q0 = ld4(Pt + rl * LDC + c), q1 = ld4(Pt + rl * LDC + c + 4);
                        p0.x = (p0.x + q0.x) / 2.0f; p0.y = (p0.y + q0.y) / 2.0f;
                        p0.z = (p0.z + q0.z) / 2.0f; p0.w = (p0.w + q0.w) / 2.0f;
                        p1.x = (p1.x + q1.x) / 2.0f; p1.y = (p1.y + q1.y) / 2.0f;
                        p1.z = (p1.z + q1.z) / 2.0f; p1.w = (p1.w + q1.w) / 2.0f;
                        st4(Pt + lr * LDC + c, p0); st4(Pt + lr * LDC + c + 4, p1);
                        st4(Pt + rl * LDC + c, p0); st4(Pt + rl * LDC + c + 4, p1);
                    }
                }
                __syncthreads();
            }
            wd_stamp(4 + 8 * LAST);
            // A[a] = sum_{b into a} w_b P[b] (mpn.py:112-118)
#pragma unroll
            for (int i = 0; i < AUPT; ++i) {
                const int v = tid + NT * i, la = v / UPR, c = 8 * (v % UPR);
                if (v >= AUNITS || la >= B.an) break;
                float4 s0, s1;
                atom_sum(P, B, aell[i], la, c, Pt, s0, s1);
                st4(At + la * LDC + c, s0);
                st4(At + la * LDC + c + 4, s1);
            }
            __syncthreads();
            wd_stamp(5 + 8 * LAST);
        }
        const float slope = ACT == ACT_PRELU ? P.slope[0] : 0.f;
        float4 ym[LAST || POUT ? YPT : 1][2];  // LAST: this thread's M_t units until P is dead; POUT: until the scale is known
        // Z_t rows of this block (the training forward's save in the last layer)
        float *zr = LAST ? P.zsave : P.zout;
        const __amdgpu_buffer_rsrc_t zrs = __builtin_amdgcn_make_buffer_rsrc(zr ? (void *)(zr + (size_t)rs * P.kp) : (void *)P.inp, 0,
                                                                            BM * P.kp * 4, 0x00020000);
        uint32_t mx = 0;               // max |dropout(act(Z_t))| of this thread's units (not LAST)
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int v = tid + NT * i, lr = v / UPR, c = 8 * (v % UPR);
            if (v >= NU) break;
            float4 y0 = f4zero(), y1 = f4zero();
            if (lr < rn) {
                const int b = rs + lr;
                float z[8];
                if constexpr (ATOM) {
                    // X[a] = sum_{a' in nbr(a)} P[a'] (mpn.py:104-108, the W_h[:, :H] part; the bond-feature
                    // part is in the residual)
                    float4 s0, s1;
                    row_sum(P.mptr, P.midx, P.mcoef, b, B.as, aell[i], c, Pt, s0, s1);
                    z[0] = s0.x; z[1] = s0.y; z[2] = s0.z; z[3] = s0.w; z[4] = s1.x; z[5] = s1.y; z[6] = s1.z; z[7] = s1.w;
                } else {
                    const int rl = rv[i] - B.bs, a = (int)sa[i];
                    // X[b] = A[src(b)] - P[rev(b)] (mpn.py:119-120)
                    const float4 a0 = ld4(At + a * LDC + c), a1 = ld4(At + a * LDC + c + 4);
                    const float4 q0 = ld4(Pt + rl * LDC + c), q1 = ld4(Pt + rl * LDC + c + 4);
                    z[0] = a0.x - q0.x; z[1] = a0.y - q0.y; z[2] = a0.z - q0.z; z[3] = a0.w - q0.w;
                    z[4] = a1.x - q1.x; z[5] = a1.y - q1.y; z[6] = a1.z - q1.z; z[7] = a1.w - q1.w;
                }
                float4 b0 = f4zero(), b1 = f4zero();
                if (P.bias) { b0 = ld4(P.bias + n0 + c); b1 = ld4(P.bias + n0 + c + 4); }
                const float r8[8] = {res[i][0].x, res[i][0].y, res[i][0].z, res[i][0].w,
                                     res[i][1].x, res[i][1].y, res[i][1].z, res[i][1].w};
                const float b8[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int q = 0; q < 8; ++q) z[q] = r8[q] + (z[q] + b8[q]);  // mpn.py:122-123
                // (16-byte buffer stores, default write-back policy: write-through, as the planes use, measured
                // slower on the first polymer layer -- 17.46 us against 16.50, same box)
                if (zr) {
                    const int o = (lr * P.kp + n0 + c) * 4;
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(z[0]), __float_as_uint(z[1]),
                                                                 __float_as_uint(z[2]), __float_as_uint(z[3])}, zrs, o, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(z[4]), __float_as_uint(z[5]),
                                                                 __float_as_uint(z[6]), __float_as_uint(z[7])}, zrs, o + 16, 0, 0);
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) z[q] = act_fwd(ACT, z[q], slope);
                if (P.p_drop > 0.f)
#pragma unroll
                    for (int q = 0; q < 8; ++q) z[q] *= dropout_scale(P.seed, P.layer, b, n0 + c + q, P.p_drop);
                if constexpr (!LAST)
#pragma unroll
                    for (int q = 0; q < 8; ++q) mx = max(mx, absbits(z[q]));
                y0 = make_float4(z[0], z[1], z[2], z[3]);
                y1 = make_float4(z[4], z[5], z[6], z[7]);
            }
            if constexpr (LAST || POUT) {
                ym[i][0] = y0;
                ym[i][1] = y1;
            }
        }
        if constexpr (!LAST && POUT) {
            // M_t as fp16 pairs scaled by this tile's max (the next layer's A operand, copied by LDS-DMA)
            __shared__ uint32_t red[MP_THREADS / 64];
            const float s = h2_scale(publish_max_all(mx, P.amax_out + (size_t)blk * P.n_tiles + n0 / BN, red));
            constexpr int CH = 2 * BM * 64;
            const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
                P.aout + (size_t)blk * (P.kp >> 5) * CH, 0, (P.kp >> 5) * CH, 0x00020000);
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const int v = tid + NT * i, lr = v / UPR, c = 8 * (v % UPR);
                // (rows up to the end of the last 16-row group the consumers multiply: zeros past the block)
                if (v >= NU || lr >= ((rn + 15) & ~15)) break;
                h2_store8(prs, h2_blk_off<BM>(lr, n0 + c), BM * 64, ym[i][0], ym[i][1], s);
            }
        } else if constexpr (!LAST) {
            __shared__ uint32_t red[MP_THREADS / 64];
            publish_max(mx, P.amax_out + (size_t)blk * P.n_tiles + n0 / BN, red);
        }
        if constexpr (LAST) {
            __syncthreads();  // every read of P done: M_t replaces it
            float *Mt = Pt;
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const int v = tid + NT * i, lr = v / UPR, c = 8 * (v % UPR);
                if (v >= NU) break;
                st4(Mt + lr * LDC + c, ym[i][0]);
                st4(Mt + lr * LDC + c + 4, ym[i][1]);
            }
            __syncthreads();
            // atom aggregate of this column tile: A[a] = sum_{x into a} w M_t[x] (mpn.py:126-131; x: the
            // atom's in-bonds, or its a2a neighbours in atom-message mode)
            if (POUT && P.apairs) {
                // A as fp16 pairs scaled by this tile's max (rows to the end of the last 16-row group: zeros)
                float4 as[AUPT][2];
                uint32_t amx = 0;
#pragma unroll
                for (int i = 0; i < AUPT; ++i) {
                    const int v = tid + NT * i, la = v / UPR, c = 8 * (v % UPR);
                    as[i][0] = as[i][1] = f4zero();
                    if (v < AUNITS && la < B.an) {
                        atom_sum(P, B, aell[i], la, c, Mt, as[i][0], as[i][1]);
                        const float q[8] = {as[i][0].x, as[i][0].y, as[i][0].z, as[i][0].w,
                                            as[i][1].x, as[i][1].y, as[i][1].z, as[i][1].w};
#pragma unroll
                        for (int k = 0; k < 8; ++k) amx = max(amx, absbits(q[k]));
                    }
                }
                __shared__ uint32_t red[MP_THREADS / 64];
                const float s = h2_scale(publish_max_all(amx, P.amax_out + (size_t)blk * P.n_tiles + n0 / BN, red));
                constexpr int CHA = 2 * BLK_ATOMS * 64;
                const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
                    P.apairs + (size_t)blk * (P.kp >> 5) * CHA, 0, (P.kp >> 5) * CHA, 0x00020000);
#pragma unroll
                for (int i = 0; i < AUPT; ++i) {
                    const int v = tid + NT * i, la = v / UPR, c = 8 * (v % UPR);
                    if (v >= AUNITS || la >= ((B.an + 15) & ~15)) break;
                    h2_store8(prs, h2_blk_off<BLK_ATOMS>(la, n0 + c), BLK_ATOMS * 64, as[i][0], as[i][1], s);
                }
            } else {
            const __amdgpu_buffer_rsrc_t ars = x6_block_rsrc<BLK_ATOMS>(P.aplanes, P.kp, blk);
#pragma unroll
            for (int i = 0; i < AUPT; ++i) {
                const int v = tid + NT * i, la = v / UPR, c = 8 * (v % UPR);
                if (v >= AUNITS || la >= B.an) break;  // rows past the block's atoms are never loaded
                float4 s0, s1;
                if constexpr (ATOM) atom_sum(P, B, gell[i], la, c, Mt, s0, s1);
                else atom_sum(P, B, aell[i], la, c, Mt, s0, s1);
                x6_store8_blk<BLK_ATOMS>(ars, la, n0 + c, s0, s1);
                if (P.asave) {
                    float *ar = P.asave + (size_t)(B.as + la) * P.kp + n0 + c;
                    st4(ar, s0);
                    st4(ar + 4, s1);
                }
            }
            }
        }
    }
};

// grid = nblk * n_tiles (XCD-grouped: the column tiles of a block share an XCD), MP_THREADS threads.
// LDS: two GEMM stages, reused by the epilogue as P [128][BN + 4] fp32 + the atom sums; the last layer
// then overwrites P with M_t (held in registers across a barrier) for the atom aggregate.
// ACT: the activation (one instantiation each: the staging of M_{t-1} and the epilogue fold it to
// straight-line code).
template <int BN, bool LAST, int ACT, bool ATOM = false, int NJ = WD_MULTI, bool PAIRS = false>
// (__launch_bounds__ min 4 waves per SIMD: <= 128 VGPRs, so that two layer workgroups -- batches in flight
// on two streams -- co-reside on a CU)
__global__ __launch_bounds__(MP_THREADS, 4) void mp_layer_kernel(const Multi<MpLayerP, NJ> MP) {
    constexpr int BM = BLK_BONDS;
    using Epi_ = MpEpilogue<BN, MP_THREADS, LAST, ATOM, PAIRS>;
    constexpr int EPI_BYTES = Epi_::LDS_FLOATS * 4;  // P tile + the atom sums
    constexpr int STG_BYTES = PAIRS ? h2p_lds_bytes<BM, BN>() : h2_lds_bytes<BM, BN>();
    constexpr int LDS_BYTES = EPI_BYTES > STG_BYTES ? EPI_BYTES : STG_BYTES;
    static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    int tile;
    wd_stamp(0 + 8 * LAST);
    const MpLayerP &P = multi_pick(MP, xcd_tile(blockIdx.x, gridDim.x), tile);
    // The entry head by value (PAIRS: all of it, pinned in scalar registers -- one batch of loads, one wait;
    // the register-staged kernels pin nothing and read their arguments where they did: pinned, their
    // allocation moved from 108-110 to 118-123 VGPRs for nothing measured).
    auto hv = [](auto v) {
        if constexpr (PAIRS) return pin_s(v);
        else return v;
    };
    const int h_nt = hv(P.n_tiles), h_kp = hv(P.kp);
    const uint32_t h_tm = hv(P.tmagic);
    const int32_t *h_blocks = hv(P.blocks);
    const uint8_t *h_ain = nullptr, *h_wh = hv(P.wh);
    const uint32_t *h_amax_in = nullptr, *h_wh_amax = nullptr;
    int h_amax_in_n = 0, h_ain_g = 0;
    if constexpr (PAIRS) {
        h_ain = pin_s(P.ain); h_amax_in = pin_s(P.amax_in); h_wh_amax = pin_s(P.wh_amax);
        h_amax_in_n = pin_s(P.amax_in_n); h_ain_g = pin_s(P.ain_g);
    }
    int blk, nt;
    tile_split(tile, h_nt, h_tm, blk, nt);
    const int n0 = nt * BN;
    // (PAIRS: a scalar load issued here, ahead of the role branch, and waited for by each role where it first
    // needs the row -- the loaders after their first weight copies have left, h2_mainloop_pairs)
    BlockRow B = PAIRS ? load_block_s(h_blocks, blk) : load_block(h_blocks, blk);
    Epi_ E;
    float *Pt = reinterpret_cast<float *>(lds);
    // Two GEMM front ends.  After either, both run the same steps -- the lists into E, the scaled tile into Pt,
    // the epilogue, the pad rows -- written out twice: shared through a function, a lambda or common code after
    // the branch, they compile to the same instructions with other register numbers in the register-staged
    // kernels, and these kernels are compared byte for byte with their predecessors.
    if constexpr (PAIRS) {
        static_assert(!ATOM, "pair operands: bond messages");
        // the epilogue's gather lists and ids, staged by the loader waves while the consumers multiply the
        // last chunk, in the tail of ring stage 2 (the last chunk lands in stage 0): clear of the P tile and
        // the atom sums the epilogue writes
        static_assert(EPI_BYTES + Epi_::PRE_BYTES <= STG_BYTES, "epilogue lists beside the P tile");
        uint8_t *pre = lds + STG_BYTES - Epi_::PRE_BYTES;
        // (the row's scalar load is in flight since the entry: nothing of the loaders' waits on vector memory
        // between the entry and their first A copy)
        auto rows = [&]() { return B.bn; };
        // (W_h's word too: only the consumers' epilogue step needs it, and a dependent load ahead of the role
        // branch stood between the loaders and their first copies.  The consumers issue the row, the words and
        // this word together -- all three addresses come from the head -- and wait once.)
        uint32_t whm = 0;
        auto words = [&]() {
            whm = *h_wh_amax;
            return lane_word(h_amax_in + (size_t)blk * h_amax_in_n, h_amax_in_n);
        };
        wd_stamp(1 + 8 * LAST);
        floatx4 acc[BM / 64][BN / 16];
        int se;
        constexpr int CH = 2 * BM * 64;
        // the lists: loaded by the loaders after their last copy (before their loop, held in registers:
        // "all waves past the GEMM" 0.5 -> 0.16 us per layer alone, the headline the same -- 218.6 vs 218.9 M
        // edges/s, DESIGN.md "Measured dead ends" -- not kept)
        struct PreHook {
            Epi_ &E; const MpLayerP &P; const BlockRow &B; uint8_t *pre;
            typename Epi_::Pre R;
            __device__ __forceinline__ void finish() {
                E.load_pre(P, B, R);
                E.store_pre(R, pre);
            }
        } hook{E, P, B, pre, {}};
        h2_mainloop_pairs<BM, BN, true>(h_ain + (size_t)blk * (h_kp >> 5) * CH, h_wh + (size_t)nt * (h_kp >> 5) * (2 * BN * 64),
                                  h_kp >> 5, rows, words, h_ain_g, lds, acc, se, hook);
        wd_stamp(2 + 8 * LAST);
        __syncthreads();
        E.take_pre(B, pre);
        wd_stamp(3 + 8 * LAST);
        if (threadIdx.x < 256) {  // (the consumer waves hold the tile)
            const float ia = se >= 0 ? __uint_as_float((uint32_t)(254 - se) << 23) : 1.f;
            x6_acc_to_lds<BM, BN, 4, 1, true>(acc, Pt, ia, h2_inv_scale(whm));
        }
        __syncthreads();
        E.template run<ACT>(P, B, blk, n0, Pt);
        wd_stamp(6 + 8 * LAST);
        if (blk == 0 && threadIdx.x < BN / 4) {  // (pad rows, as below)
            float *zr = LAST ? P.zsave : P.zout;
            if (zr) st4(zr + n0 + 4 * threadIdx.x, f4zero());
            if (LAST && P.asave) st4(P.asave + n0 + 4 * threadIdx.x, f4zero());
        }
    } else {
        const int rs = ATOM ? B.as : B.bs, rn = ATOM ? B.an : B.bn;  // the block's message rows
        // the block's scale words of M_{t-1} (<= 64, one per lane) and W_h's: loaded before the GEMM's first
        // loads, reduced by the producers before their first stage and by the consumers after the GEMM
        int w0 = blk * P.amax_in_n, wn = P.amax_in_n;
        if (P.amax_rt > 0) {  // (the row tiles of the block's rows)
            const int t0 = rs / P.amax_rt, t1 = (rs + max(rn, 1) - 1) / P.amax_rt;
            w0 = t0 * P.amax_in_n;
            wn = (t1 - t0 + 1) * P.amax_in_n;
        }
        const uint32_t wv = lane_word(P.amax_in + w0, wn);
        const uint32_t whm = *P.wh_amax;
        H2Prod<BM, ACT> ap(P, rs, rn, wv);
        wd_stamp(1 + 8 * LAST);
        floatx4 acc[BM / 64][BN / 16];
        h2_mainloop_ws<BM, BN>(P.wh + (size_t)nt * (P.kp >> 5) * (2 * BN * 64), P.kp >> 5, rn, lds, acc, ap);
        // the epilogue's gather lists and ids: not during the GEMM (live across the GEMM loop they pushed the
        // consumers' accumulators and fragments past 128 VGPRs); the staging waves load them into LDS while the
        // MFMA waves finish the last chunk
        wd_stamp(2 + 8 * LAST);
        __shared__ __attribute__((aligned(16))) uint8_t pre[Epi_::PRE_BYTES];
        static_assert(LDS_BYTES + Epi_::PRE_BYTES + 64 <= 80 * 1024, "two workgroups per CU");
        if (threadIdx.x >= MP_THREADS / 2) E.fill_pre(P, B, pre);
        __syncthreads();
        E.take_pre(B, pre);
        wd_stamp(3 + 8 * LAST);
        const float ia = h2_inv_scale(wave_max_u32(wv));  // (the producers' scale)
        const float iw = h2_inv_scale(whm);
        if (threadIdx.x < 256) x6_acc_to_lds<BM, BN, 4, 1, true>(acc, Pt, ia, iw);  // (the consumer waves hold the tile)
        __syncthreads();
        E.template run<ACT>(P, B, blk, n0, Pt);
        wd_stamp(6 + 8 * LAST);
        // the pad row 0 (bond and atom) belongs to no block: its Z rows are written as zeros (the backward
        // multiplies them by its zero gradients, where an uninitialised NaN would poison them)
        if (blk == 0 && threadIdx.x < BN / 4) {
            float *zr = LAST ? P.zsave : P.zout;
            if (zr) st4(zr + n0 + 4 * threadIdx.x, f4zero());
            if (LAST && P.asave) st4(P.asave + n0 + 4 * threadIdx.x, f4zero());
        }
    }
}

// ------------------------------------------------------------------------------------------------
// embed_kernel: the input layer (mpn.py:92-97) of a compact batch without a GEMM.  Every f_bonds row is
// its source atom's one-hot row + the bond's binary columns (+ mass * 0.01 in the atom's last column,
// featurization.py:190-250, 467-468), so f_bonds[b] W_i^T is a sum of W_i columns:
//     Ea[a]  = sum_{c in code(a)} W_i[:, c] + last(a) W_i[:, Fa-1]          (per atom of the block)
//     inp[b] = Ea[src(b)] + sum_{k in tail(b)} W_i[:, Fa + k] (+ b_i)       (per bond)
//     Eo[a]  = sum_{c in code(a)} W_o[:, c] + last(a) W_o[:, Fa-1]          (the f_atoms half of W_o)
// One workgroup per (block, BN-column tile), the tile's W_o[:, :Fa]^T and then W_i^T rows staged in LDS.
// Writes inp (fp32, natural rows: the residual of every layer, and the first layer's A operand, which
// applies the activation M_0 = act(inp) while staging) and Eo (fp32, blocked atom rows) for
// wo_readout_kernel's epilogue.  Every global load of the workgroup (atom
// codes, both weight tiles, the bonds' source atoms and tail bits) is issued up front, so the kernel
// waits for memory once.
// ------------------------------------------------------------------------------------------------
struct EmbedP {
    // the entry head (19 dwords, adjacent: copied by value at the entry, embed_kernel): everything the up-front
    // loads' addresses are made of
    const WdAtomCode *codes;     // natural atom rows
    const uint8_t *src_blk;      // per natural bond row: block-local source atom
    const uint16_t *tail;        // per natural bond row: bond columns as bits
    const float *wt;             // W_i^T [>= Fb][Hk] (fp32, packed)
    const float *woat;           // W_o[:, :Fa]^T [>= Fa][Hk] (fp32, packed)
    const float *bias;           // b_i (padded) or null
    const int32_t *blocks;
    int Fa, Fb, Hk, n_tiles;
    uint32_t tmagic;             // tile_magic(n_tiles) (common.hpp)
    // ... and what the stores need
    float *eo;                   // [atom rows][Hk] (natural rows)
    float *inp;                  // [Rp][Hk]
    const float *slope;          // PReLU slope (or null)
    uint32_t *amax;              // [nblk][n_tiles]: max |act(inp)| per workgroup (the first layer's scale, planes.hpp h2)
    uint8_t *m0;                 // the template's PAIRS: M_0 = act(inp) as fp16 pair tiles of the molecule blocks
                                 // ([nblk][Hk / 32][2][128][64 B]), scaled by this workgroup's word (the first
                                 // layer's A operand, copied by LDS-DMA: mp_layer_kernel<..., PAIRS>)
};

// Graphs with extra features (the template's XTRA; WdGraph.atom_extra / bond_extra): the rows carry a small dense
// tail behind the codes, f_atoms = [base | xa], f_bonds = [f_atoms[src] | bits | xb], and the sums gain its terms
// in ascending column order, the order of the dense dot product's non-zero terms:
//     Eo[a]  = code sum (W_o) + sum_j xa[a][j] W_o[:, Fa0 + j]                     (Fa0 = Fa - da: the base block)
//     Ea[a]  = code sum (W_i) + sum_j xa[a][j] W_i[:, Fa0 + j]
//     inp[b] = Ea[src(b)] + sum_{k in tail(b)} W_i[:, Fa + k] + sum_j xb[pair(b)][j] W_i[:, Fb - db + j] (+ b_i)
// The weight rows are in the tiles the kernel stages anyway (W_i^T / W_o^T are packed in natural column order);
// the block's xa rows (<= 64 x da) and xb rows (<= 64 pairs x db) are loaded with the other up-front loads into
// LDS (da + db <= EMBED_MAXX, 3.3 KB).  A term whose x is 0.0 leaves its sum bitwise unchanged (fma(0, w, s) = s
// for finite w, and no partial sum is -0), so all-zero extras give the base graph's inp and Eo exactly.
struct EmbedXP : EmbedP {
    const float *xa;             // atom_extra: natural atom rows [n_atoms][da] (da = 0: any readable address)
    const float *xb;             // bond_extra: [pairs][db], directed bond b reads row (b - 1) >> 1 (db = 0: as xa)
    int da, db;
};
constexpr int EMBED_MAXX = 13;   // da + db the embed serves: Fb <= 160 with the default 133 + 14 columns

// s = sum_{c in code} T[c][c4 .. c4+3] + last * T[Fa - 1][c4 ..] (ascending columns, then the mass column:
// the order of the f_atoms row's dot product terms that are not zero)
// Straight-line: the eight slot rows and the mass row are read together and waited for once (a branch per
// slot made nine dependent LDS round trips).  An absent slot (0xFF) reads row 0 of the tile -- staged, in
// bounds -- and adds +0.0f in its place by a select.  Bitwise the same sum as skipping it: s starts at +0 and
// no partial sum of this chain can be -0 (x + y is -0 only for x = y = -0 in round-to-nearest, and s is never
// -0 by induction), so s + (+0) == s for every s, NaN and infinities included.
template <int LDT>
__device__ __forceinline__ float4 code_sum(const WdAtomCode &cd, const float *T, int Fa, int c) {
    float4 w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = ld4(T + (cd.col[q] == 0xFF ? 0 : (int)cd.col[q]) * LDT + c);
    const float4 wm = ld4(T + (Fa - 1) * LDT + c);
    float4 s = f4zero();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const bool on = cd.col[q] != 0xFF;
        s.x += on ? w[q].x : 0.f; s.y += on ? w[q].y : 0.f; s.z += on ? w[q].z : 0.f; s.w += on ? w[q].w : 0.f;
    }
    fma4(s, cd.last, wm);
    return s;
}

template <int BN, int ACT, int NJ = WD_MULTI, bool PAIRS = false, bool XTRA = false>
__global__ __launch_bounds__(512) void embed_kernel(const Multi<std::conditional_t<XTRA, EmbedXP, EmbedP>, NJ> MP) {
    static_assert(!PAIRS || BN % 16 == 0, "pair groups of whole 16-column halves");
    constexpr int NT = 512, LDC = BN + 4, C4 = BN / 4, U8 = BN / 8, MAXK = 160, PER = (MAXK * C4 + NT - 1) / NT;
    constexpr int BU = (BLK_BONDS * U8 + NT - 1) / NT;  // bond units (8 columns of a row) per thread
    __shared__ __attribute__((aligned(16))) float wt[MAXK * BN];        // the staged W_i^T tile
    __shared__ __attribute__((aligned(16))) float ea[BLK_ATOMS * LDC];  // Ea of the block's atoms
    __shared__ __attribute__((aligned(16))) float bb[BN];
    __shared__ WdAtomCode code[BLK_ATOMS];
    // XTRA: the block's extra-feature rows, xa [64][da] then xb [64 pairs][db]
    constexpr int XS = XTRA ? BLK_ATOMS * EMBED_MAXX : 1, XQ = (XS + NT - 1) / NT;
    __shared__ float xs[XS];
    static_assert(sizeof(float) * (MAXK * BN + BLK_ATOMS * LDC + BN + (XTRA ? XS : 0)) + sizeof(WdAtomCode) * BLK_ATOMS <= 80 * 1024,
                  "LDS of two co-resident workgroups");
    static_assert(BLK_BONDS / 2 == BLK_ATOMS, "xb rows: one per pair of the block's bond rows");
    int tile;
    wd_estamp(0);
    const auto &P = multi_pick(MP, xcd_tile(blockIdx.x, gridDim.x), tile);
    // The entry head by value, pinned in scalar registers: one batch of scalar loads and one wait, and every
    // address below is made of registers (through the reference the compiler re-read Hk and the table pointers
    // from the argument segment inside each load's branch: a scalar round trip in front of every vector load).
    const WdAtomCode *h_codes = pin_s(P.codes);
    const uint8_t *h_src = pin_s(P.src_blk);
    const uint16_t *h_tail = pin_s(P.tail);
    const float *h_wt = pin_s(P.wt), *h_woat = pin_s(P.woat), *h_bias = pin_s(P.bias);
    const int32_t *h_blocks = pin_s(P.blocks);
    const int h_Fa = pin_s(P.Fa), h_Fb = pin_s(P.Fb), h_Hk = pin_s(P.Hk), h_nt = pin_s(P.n_tiles);
    const uint32_t h_tm = pin_s(P.tmagic);
    const float *h_xa = nullptr, *h_xb = nullptr;
    int h_da = 0, h_db = 0;
    if constexpr (XTRA) {
        h_xa = pin_s(P.xa); h_xb = pin_s(P.xb);
        h_da = pin_s(P.da); h_db = pin_s(P.db);
    }
    const int fa0 = h_Fa - h_da;  // the base block of an atom row (its last column: the mass)
    int blk, nt;
    tile_split(tile, h_nt, h_tm, blk, nt);
    const int n0 = nt * BN;
    const int tid = threadIdx.x;
    // Every load up front.  The block row (a scalar load) is the one dependent step, and only the codes, the
    // source atoms and the tails need it: it is issued first, the bias and both weight tiles go out while it
    // is in flight, and the three loads that use it follow, in the order their values are needed.
    const BlockRow B = load_block_s(h_blocks, blk);
    float4 bq = f4zero();
    if (tid >= NT - C4 && h_bias) bq = ld4(h_bias + n0 + 4 * (tid - (NT - C4)));
    // (The weight loads are unconditional: a thread whose row k is past the table reads the table's last row,
    // in bounds, and never stores it.  Behind a branch each, the register allocator put a copy of a loaded
    // register into the branch -- and with it a vmcnt(0) wait right behind the load, two memory latencies in a
    // row at the kernel's entry.)
    float4 ro[PER], ri[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int v = tid + NT * q, k = v / C4, c = 4 * (v % C4);
        ro[q] = ld4(h_woat + (size_t)min(k, h_Fa - 1) * h_Hk + n0 + c);
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int v = tid + NT * q, k = v / C4, c = 4 * (v % C4);
        ri[q] = ld4(h_wt + (size_t)min(k, h_Fb - 1) * h_Hk + n0 + c);
    }
    static_assert(sizeof(WdAtomCode) == 16, "codes move as one 16-byte word");
    // (raw words: a struct with a byte array went to scratch.  Unconditional, as the weight loads: a thread
    // past the block's atoms reads the pad atom's row 0 and never stores it.)
    const u32x4 cd = reinterpret_cast<const u32x4 *>(h_codes)[tid < B.an ? B.as + tid : 0];
    uint32_t sa[BU], tl[BU];
#pragma unroll
    for (int u = 0; u < BU; ++u) {
        const int v = tid + NT * u, lb = v / U8;
        sa[u] = tl[u] = 0;
        if (lb < B.bn) {
            sa[u] = h_src[B.bs + lb];
            tl[u] = h_tail[B.bs + lb];
        }
    }
    if constexpr (XTRA) {
        // the block's xa and xb values, both contiguous in memory: element v of xa [an][da] for v < 64 da, then
        // element v - 64 da of xb [bn / 2][db] (the block's first bond id is odd: pair (bs - 1) / 2 is its first).
        // Unconditional, as the loads above: a thread past either range reads element 0 of the array (the pad
        // atom's row, the first pair's row; the host points an absent side at readable memory) and stores 0.
        float xv[XQ];
        const int na = B.an * h_da, nb = (B.bn >> 1) * h_db, xa0 = BLK_ATOMS * h_da;
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int v = tid + NT * q, w = v - xa0;
            const size_t ia = v < na ? (size_t)B.as * h_da + v : 0;
            const size_t ib = w >= 0 && w < nb ? (size_t)((B.bs - 1) >> 1) * h_db + w : 0;
            const float *src = v < xa0 ? h_xa + ia : h_xb + ib;
            xv[q] = *src;
        }
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int v = tid + NT * q, w = v - xa0;
            if (v < XS) xs[v] = (v < xa0 ? v < na : w < nb) ? xv[q] : 0.f;
        }
    }
    if (tid < B.an) reinterpret_cast<u32x4 *>(code)[tid] = cd;
    if (tid >= NT - C4) st4(bb + 4 * (tid - (NT - C4)), bq);
    // The f_atoms half of W_o first.  (Last, while the M_0 stores drain, measured, same box: embed 10.00 vs 10.25
    // us, the bench's single stream 119.2 vs 125.2 M, headline 202.7 vs 204.8 M -- not kept.)  A lambda called
    // once, not straight-line code: written inline, the compiler shares the store addresses with the W_i tile's
    // below and waits for every load before the first W_o store instead of before the last.
    auto eo_half = [&]() {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int v = tid + NT * q, k = v / C4, c = 4 * (v % C4);
            if (k < h_Fa) st4(wt + k * BN + c, ro[q]);
        }
        __syncthreads();
        // Eo[a] = sum_{c in code(a)} W_o[:, c] + last(a) W_o[:, Fa-1] (the f_atoms half of W_o)
        for (int v = tid; v < B.an * C4; v += NT) {
            const int la = v / C4, c = 4 * (v % C4);
            float4 s = code_sum<BN>(code[la], wt, fa0, c);
            if constexpr (XTRA)
                for (int j = 0; j < h_da; ++j) fma4(s, xs[la * h_da + j], ld4(wt + (fa0 + j) * BN + c));
            st4(P.eo + (size_t)(B.as + la) * h_Hk + n0 + c, s);
        }
    };
    eo_half();
    __syncthreads();  // every read of the W_o tile done
    wd_estamp(2);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int v = tid + NT * q, k = v / C4, c = 4 * (v % C4);
        if (k < h_Fb) st4(wt + k * BN + c, ri[q]);
    }
    __syncthreads();
    wd_estamp(3);
    // Ea[a] = sum_{c in code(a)} W_i[:, c] + last(a) W_i[:, Fa-1]
    for (int v = tid; v < B.an * C4; v += NT) {
        const int la = v / C4, c = 4 * (v % C4);
        float4 s = code_sum<BN>(code[la], wt, fa0, c);
        if constexpr (XTRA)
            for (int j = 0; j < h_da; ++j) fma4(s, xs[la * h_da + j], ld4(wt + (fa0 + j) * BN + c));
        st4(ea + la * LDC + c, s);
    }
    __syncthreads();
    wd_estamp(4);
    const float slope = ACT == ACT_PRELU ? P.slope[0] : 0.f;
    uint32_t mx = 0;
    float4 ym[PAIRS ? BU : 1][2];  // PAIRS: this thread's act(inp) units until the scale is known
#pragma unroll
    for (int u = 0; u < (PAIRS ? BU : 1); ++u) ym[u][0] = ym[u][1] = f4zero();
#pragma unroll
    for (int u = 0; u < BU; ++u) {
        const int v = tid + NT * u, lb = v / U8, c = 8 * (v % U8), b = B.bs + lb;
        if (lb >= B.bn) break;
        const int s_ = (int)sa[u];
        float4 z0 = ld4(ea + s_ * LDC + c), z1 = ld4(ea + s_ * LDC + c + 4);
        for (uint32_t m = tl[u]; m; m &= m - 1) {
            const float *w = wt + (h_Fa + __builtin_ctz(m)) * BN + c;
            const float4 w0 = ld4(w), w1 = ld4(w + 4);
            z0.x += w0.x; z0.y += w0.y; z0.z += w0.z; z0.w += w0.w;
            z1.x += w1.x; z1.y += w1.y; z1.z += w1.z; z1.w += w1.w;
        }
        if constexpr (XTRA) {  // the bond's dense tail: columns Fb - db .. Fb - 1, the pair's xb row
            const float *x = xs + BLK_ATOMS * h_da + (lb >> 1) * h_db;
            for (int j = 0; j < h_db; ++j) {
                const float *w = wt + (h_Fb - h_db + j) * BN + c;
                fma4(z0, x[j], ld4(w));
                fma4(z1, x[j], ld4(w + 4));
            }
        }
        const float4 b0 = ld4(bb + c), b1 = ld4(bb + c + 4);
        z0.x += b0.x; z0.y += b0.y; z0.z += b0.z; z0.w += b0.w;
        z1.x += b1.x; z1.y += b1.y; z1.z += b1.z; z1.w += b1.w;
        float *zr = P.inp + (size_t)b * h_Hk + n0 + c;
        st4(zr, z0);
        st4(zr + 4, z1);
        float zz[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            zz[q] = act_fwd(ACT, zz[q], slope);
            mx = max(mx, absbits(zz[q]));
        }
        if constexpr (PAIRS) {
            ym[u][0] = make_float4(zz[0], zz[1], zz[2], zz[3]);
            ym[u][1] = make_float4(zz[4], zz[5], zz[6], zz[7]);
        }
    }
    if (blk == 0 && tid < C4) st4(P.inp + n0 + 4 * tid, f4zero());  // pad row 0 (Z_0 of the backward)
    wd_estamp(5);
    __shared__ uint32_t red[NT / 64];
    if constexpr (PAIRS) {
        // M_0 = act(inp) as fp16 pairs scaled by this tile's max (rows up to the end of the last 16-row group
        // the layer multiplies: zeros past the block)
        const float s = h2_scale(publish_max_all(mx, P.amax + (size_t)blk * h_nt + nt, red));
        wd_estamp(6);
        constexpr int CH = 2 * BLK_BONDS * 64;
        const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
            P.m0 + (size_t)blk * (h_Hk >> 5) * CH, 0, (h_Hk >> 5) * CH, 0x00020000);
#pragma unroll
        for (int u = 0; u < BU; ++u) {
            const int v = tid + NT * u, lb = v / U8, c = 8 * (v % U8);
            if (lb >= ((B.bn + 15) & ~15)) break;
            h2_store8(prs, h2_blk_off<BLK_BONDS>(lb, n0 + c), BLK_BONDS * 64, ym[u][0], ym[u][1], s);
        }
        wd_estamp(7);
    } else {
        publish_max(mx, P.amax + (size_t)blk * h_nt + nt, red);
    }
}

constexpr int WO_MAXK = 160;  // f_atoms / f_bonds columns embed_kernel stages (Fa, Fb <= 160)

struct WoReadoutP {
    // The entry head: what the pair kernel reads before its main loop -- the operands, the block row, the scale
    // words, then what the row's prefetch loads from -- adjacent and first, copied by value at the entry with one
    // batch of scalar loads (wo_readout_kernel; 28 dwords).  The rest is first touched in the epilogue.
    const uint8_t *apairs;                   // (the template's PAIRS, below)
    const uint8_t *woh;
    const int32_t *blocks;
    const uint32_t *a_amax, *wo_amax;
    int kp;                                  // Hk (the A operand's row length)
    int n_tiles;
    uint32_t tmagic;                         // tile_magic(n_tiles) (common.hpp)
    int a_nw, a_g;
    int ldeo;
    const float *bias;                       // b_o (padded)
    const float *w_atoms; const int32_t *mol_start, *mol_size; const float *xn;
    const float *eo;                         // (kca = 0, below)
    const uint8_t *fa; int kpa; int kca;     // f_atoms: blocked atom plane tiles [nblk * 64][kpa], kca chunks used
    int kcw;                                 // f_atoms chunks in the W_o plane tiles (Fak / 32; kca = 0 or kcw)
    const uint8_t *ag;                       // A: blocked atom plane tiles [nblk * 64][kp = Hk]
    const uint8_t *wo;                       // W_o plane tiles [Hk][Fak + Hk] with BN-row blocks
    int agg; float norm; const float *zero_vec;
    int act; const float *slope; float p_drop; uint64_t seed; uint32_t layer;
    float *out; int ncols;                   // out [B][ncols] (ncols = H)
    // kca = 0: the f_atoms half of [f_atoms | A] W_o^T, precomputed per atom (by embed_kernel as sums of
    // W_o columns, or by the atom-message input GEMM): fp32 natural atom rows, row stride ldeo (null: GEMM
    // segment): eo, ldeo in the entry head
    int Hk;
    float *zosave;  // training forward or null: the W_o pre-activation (mpn.py:133) as fp32 natural atom rows [Vap][Hk]
    // the template's PAIRS (round 6): A as fp16 pair tiles of the blocks' atom rows ([nblk][Hk / 32][2][64][64 B],
    // written by the last layer) with its words [nblk][a_nw] (groups of a_g columns), and W_o[:, Fa:] as fp16
    // pair tiles with BN-row blocks scaled by the word wo_amax (wdmpnn_pack_params)
    // (apairs, a_amax, a_nw, a_g, woh, wo_amax: in the entry head)
};

template <int BN> struct WoWaves;
template <> struct WoWaves<64> { static constexpr int WM = 4, WN = 2; };
template <> struct WoWaves<80> { static constexpr int WM = 2, WN = 5; };

// grid = nblk * n_tiles: 64 atom rows x BN columns per workgroup.  CPS: K chunks per LDS stage (one
// barrier per CPS chunks; two stages).  80-column tiles: CPS 2 (W_o's 64-row chunks are short: one barrier
// per chunk cost 0.6 us alone on the chip, 12.5 vs 13.1 us) for launches of several batches, where
// workgroups queue per CU; CPS 1 (55 KB of LDS) for one batch, whose 256 workgroups then co-reside
// with the layer kernels of batches in flight on other streams (+5 % with two streams, same-box A/B,
// profiles/round3_*).  64-column tiles: CPS 1.
// PAIRS (round 6): the GEMM on fp16 pair tiles of A and W_o (gemm_x6.hpp h2_mainloop_pairs: 4 MFMA waves of
// 16 atom rows, 4 waves copying A; three products per fp32 product instead of the planes' six), 512 threads.
template <int BN, int CPS, int NJ = WD_MULTI, bool PAIRS = false>
// (PAIRS: <= 128 VGPRs, two workgroups per CU beside other streams' layers)
__global__ __launch_bounds__(PAIRS ? 512 : 64 * WoWaves<BN>::WM * WoWaves<BN>::WN, PAIRS ? 4 : 1) void wo_readout_kernel(const Multi<WoReadoutP, NJ> MP) {
    // (PAIRS: WM x WN = 4 x 1 MFMA waves, and four more copying A: NT = 512)
    constexpr int BM = BLK_ATOMS, LDC = BN + 4, WM = PAIRS ? 4 : WoWaves<BN>::WM, WN = PAIRS ? 1 : WoWaves<BN>::WN;
    constexpr int NT = PAIRS ? 512 : 64 * WM * WN;
    // (two LDS stages; deeper single-chunk pipelines measured slower: three / four stages 15.1 / 14.8 us here,
    // 12.8 / 11.8 against 9.7 us on QM9-shaped batches)
    constexpr int EPI_BYTES = (BM * LDC + BM + 3 * BLK_MOLS + BN) * 4;  // (+ the bias columns: PAIRS)
    constexpr int LDS_BYTES = PAIRS ? (h2p_lds_bytes<BM, BN>() > EPI_BYTES ? h2p_lds_bytes<BM, BN>() : EPI_BYTES)
                                    : 2 * CPS * x6_stage_bytes<BM, BN>();
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    int tile;
    const WoReadoutP &P = multi_pick(MP, xcd_tile(blockIdx.x, gridDim.x), tile);
    // the entry head by value (PAIRS: pinned in scalar registers, all of it; as mp_layer_kernel)
    auto hv = [](auto v) {
        if constexpr (PAIRS) return pin_s(v);
        else return v;
    };
    const int h_nt = hv(P.n_tiles), h_kp = hv(P.kp), h_ldeo = hv(P.ldeo);
    const uint32_t h_tm = hv(P.tmagic);
    const int32_t *h_blocks = hv(P.blocks);
    const float *h_bias = hv(P.bias), *h_w_atoms = hv(P.w_atoms), *h_xn = hv(P.xn), *h_eo = hv(P.eo);
    const int32_t *h_mol_start = hv(P.mol_start), *h_mol_size = hv(P.mol_size);
    const uint8_t *h_apairs = nullptr, *h_woh = nullptr;
    const uint32_t *h_a_amax = nullptr, *h_wo_amax = nullptr;
    int h_a_nw = 0, h_a_g = 0;
    if constexpr (PAIRS) {
        h_apairs = pin_s(P.apairs); h_woh = pin_s(P.woh); h_a_amax = pin_s(P.a_amax); h_wo_amax = pin_s(P.wo_amax);
        h_a_nw = pin_s(P.a_nw); h_a_g = pin_s(P.a_g);
    }
    int blk, nt;
    tile_split(tile, h_nt, h_tm, blk, nt);
    const int n0 = nt * BN;
    // (PAIRS: a scalar load issued here, waited for by each role where it needs the row: mp_layer_kernel)
    BlockRow B = PAIRS ? load_block_atoms_s(h_blocks, blk) : load_block(h_blocks, blk);
    const int tid = threadIdx.x;
    X6Operands O{};
    O.a0 = P.fa; O.nkc0 = P.kpa >> 5; O.kc0 = P.kca;
    O.a1 = P.ag; O.nkc1 = P.kp >> 5; O.kc1 = P.kp >> 5;
    O.rb = blk;
    O.a_rows = B.an;
    // W_o planes: per BN-row block, kcw f_atoms chunks then kp / 32 A chunks; the f_atoms chunks are
    // skipped when the codes path adds that half in the epilogue (kca = 0)
    O.b = P.wo + ((size_t)nt * (P.kcw + (P.kp >> 5)) + (P.kcw - P.kca)) * (3 * BN * 64);
    // prefetched during the GEMM (mainloop hook): this thread's bias columns, the block's atom weights
    // (thread a < an: w_atoms[as + a]) and its molecules' scope / Xn (thread i < nm)
    constexpr int C4 = BN / 4;
    static_assert((PAIRS || NT % C4 == 0) && BM <= NT, "one bias group per thread, one atom weight per thread");
    int nm = PAIRS ? 0 : min(B.mh - B.ml, BLK_MOLS);  // (the packer never exceeds BLK_MOLS; PAIRS: in rows() below)
    // (PAIRS: the pad row's store follows the main loop -- zosave is no entry field)
    if (!PAIRS && P.zosave && blk == 0 && tid < BN / 4) st4(P.zosave + n0 + 4 * tid, f4zero());  // pad atom row 0
    float4 bb = f4zero();
    float watom = 0.f, mxn = 0.f;
    int mstart = 0, msize = 0;
    // codes path: this thread's rows of the precomputed f_atoms W_o[:, :Fa]^T (the epilogue units below)
    constexpr int EPU = (BM * C4 + NT - 1) / NT;
    float4 eo[EPU];
    auto prefetch = [&](int phase) {
        if (phase != 0) return;
        if (!PAIRS || tid < C4) bb = ld4(h_bias + n0 + 4 * (tid % C4));  // (PAIRS: staged through LDS below)
        if (tid < B.an) watom = h_w_atoms[B.as + tid];
#pragma unroll
        for (int j = 0; j < EPU; ++j) {
            const int v = tid + NT * j, la = v / C4, c = 4 * (v % C4);
            eo[j] = h_eo && v < BM * C4 && la < B.an ? ld4(h_eo + (size_t)(B.as + la) * h_ldeo + n0 + c) : f4zero();
        }
        if (tid < nm) {
            mstart = h_mol_start[B.ml + tid];
            msize = h_mol_size[B.ml + tid];
            mxn = h_xn[B.ml + tid];
        }
    };
    float *H = reinterpret_cast<float *>(lds);
    floatx4 acc[BM / WM / 16][BN / WN / 16];
    if constexpr (PAIRS) {
        // the block row and the prefetch that needs it (registers across the GEMM: 16 rows per MFMA wave leave
        // room), per role
        auto rows = [&]() {
            nm = min(B.mh - B.ml, BLK_MOLS);
            prefetch(0);
            return B.an;
        };
        uint32_t wom = 0;  // (W_o's word: loaded by the consumers before their loop, not after it)
        auto words = [&]() {
            wom = *h_wo_amax;
            return lane_word(h_a_amax + (size_t)blk * h_a_nw, h_a_nw);
        };
        int se;
        h2_mainloop_pairs<BM, BN>(h_apairs + (size_t)blk * (h_kp >> 5) * (2 * BM * 64),
                                  h_woh + (size_t)nt * (h_kp >> 5) * (2 * BN * 64), h_kp >> 5, rows, words, h_a_g, lds,
                                  acc, se);
        if (P.zosave && blk == 0 && tid < BN / 4) st4(P.zosave + n0 + 4 * tid, f4zero());  // pad atom row 0
        __syncthreads();
        if (threadIdx.x < 256)
            x6_acc_to_lds<BM, BN, 4, 1, true>(acc, H, se >= 0 ? __uint_as_float((uint32_t)(254 - se) << 23) : 1.f,
                                              h2_inv_scale(wom));
    } else {
        x6_mainloop<BM, BN, WM, WN, CPS>(O, lds, acc, prefetch);
        __syncthreads();
        x6_acc_to_lds<BM, BN, WM, WN>(acc, H);
    }
    float *Wl = H + BM * LDC;           // [BM] atom weights of the block
    float *Ml = Wl + BM;                // [3][BLK_MOLS] per molecule: start (as float bits), size, Xn
    static_assert(EPI_BYTES <= LDS_BYTES, "readout staging fits");
    static_assert(BLK_MOLS <= NT, "one molecule per thread in the prefetch");
    if (tid < BM) Wl[tid] = watom;
    if (PAIRS && tid < C4) st4(Ml + 3 * BLK_MOLS + 4 * tid, bb);
    if (tid < nm) {
        Ml[tid] = __int_as_float(mstart);
        Ml[BLK_MOLS + tid] = __int_as_float(msize);
        Ml[2 * BLK_MOLS + tid] = mxn;
    }
    __syncthreads();
    // h = act(. + b_o) (* dropout), in place (mpn.py:133-134)
    with_act(P.act, [&](auto act_c) {
        constexpr int ACT = decltype(act_c)::value;
        const float slope = ACT == ACT_PRELU ? P.slope[0] : 0.f;
#pragma unroll
        for (int j = 0; j < EPU; ++j) {
            const int v = tid + NT * j;
            if (v >= BM * C4) break;
            const int la = v / C4, c = 4 * (v % C4);
            float4 hv = ld4(H + la * LDC + c);
            hv.x += eo[j].x; hv.y += eo[j].y; hv.z += eo[j].z; hv.w += eo[j].w;  // (0 without codes)
            // (PAIRS, 512 threads: NT % C4 != 0, each unit its own bias columns, from LDS)
            const float4 b4 = PAIRS ? ld4(Ml + 3 * BLK_MOLS + c) : bb;
            float z[4] = {hv.x + b4.x, hv.y + b4.y, hv.z + b4.z, hv.w + b4.w};
            if (P.zosave && la < B.an) st4(P.zosave + (size_t)(B.as + la) * P.Hk + n0 + c, make_float4(z[0], z[1], z[2], z[3]));
#pragma unroll
            for (int q = 0; q < 4; ++q) z[q] = act_fwd(ACT, z[q], slope);
            if (P.p_drop > 0.f && la < B.an)
#pragma unroll
                for (int q = 0; q < 4; ++q) z[q] *= dropout_scale(P.seed, P.layer, B.as + la, n0 + c + q, P.p_drop);
            st4(H + la * LDC + c, make_float4(z[0], z[1], z[2], z[3]));
        }
    });
    __syncthreads();
    // readout (mpn.py:145-171) of this block's molecules, columns n0 .. n0 + BN - 1: eight lanes per
    // (molecule, column), lane j summing the molecule's atoms j, j + 8, ... from LDS, then a fixed xor
    // butterfly over the eight lanes (deterministic; every lane ends with the same sum)
    constexpr int RP = 8;
    static_assert(NT % RP == 0 && 64 % RP == 0, "lane groups stay inside a wave");
    for (int t = tid; t < nm * BN * RP; t += NT) {
        const int part = t % RP, u = t / RP, im = u / BN, i = B.ml + im, cc = u % BN, col = n0 + cc;
        const int n = __float_as_int(Ml[BLK_MOLS + im]);
        float s = 0.f, wsum = 0.f;
        const int a0 = __float_as_int(Ml[im]) - B.as;
        for (int a = part; a < n; a += RP) {
            const float w = Wl[a0 + a];
            s = fmaf(w, H[(a0 + a) * LDC + cc], s);
            wsum += w;
        }
#pragma unroll
        for (int off = 1; off < RP; off <<= 1) {
            s += __shfl_xor(s, off, 64);
            wsum += __shfl_xor(wsum, off, 64);
        }
        if (part != 0 || col >= P.ncols) continue;
        float v;
        if (n == 0) {
            v = P.zero_vec[col];  // cached_zero_vector, no Xn factor (mpn.py:148-149)
        } else {
            const float m = P.agg == 0 ? s / wsum : (P.agg == 2 ? s / P.norm : s);
            v = Ml[2 * BLK_MOLS + im] * m;
        }
        P.out[(size_t)i * P.ncols + col] = v;
    }
}

}  // namespace wd
