// graph_build.hpp — the whole device graph (WdGraph) of a compact batch, built on the GPU in one launch
// (format: include/wdmpnn.h "Compact graphs").
//
// One workgroup per molecule block (<= 128 directed bonds, <= 64 atoms, <= 64 molecules: every index of
// the block is block-local, so the in-lists are built in LDS) plus one workgroup for the pad rows.
// It reproduces, value for value and entry for entry, what the host path builds:
//   * feature rows: f_atoms[a] = one-hot columns from the atom code + the last column's value
//     (featurization.py:190-211), f_bonds[b] = f_atoms[src(b)] ‖ bond columns (featurization.py:467-468,
//     545-546, 616-617), fp32 with 16-byte aligned rows, and their bf16x3 plane tiles (planes.hpp);
//     with extra features (WdCompact.atom_extra / bond_extra, featurization.py:436-440, 460-468) the rows are
//     f_atoms[a] = base ‖ atom_extra[a] and f_bonds[b] = f_atoms[src(b)] ‖ bond bits ‖ bond_extra[pair(b)]:
//     natural rows (BR 64) and, for atoms, the molecule-blocked layout of the fused W_o;
//   * in(a) = the bonds into a in creation order (= a2b[a], featurization.py:471-476, 624-627);
//   * msg_gather row b (mpn.py:112-120): j in in(src(b)), coefficient w_j - [j == rev(b)] (w - 1 is a
//     single fp32 rounding, as the host's double-then-float), zero coefficients dropped;
//     atom_gather row a (mpn.py:126-131): j in in(a), coefficient w_j != 0;
//     their transposes (the backward's gathers): msg_gather_t row j = the rows b with src(b) = dst(j) in
//     increasing b, atom_gather_t row j = (dst(j), w_j);
//   * the ELL-8 rows, the block maps, b2revb, w_atoms and the molecule scope arrays.
// A lean graph (WDMPNN_GRAPH_LEAN) gets only what the fused inference forward reads: the atom gather
// (CSR + ELL), the block maps, b2revb, the bonds' source atoms and tails, the scope arrays.
// Pair structure: bond ids 1 + 2p and 2 + 2p are pair p's b1 = a1 -> a2 and b2 = a2 -> a1 (pad bond 0),
// so every molecule's first bond id is odd and a block-local bond index lb has rev(lb) = lb ^ 1.
#pragma once
#include "planes.hpp"
#include "wdmpnn.h"

namespace wd {

constexpr int GB_BONDS = 128, GB_ATOMS = 64, GB_MOLS = 64, GB_ELLW = 8, GB_CSR_PAD = 8;
// workgroups per block for a full (non-lean) build: slice 0 builds the block's structure (in-lists, CSR,
// ELL, maps) and every slice writes a quarter of its feature rows and planes -- with one workgroup per
// block a B = 64 batch (65 workgroups) wrote its ~30 MB from a quarter of the CUs (48 us, 0.08 of HBM)
constexpr int GB_SLICES = 4;

struct GraphBuildP {
    WdCompact c;
    int Fa, Fb, lda, ldb, Vap, Rbp;
    float *f_atoms, *f_bonds;
    uint8_t *fa_x6, *fb_x6, *fa_blk_x6;
    float *w_atoms, *xn;
    int32_t *mol_start, *mol_size, *b2revb, *blocks, *bond_blk_row, *atom_blk_row;
    uint8_t *bond_src_blk;
    uint16_t *bond_tail;
    uint8_t *msg_ell_idx, *agg_ell_idx;
    float *msg_ell_coef, *agg_ell_coef;
    int32_t *msg_ptr, *msg_idx, *agg_ptr, *agg_idx, *msgt_ptr, *msgt_idx, *aggt_ptr, *aggt_idx;
    float *msg_coef, *agg_coef, *msgt_coef, *aggt_coef;
    int lean;    // 1: no dense feature rows / planes and no transposed gathers (inference-only graph)
    int planes;  // 0: no plane tiles of the feature rows (WDMPNN_GRAPH_NO_PLANES)
};

// value of f_atoms column c for an atom code (c < Fa: the base block's width, the mass in its last column)
__device__ __forceinline__ float code_value(const WdAtomCode &a, int c, int Fa) {
    if (c == Fa - 1) return a.last;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) hit |= a.col[k] == c;
    return hit ? 1.f : 0.f;
}

// 8 consecutive columns c0 .. c0 + 7 of a natural fp32 row + its plane tiles (BR 64; planes null: none)
__device__ __forceinline__ void put_row8(float *row_f32, uint8_t *planes, int ld, int r, int c0, const float (&v)[8]) {
    const float4 lo = make_float4(v[0], v[1], v[2], v[3]), hi = make_float4(v[4], v[5], v[6], v[7]);
    st4(row_f32 + c0, lo);
    st4(row_f32 + c0 + 4, hi);
    if (planes) x6_store8<64>(planes, ld, r, c0, lo, hi);
}

// in(a) / out(a) in creation order by counting sort: a bond's slot = start of its atom + the number of
// earlier bonds with the same endpoint (16-byte broadcast reads of the endpoint arrays: no serial
// loops over the block's bonds); every pair gives each endpoint one in- and one out-bond, so
// |in(a)| = |out(a)| = deg(a).  in(a) = s_in[s_start[a] .. s_start[a + 1]), out(a) likewise in s_out; returns
// the slot of bond tid in s_in (threads tid < bn; -1 otherwise).  Every thread of the workgroup calls this.
__device__ __forceinline__ int build_in_out(int bn, int an, const uint8_t *s_src, const uint8_t *s_dst, uint8_t *s_in,
                                            uint8_t *s_out, int *s_start) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto count_eq = [](const uint8_t *arr, int v, int below) {
        int n = 0;
        for (int q = 0; q < GB_BONDS / 16 && 16 * q < below; ++q) {
            const uint4 w = *reinterpret_cast<const uint4 *>(arr + 16 * q);
            const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int u = 0; u < 16; ++u)
                n += ((wd[u >> 2] >> (8 * (u & 3))) & 0xFF) == (uint32_t)v && 16 * q + u < below;
        }
        return n;
    };
    if (wave == 0) {  // deg + exclusive prefix over the atoms (one wave)
        const int d = lane < an ? count_eq(s_dst, lane, bn) : 0;
        int incl = d;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane < an) s_start[lane] = incl - d;
        if (lane == 63) s_start[an] = incl;  // (an <= 64: lanes >= an add 0)
    }
    __syncthreads();
    int slot = -1;
    if (tid < bn) {
        slot = s_start[s_dst[tid]] + count_eq(s_dst, s_dst[tid], tid);
        s_in[slot] = (uint8_t)tid;
        s_out[s_start[s_src[tid]] + count_eq(s_src, s_src[tid], tid)] = (uint8_t)tid;
    }
    __syncthreads();
    return slot;
}

// the block's in-lists, gather CSRs (+ transposes) and ELL rows (slice 0 of a block's workgroups; the
// endpoint arrays are in LDS, every thread of the workgroup calls this)
__device__ __forceinline__ void build_structure(const GraphBuildP &P, int k, int bs, int bn, int as, int an,
                                                const uint8_t *s_src, const uint8_t *s_dst, uint8_t *s_in,
                                                uint8_t *s_out, const float *s_w, int *s_start, int *s_pm, int *s_pt,
                                                int *s_pg, int *s_pa, const int *s_off) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    (void)k;
    build_in_out(bn, an, s_src, s_dst, s_in, s_out, s_start);
    // entry counts: msg row, msg_t row, agg_t row (bonds); agg row (atoms)
    if (tid < bn) {
        const int s = s_src[tid], rev = tid ^ 1;
        int cm = 0;
        for (int e = s_start[s]; e < s_start[s + 1]; ++e) {
            const int j = s_in[e];
            cm += (j == rev ? s_w[j] - 1.0f : s_w[j]) != 0.f;
        }
        // msg_t row: the rows lb in out(dst(tid)); every one has coefficient w - [lb == rev(tid)], and
        // rev(tid) is among them (src(rev) = dst(tid))
        const int nout = s_start[s_dst[tid] + 1] - s_start[s_dst[tid]];
        s_pm[tid + 1] = cm;
        s_pt[tid + 1] = (nout - 1) * (s_w[tid] != 0.f) + (s_w[tid] - 1.0f != 0.f);
        s_pg[tid + 1] = s_w[tid] != 0.f;
    }
    if (tid < an) {
        int ca = 0;
        for (int e = s_start[tid]; e < s_start[tid + 1]; ++e) ca += s_w[s_in[e]] != 0.f;
        s_pa[tid + 1] = ca;
    }
    __syncthreads();
    if (wave < 4) {  // four exclusive prefix sums, one wave each (two elements per lane)
        int *pre = wave == 0 ? s_pm : wave == 1 ? s_pt : wave == 2 ? s_pg : s_pa;
        const int n = wave == 3 ? an : bn;
        const int e0 = 2 * lane + 1, e1 = 2 * lane + 2;
        const int a = e0 <= n ? pre[e0] : 0, c = e1 <= n ? pre[e1] : 0;
        int incl = a + c;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        const int base = incl - a - c;
        if (e0 <= n) pre[e0] = base + a;
        if (e1 <= n) pre[e1] = base + a + c;
        if (lane == 0) pre[0] = 0;
    }
    __syncthreads();
    const int om = s_off[0], oa = s_off[1];
    if (tid < bn && !P.lean) {  // (a lean graph serves only the fused forward, which gathers by src / rev)
        const int b = bs + tid, s = s_src[tid], rev = tid ^ 1;
        // msg_gather row b + its ELL-8 row
        int o = om + s_pm[tid], n = 0;
        uint8_t eidx[GB_ELLW];
        float ecoef[GB_ELLW];
#pragma unroll
        for (int q = 0; q < GB_ELLW; ++q) { eidx[q] = 0; ecoef[q] = 0.f; }
        for (int e = s_start[s]; e < s_start[s + 1]; ++e) {
            const int j = s_in[e];
            const float c = j == rev ? s_w[j] - 1.0f : s_w[j];
            if (c == 0.f) continue;
            P.msg_idx[o] = bs + j;
            P.msg_coef[o] = c;
            ++o;
            if (n < GB_ELLW) { eidx[n] = (uint8_t)j; ecoef[n] = c; }
            ++n;
        }
        P.msg_ptr[b + 1] = om + s_pm[tid + 1];
        if (n > GB_ELLW) eidx[GB_ELLW - 1] |= 0x80;
#pragma unroll
        for (int q = 0; q < GB_ELLW; ++q) {
            P.msg_ell_idx[(size_t)GB_ELLW * b + q] = eidx[q];
            P.msg_ell_coef[(size_t)GB_ELLW * b + q] = ecoef[q];
        }
        {
            // msg_gather_t row b: the rows lb in out(dst(b)), increasing lb
            o = om + s_pt[tid];
            const int d = s_dst[tid];
            for (int e = s_start[d]; e < s_start[d + 1]; ++e) {
                const int lb = s_out[e];
                const float c = tid == (lb ^ 1) ? s_w[tid] - 1.0f : s_w[tid];
                if (c == 0.f) continue;
                P.msgt_idx[o] = bs + lb;
                P.msgt_coef[o] = c;
                ++o;
            }
            P.msgt_ptr[b + 1] = om + s_pt[tid + 1];
            // atom_gather_t row b: (dst(b), w_b)
            if (s_w[tid] != 0.f) {
                P.aggt_idx[oa + s_pg[tid]] = as + s_dst[tid];
                P.aggt_coef[oa + s_pg[tid]] = s_w[tid];
            }
            P.aggt_ptr[b + 1] = oa + s_pg[tid + 1];
        }
    }
    if (tid < an) {  // atom_gather row a + its ELL-8 row
        const int a = as + tid;
        int o = oa + s_pa[tid], n = 0;
        uint8_t eidx[GB_ELLW];
        float ecoef[GB_ELLW];
#pragma unroll
        for (int q = 0; q < GB_ELLW; ++q) { eidx[q] = 0; ecoef[q] = 0.f; }
        for (int e = s_start[tid]; e < s_start[tid + 1]; ++e) {
            const int j = s_in[e];
            if (s_w[j] == 0.f) continue;
            P.agg_idx[o] = bs + j;
            P.agg_coef[o] = s_w[j];
            ++o;
            if (n < GB_ELLW) { eidx[n] = (uint8_t)j; ecoef[n] = s_w[j]; }
            ++n;
        }
        P.agg_ptr[a + 1] = oa + s_pa[tid + 1];
        if (n > GB_ELLW) eidx[GB_ELLW - 1] |= 0x80;
#pragma unroll
        for (int q = 0; q < GB_ELLW; ++q) {
            P.agg_ell_idx[(size_t)GB_ELLW * a + q] = eidx[q];
            P.agg_ell_coef[(size_t)GB_ELLW * a + q] = ecoef[q];
        }
    }
}

// LDS image of one molecule block: its row of the block table, its molecules' first atoms / bonds, its atoms'
// codes, its bonds' block-local endpoints, weights and tails, and the in- / out-lists (build_in_out)
struct GbBlock {
    int blk[8];
    int mas[GB_MOLS], mbs[GB_MOLS];
    WdAtomCode code[GB_ATOMS];
    __attribute__((aligned(16))) uint8_t src[GB_BONDS], dst[GB_BONDS];
    uint8_t in[GB_BONDS], out[GB_BONDS];
    uint16_t tail[GB_BONDS];
    float w[GB_BONDS];
    int start[GB_ATOMS + 1];  // in(a) = in[start[a] ..), out(a) = out[start[a] ..)
};

// loads block k into S and (head: the slice that writes the block's structure) writes the scope arrays, w_atoms,
// b2revb and the block maps; BOND_MAPS: also bond_src_blk / bond_tail (bond-message graphs).  false: a block
// past the capacities, which the host plan never makes (the workgroup returns).  Every thread calls this.
template <bool BOND_MAPS, typename Params>
__device__ __forceinline__ bool load_block(const Params &P, GbBlock &S, int k, bool head) {
    const WdCompact &C = P.c;
    const int tid = threadIdx.x;
    if (tid < 8) S.blk[tid] = C.blocks[8 * k + tid];
    __syncthreads();
    const int bs = S.blk[0], bn = S.blk[1], as = S.blk[2], an = S.blk[3], ml = S.blk[4], nm = S.blk[5] - S.blk[4];
    if (bn > GB_BONDS || an > GB_ATOMS || nm > GB_MOLS || nm < 0 || bn < 0 || an < 0) return false;
    if (tid < nm) {
        S.mas[tid] = C.mols[4 * (ml + tid)];
        S.mbs[tid] = C.mols[4 * (ml + tid) + 2];
        if (head) {
            P.mol_start[ml + tid] = C.mols[4 * (ml + tid)];
            P.mol_size[ml + tid] = C.mols[4 * (ml + tid) + 1];
            P.xn[ml + tid] = C.xn[ml + tid];
        }
    }
    if (tid < an) {
        S.code[tid] = C.atoms[as + tid];
        if (head) {
            P.w_atoms[as + tid] = S.code[tid].w;
            P.atom_blk_row[as + tid] = GB_ATOMS * k + tid;
        }
    }
    if (tid < 8 && head) P.blocks[8 * k + tid] = S.blk[tid];
    if (tid >= bn && tid < GB_BONDS) S.src[tid] = S.dst[tid] = 0xFF;  // never equal to an atom of the block
    __syncthreads();
    if (tid < bn) {  // endpoints of bond b = bs + tid
        const int b = bs + tid;
        int lo = 0, hi = nm - 1;  // the molecule: last one whose first bond is <= b
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (S.mbs[mid] <= b) lo = mid; else hi = mid - 1;
        }
        const int p = (b - 1) >> 1, dir = (b - 1) & 1;
        const WdBondPair q = C.pairs[p];
        const int l1 = S.mas[lo] + q.a1 - as, l2 = S.mas[lo] + q.a2 - as;
        S.src[tid] = (uint8_t)(dir ? l2 : l1);
        S.dst[tid] = (uint8_t)(dir ? l1 : l2);
        S.w[tid] = dir ? q.w21 : q.w12;
        S.tail[tid] = q.tail;
        if (head) {
            P.b2revb[b] = dir ? b - 1 : b + 1;
            P.bond_blk_row[b] = GB_BONDS * k + tid;
            if constexpr (BOND_MAPS) {
                P.bond_src_blk[b] = (uint8_t)(dir ? l2 : l1);
                P.bond_tail[b] = q.tail;
            }
        }
    }
    __syncthreads();
    return true;
}

// the block's f_atoms rows (base columns from the codes ‖ atom extras) with their natural plane tiles, and its
// rows of the molecule-blocked layout (zero past an): 8 columns per thread-step, slice sl of nsl
template <typename Params>
__device__ __forceinline__ void write_atom_rows(const Params &P, const GbBlock &S, int k, int sl, int nsl) {
    const WdCompact &C = P.c;
    const int as = S.blk[2], an = S.blk[3], Fa = P.Fa, UA = P.lda / 8, da = C.atom_extra_dim, Fa0 = Fa - da;
    for (int u = threadIdx.x + 256 * sl; u < GB_ATOMS * UA; u += 256 * nsl) {
        const int la = u / UA, c0 = (u % UA) * 8;
        float v[8];
        if (la < an) {
            const WdAtomCode &cd = S.code[la];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = c0 + q;
                v[q] = c < Fa0 ? code_value(cd, c, Fa0) : (c < Fa ? C.atom_extra[(size_t)(as + la) * da + (c - Fa0)] : 0.f);
            }
            put_row8(P.f_atoms + (size_t)(as + la) * P.lda, P.fa_x6, P.lda, as + la, c0, v);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = 0.f;
        }
        if (P.fa_blk_x6)
            x6_store8<64>(P.fa_blk_x6, P.lda, GB_ATOMS * k + la, c0, make_float4(v[0], v[1], v[2], v[3]),
                          make_float4(v[4], v[5], v[6], v[7]));
    }
}

// zero feature rows outside the batch: row 0 and rows n .. n_padded - 1 (fp32 rows, null: none; plane tiles,
// null: none)
__device__ __forceinline__ void zero_pad_rows(float *rows_f32, uint8_t *planes, int ld, int n, int n_padded) {
    const int U = ld / 8;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int u = threadIdx.x; u < (1 + n_padded - n) * U; u += 256) {
        const int i = u / U, r = i == 0 ? 0 : n + i - 1, c0 = (u % U) * 8;
        if (rows_f32) {
            st4(rows_f32 + (size_t)r * ld + c0, z);
            st4(rows_f32 + (size_t)r * ld + c0 + 4, z);
        }
        if (planes) x6_store8<64>(planes, ld, r, c0, z, z);
    }
}

// grid: per batch its n_blocks + 1 workgroups (Multi: up to WD_MULTI batches per launch) x gridDim.y
// slices (GB_SLICES for full builds, 1 for lean ones)
__global__ __launch_bounds__(256) void graph_build_kernel(const Multi<GraphBuildP> MP) {
    int k;
    const GraphBuildP &P = multi_pick(MP, (int)blockIdx.x, k);
    const int tid = threadIdx.x, sl = blockIdx.y, nsl = gridDim.y;
    const WdCompact &C = P.c;
    const int Fa = P.Fa, Fb = P.Fb, UB = P.ldb / 8;
    // extra features: columns [Fa0, Fa) of an atom row, [Fx, Fb) of a bond row (none: Fa0 = Fa, Fx = Fb)
    const int da = C.atom_extra_dim, db = C.bond_extra_dim, Fa0 = Fa - da, Fx = Fb - db;
    if (k == C.n_blocks && sl != 0) return;
    if (k == C.n_blocks) {  // pad rows: atom / bond row 0, the rows up to the padded extents, CSR heads and tails
        const int V1 = C.n_atoms, E1 = C.n_bonds;
        const int na_pad = 1 + (P.Vap - V1), nb_pad = 1 + (P.Rbp - E1);
        if (!P.lean) {
            zero_pad_rows(P.f_atoms, P.fa_x6, P.lda, V1, P.Vap);
            zero_pad_rows(P.f_bonds, P.fb_x6, P.ldb, E1, P.Rbp);
        }
        for (int i = tid; i < na_pad; i += 256) {
            const int r = i == 0 ? 0 : V1 + i - 1;
            P.atom_blk_row[r] = -1;
            for (int s = 0; s < GB_ELLW; ++s) { P.agg_ell_idx[GB_ELLW * r + s] = 0; P.agg_ell_coef[GB_ELLW * r + s] = 0.f; }
        }
        for (int i = tid; i < nb_pad; i += 256) {
            const int r = i == 0 ? 0 : E1 + i - 1;
            P.bond_blk_row[r] = -1;
            P.bond_src_blk[r] = 0;
            P.bond_tail[r] = 0;
            if (!P.lean)
                for (int s = 0; s < GB_ELLW; ++s) { P.msg_ell_idx[GB_ELLW * r + s] = 0; P.msg_ell_coef[GB_ELLW * r + s] = 0.f; }
        }
        if (tid < 2) {  // row 0 (pad atom / bond) has no entries
            P.agg_ptr[tid] = 0;
            if (!P.lean) { P.msg_ptr[tid] = 0; P.msgt_ptr[tid] = 0; P.aggt_ptr[tid] = 0; }
        }
        if (tid == 0) { P.w_atoms[0] = 0.f; P.b2revb[0] = 0; }
        if (tid < GB_CSR_PAD) {  // readable dummy entries past the end (WdCsr)
            P.agg_idx[C.nnz_agg + tid] = 0; P.agg_coef[C.nnz_agg + tid] = 0.f;
            if (!P.lean) {
                P.msg_idx[C.nnz_msg + tid] = 0; P.msg_coef[C.nnz_msg + tid] = 0.f;
                P.msgt_idx[C.nnz_msg + tid] = 0; P.msgt_coef[C.nnz_msg + tid] = 0.f;
                P.aggt_idx[C.nnz_agg + tid] = 0; P.aggt_coef[C.nnz_agg + tid] = 0.f;
            }
        }
        return;
    }

    __shared__ GbBlock S;
    __shared__ int s_pm[GB_BONDS + 1], s_pt[GB_BONDS + 1], s_pg[GB_BONDS + 1], s_pa[GB_ATOMS + 1];
    __shared__ int s_off[2];
    if (tid < 2) s_off[tid] = C.block_nnz[2 * k + tid];
    const bool head = sl == 0;  // the slice that writes the block's structure
    if (!load_block<true>(P, S, k, head)) return;
    const int bs = S.blk[0], bn = S.blk[1], as = S.blk[2], an = S.blk[3];
    if (head) build_structure(P, k, bs, bn, as, an, S.src, S.dst, S.in, S.out, S.w, S.start, s_pm, s_pt, s_pg, s_pa, s_off);
    if (P.lean) return;
    // feature rows (8 columns per thread-step, slice sl of them): atoms natural + blocked (zero rows past
    // an), bonds natural
    write_atom_rows(P, S, k, sl, nsl);
    for (int u = tid + 256 * sl; u < bn * UB; u += 256 * nsl) {
        const int lb = u / UB, c0 = (u % UB) * 8;
        const WdAtomCode &cd = S.code[S.src[lb]];
        const int tail = S.tail[lb];
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = c0 + q;
            if (c < Fa0) v[q] = code_value(cd, c, Fa0);
            else if (c < Fa) v[q] = C.atom_extra[(size_t)(as + S.src[lb]) * da + (c - Fa0)];
            else if (c < Fx) v[q] = (float)((tail >> (c - Fa)) & 1);
            else if (c < Fb) v[q] = C.bond_extra[(size_t)((bs + lb - 1) >> 1) * db + (c - Fx)];
            else v[q] = 0.f;
        }
        put_row8(P.f_bonds + (size_t)(bs + lb) * P.ldb, P.fb_x6, P.ldb, bs + lb, c0, v);
    }
}

// ------------------------------------------------------------------------------------------------
// atom-message mode (mpn.py:47-53, 93-94, 104-108, 126-128): the same compact image and block plan, the graph
// the atom-message kernels read.  Message rows are atoms, and every atom's entry counts are its degree, so
// every offset follows from the block table: the bonds before a block are the in-bonds of the atoms before it.
//   bond_feat_gather row a = in(a), atom_gather row a = (src(j), w_bonds[src(j)]) for j in in(a) -- the
//     reference indexes w_bonds with the ATOM id (mpn.py:128) -- zero coefficients kept: entry bs - 1 + e of
//     both lists belongs to the bond in slot e of the block's in-lists;
//   msg_gather row a = (src(j), 1) for j in in(a), then the pad slots' (0, max_num_bonds - deg(a)), written even
//     when 0: a + 1 + (entries of in() before a) entries precede row a's pad entry; row 0 = (0, max_num_bonds);
//   the transposes over atoms: row a' of either lists dst(j) for j in out(a'), ordered by the slot of j in the
//     in-lists (= increasing forward row, then position in it: Csr.transpose); msg_gather_t row 0 = every atom's
//     pad entry;
//   ELL-8 rows per atom with block-local atom indices (msg: the real entries only; atom: CSR entry q in slot q);
//   f_bonds rows hold the bond's own columns only (bits ‖ bond extras), atom_feat_sum_x6 the planes of the per-atom
//     sums of those rows over in(a), fp32, added in list order.
// Slices as in graph_build_kernel: slice 0 writes the structure, every slice a share of the feature rows.
// ------------------------------------------------------------------------------------------------
struct GraphBuildAtomP {
    WdCompact c;
    int Fa, Fb, lda, ldb, Vap, Rbp, max_nb;  // Fb: the bond's own columns (c.bond_fdim - c.atom_fdim)
    float *f_atoms, *f_bonds;
    uint8_t *fa_x6, *fb_x6, *fa_blk_x6, *fs_x6;
    float *w_atoms, *xn;
    int32_t *mol_start, *mol_size, *b2revb, *blocks, *bond_blk_row, *atom_blk_row;
    uint8_t *msg_ell_idx, *agg_ell_idx;
    float *msg_ell_coef, *agg_ell_coef;
    int32_t *feat_ptr, *feat_idx, *msg_ptr, *msg_idx, *agg_ptr, *agg_idx, *msgt_ptr, *msgt_idx, *aggt_ptr, *aggt_idx;
    float *feat_coef, *msg_coef, *agg_coef, *msgt_coef, *aggt_coef;
};

// w_bonds[i] from the pair records: bond i is pair (i - 1) >> 1, direction (i - 1) & 1 (pad bond 0: 0)
__device__ __forceinline__ float pair_weight(const WdCompact &C, int i) {
    if (i < 1 || i >= C.n_bonds) return 0.f;
    const WdBondPair &q = C.pairs[(i - 1) >> 1];
    return ((i - 1) & 1) ? q.w21 : q.w12;
}

// 8 consecutive columns c0 .. c0 + 7 of an atom-mode bond row: bit columns [0, nbits), bond extras [nbits, Fb)
__device__ __forceinline__ void atom_mode_bond_row8(const WdCompact &C, int tail, int pair, int c0, int nbits, int Fb,
                                                    float (&v)[8]) {
    const int db = C.bond_extra_dim;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = c0 + q;
        v[q] = c < nbits ? (float)((tail >> c) & 1) : (c < Fb ? C.bond_extra[(size_t)pair * db + (c - nbits)] : 0.f);
    }
}

// grid: (n_blocks + 1) x GB_SLICES
__global__ __launch_bounds__(256) void graph_build_atom_kernel(const GraphBuildAtomP P) {
    const int k = blockIdx.x, tid = threadIdx.x, sl = blockIdx.y, nsl = gridDim.y;
    const WdCompact &C = P.c;
    const int V1 = C.n_atoms, E1 = C.n_bonds, UB = P.ldb / 8, Fb = P.Fb, nbits = Fb - C.bond_extra_dim;
    if (k == C.n_blocks && sl != 0) return;
    if (k == C.n_blocks) {  // pad rows, row 0 of every list, the dummy entries past the lists' ends
        zero_pad_rows(P.f_atoms, P.fa_x6, P.lda, V1, P.Vap);
        zero_pad_rows(P.f_bonds, P.fb_x6, P.ldb, E1, P.Rbp);
        zero_pad_rows(nullptr, P.fs_x6, P.ldb, V1, P.Vap);
        for (int i = tid; i < 1 + (P.Vap - V1); i += 256) {
            const int r = i == 0 ? 0 : V1 + i - 1;
            P.atom_blk_row[r] = -1;
            for (int s = 0; s < GB_ELLW; ++s) {
                P.msg_ell_idx[GB_ELLW * r + s] = 0; P.msg_ell_coef[GB_ELLW * r + s] = 0.f;
                P.agg_ell_idx[GB_ELLW * r + s] = 0; P.agg_ell_coef[GB_ELLW * r + s] = 0.f;
            }
        }
        for (int i = tid; i < 1 + (P.Rbp - E1); i += 256) P.bond_blk_row[i == 0 ? 0 : E1 + i - 1] = -1;
        if (tid < 2) {  // row 0: the pad slots only (msg), nothing (the others); msg_t row 0: every atom's pad entry
            P.feat_ptr[tid] = 0; P.agg_ptr[tid] = 0; P.aggt_ptr[tid] = 0;
            P.msg_ptr[tid] = tid;
            P.msgt_ptr[tid] = tid * V1;
        }
        if (tid == 0) {
            P.w_atoms[0] = 0.f; P.b2revb[0] = 0;
            P.msg_idx[0] = 0; P.msg_coef[0] = (float)P.max_nb;
            P.msgt_idx[0] = 0; P.msgt_coef[0] = (float)P.max_nb;
        }
        if (tid < GB_CSR_PAD) {  // readable dummy entries past the end (WdCsr)
            const int n1 = E1 - 1 + tid, n2 = E1 - 1 + V1 + tid;
            P.feat_idx[n1] = 0; P.feat_coef[n1] = 0.f;
            P.agg_idx[n1] = 0; P.agg_coef[n1] = 0.f;
            P.aggt_idx[n1] = 0; P.aggt_coef[n1] = 0.f;
            P.msg_idx[n2] = 0; P.msg_coef[n2] = 0.f;
            P.msgt_idx[n2] = 0; P.msgt_coef[n2] = 0.f;
        }
        return;
    }

    __shared__ GbBlock S;
    __shared__ uint8_t s_slot[GB_BONDS];  // a bond's slot in the in-lists
    __shared__ float s_wq[GB_ATOMS];      // w_bonds[atom id] (the atom gather's coefficient of a source atom)
    const bool head = sl == 0;
    if (!load_block<false>(P, S, k, head)) return;
    const int bs = S.blk[0], bn = S.blk[1], as = S.blk[2], an = S.blk[3];
    const int slot = build_in_out(bn, an, S.src, S.dst, S.in, S.out, S.start);
    if (tid < bn) s_slot[tid] = (uint8_t)slot;
    if (tid < an) s_wq[tid] = pair_weight(C, as + tid);
    __syncthreads();
    if (head) {
        // entries of in() before the block = its first bond - 1; rows before atom as: as (row 0 included)
        const int e0 = bs - 1;
        if (tid < bn) {  // one thread per bond j: its entry of the three forward lists, and of the two transposes
            const int j = tid, la = S.dst[j], ls = S.src[j], e = s_slot[j];
            P.feat_idx[e0 + e] = bs + j; P.feat_coef[e0 + e] = 1.f;
            P.agg_idx[e0 + e] = as + ls; P.agg_coef[e0 + e] = s_wq[ls];
            const int m = e0 + e + as + la;  // + one pad entry per earlier row
            P.msg_idx[m] = as + ls; P.msg_coef[m] = 1.f;
            int rank = 0;  // among out(src(j)), by slot
            for (int x = S.start[ls]; x < S.start[ls + 1]; ++x) rank += s_slot[S.out[x]] < e;
            const int t = e0 + S.start[ls] + rank;
            P.msgt_idx[V1 + t] = as + la; P.msgt_coef[V1 + t] = 1.f;
            P.aggt_idx[t] = as + la; P.aggt_coef[t] = s_wq[ls];
        }
        if (tid < an) {  // one thread per atom: row ends, the pad entries, the ELL-8 rows
            const int a = as + tid, r0 = S.start[tid], r1 = S.start[tid + 1], d = r1 - r0;
            const float pad = (float)(P.max_nb - d);
            P.feat_ptr[a + 1] = e0 + r1; P.agg_ptr[a + 1] = e0 + r1; P.aggt_ptr[a + 1] = e0 + r1;
            P.msgt_ptr[a + 1] = V1 + e0 + r1;
            P.msg_ptr[a + 1] = e0 + r1 + a + 1;
            P.msg_idx[e0 + r1 + a] = 0; P.msg_coef[e0 + r1 + a] = pad;
            P.msgt_idx[a] = a; P.msgt_coef[a] = pad;
            uint8_t eidx[GB_ELLW];
            float ecoef[GB_ELLW], ones[GB_ELLW];
#pragma unroll
            for (int q = 0; q < GB_ELLW; ++q) {
                const bool in_row = q < d;
                const int ls = in_row ? S.src[S.in[r0 + q]] : 0;
                eidx[q] = (uint8_t)ls;
                ecoef[q] = in_row ? s_wq[ls] : 0.f;
                ones[q] = in_row ? 1.f : 0.f;
            }
            if (d > GB_ELLW) eidx[GB_ELLW - 1] |= 0x80;
#pragma unroll
            for (int q = 0; q < GB_ELLW; ++q) {
                P.msg_ell_idx[(size_t)GB_ELLW * a + q] = eidx[q]; P.msg_ell_coef[(size_t)GB_ELLW * a + q] = ones[q];
                P.agg_ell_idx[(size_t)GB_ELLW * a + q] = eidx[q]; P.agg_ell_coef[(size_t)GB_ELLW * a + q] = ecoef[q];
            }
        }
    }
    write_atom_rows(P, S, k, sl, nsl);
    for (int u = tid + 256 * sl; u < bn * UB; u += 256 * nsl) {  // f_bonds rows
        const int lb = u / UB, c0 = (u % UB) * 8;
        float v[8];
        atom_mode_bond_row8(C, S.tail[lb], (bs + lb - 1) >> 1, c0, nbits, Fb, v);
        put_row8(P.f_bonds + (size_t)(bs + lb) * P.ldb, P.fb_x6, P.ldb, bs + lb, c0, v);
    }
    for (int u = tid + 256 * sl; u < an * UB; u += 256 * nsl) {  // planes of the sums over in(a), list order
        const int la = u / UB, c0 = (u % UB) * 8;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int e = S.start[la]; e < S.start[la + 1]; ++e) {
            const int lb = S.in[e];
            float v[8];
            atom_mode_bond_row8(C, S.tail[lb], (bs + lb - 1) >> 1, c0, nbits, Fb, v);
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] += v[q];
        }
        x6_store8<64>(P.fs_x6, P.ldb, as + la, c0, make_float4(acc[0], acc[1], acc[2], acc[3]),
                      make_float4(acc[4], acc[5], acc[6], acc[7]));
    }
}

}  // namespace wd
