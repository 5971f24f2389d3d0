// atom_desc.hpp — atom descriptors from a device-resident table (wdmpnn.h "Atom descriptors").
//
// atom_descriptors_layer is a Linear without an activation and the readout is linear in the atom rows, so with
// encoder dropout inactive the two commute (DESIGN.md §3 "Descriptor layer after the readout"):
//     readout([h | desc] W_d^T + b_d) = [readout(h) | readout(desc)] W_d^T + s_b b_d,   s_b = sum_a c_a
// desc_join_kernel builds x = [readout(h) | readout(desc) | s] per molecule from the table, desc_layer_kernel
// applies the layer to the B rows, desc_layer_bwd_kernel gives dW_d | db_d | d readout(h) in one launch.
// desc_rows_kernel fills the padded per-atom array of the per-atom path (active dropout) from the same table.
//
// All four are small and latency-bound: fp32 FMA, wave64, fixed thread-to-element maps, fixed summation orders
// (k increasing), no atomics, plain vector stores: bitwise repeatable.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace wd {

// ---------------------------------------------------------------------------------------------
// Join: one workgroup per molecule, thread t takes the columns t, t + 256, ...: a column below H is a word
// copy of emb, column H + j the weighted sum of table column j over the molecule's atoms in index order, column
// H + d the weight sum itself.  Every summing thread also forms the weight sum (the same loop, the same order),
// the mean's denominator.  The sum is divided afterwards: a zero weight sum under mean gives 0 / 0 = NaN.
// ---------------------------------------------------------------------------------------------
struct DescJoinArgs {
    const uint32_t *emb;
    const float *table;
    const int64_t *row0;
    const int32_t *mol_start, *mol_size;
    const float *w_atoms, *xn;
    uint32_t *x;
    float norm;
    int H, d, ld_emb, ld_table, ld_x, agg;
};

__global__ __launch_bounds__(256) void desc_join_kernel(const DescJoinArgs A) {
    const int b = blockIdx.x;
    const int a0 = A.mol_start[b], n = A.mol_size[b];
    const int64_t r0 = A.row0[b];
    const float xn = A.xn[b];
    const uint32_t *emb = A.emb + (size_t)b * A.ld_emb;
    uint32_t *x = A.x + (size_t)b * A.ld_x;
    const int cols = A.H + A.d + 1;
    for (int c = threadIdx.x; c < cols; c += 256) {
        if (c < A.H) {
            x[c] = emb[c];
            continue;
        }
        const int j = c - A.H;
        const float *w = A.w_atoms + a0;
        float s = 0.f, wsum = 0.f;
        if (j < A.d) {
            const float *t = A.table + r0 * A.ld_table + j;
            for (int a = 0; a < n; ++a) {
                const float wa = w[a];
                s = fmaf(wa, t[(size_t)a * A.ld_table], s);
                wsum += wa;
            }
        } else {
            for (int a = 0; a < n; ++a) wsum += w[a];
            s = wsum;
        }
        const float m = A.agg == 0 ? s / wsum : (A.agg == 2 ? s / A.norm : s);
        x[c] = __float_as_uint(xn * m);
    }
}

// ---------------------------------------------------------------------------------------------
// A 16 x 16 tile of C[m][n] = sum_k A(m, k) B(n, k), k increasing, one thread per element, the operands staged
// 16 k at a time through LDS.  Either operand is addressed by two strides (row, k), so the same code serves
// x W_d^T (k along both rows), dy^T x (k across the rows of both) and dy W_d (k along dy's rows, across W_d's).
// Elements outside (M, N, K) are staged as 0 and add nothing.  Returns the thread's element (tm, tn).
// ---------------------------------------------------------------------------------------------
struct TileOp {
    const float *p;
    int64_t s_row, s_k;
    int rows;  // valid rows of this operand
};

__device__ __forceinline__ float desc_tile16(const TileOp Aop, const TileOp Bop, int m0, int n0, int K,
                                             float (*As)[17], float (*Bs)[17]) {
    const int tid = threadIdx.x;
    const int tm = tid >> 4, tn = tid & 15;
    // staging map: the operand's contiguous direction along the 16 neighbouring lanes
    const int ar = Aop.s_k == 1 ? tm : tn, ak = Aop.s_k == 1 ? tn : tm;
    const int br = Bop.s_k == 1 ? tm : tn, bk = Bop.s_k == 1 ? tn : tm;
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        float av = 0.f, bv = 0.f;
        if (m0 + ar < Aop.rows && k0 + ak < K) av = Aop.p[(int64_t)(m0 + ar) * Aop.s_row + (int64_t)(k0 + ak) * Aop.s_k];
        if (n0 + br < Bop.rows && k0 + bk < K) bv = Bop.p[(int64_t)(n0 + br) * Bop.s_row + (int64_t)(k0 + bk) * Bop.s_k];
        __syncthreads();  // the previous chunk's reads are done
        As[ar][ak] = av;
        Bs[br][bk] = bv;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = fmaf(As[tm][k], Bs[tn][k], acc);
    }
    return acc;
}

// y[b][i] = sum_{j < Hd} x[b][j] W[i][j] + x[b][Hd] bias[i].  grid = (ceil(Hd / 16), ceil(B / 16)).
struct DescLayerArgs {
    const float *x, *W, *bias;
    float *y;
    int B, Hd, ld_x, ld_y;
};

__global__ __launch_bounds__(256) void desc_layer_kernel(const DescLayerArgs A) {
    __shared__ float As[16][17], Bs[16][17];
    const int b0 = blockIdx.y * 16, i0 = blockIdx.x * 16;
    const float acc = desc_tile16(TileOp{A.x, A.ld_x, 1, A.B}, TileOp{A.W, A.Hd, 1, A.Hd}, b0, i0, A.Hd, As, Bs);
    const int b = b0 + (threadIdx.x >> 4), i = i0 + (threadIdx.x & 15);
    if (b >= A.B || i >= A.Hd) return;
    float v = acc;
    if (A.bias) v = fmaf(A.x[(size_t)b * A.ld_x + A.Hd], A.bias[i], v);
    A.y[(size_t)b * A.ld_y + i] = v;
}

// One launch, two kinds of tiles in one grid (the workgroup index decides, uniformly per workgroup):
//   [0, n_w)        dWext[i][j] = sum_b dy[b][i] x[b][j], j in [16 jt0, 16 jt0 + 16 jt_n): j < Hd goes to dW
//                   [Hd][Hd], j == Hd (the s column of x) to db
//   [n_w, n_w + n_e) demb[b][h] = sum_i dy[b][i] W[i][h], h < H
struct DescLayerBwdArgs {
    const float *dy, *x, *W;
    float *dW, *db, *demb;
    int B, H, Hd, ld_dy, ld_x, ld_demb;
    int jt0, jt_n, n_w, e_cols;  // first column tile and column tiles of the dW part; its tiles; demb column tiles
};

__global__ __launch_bounds__(256) void desc_layer_bwd_kernel(const DescLayerBwdArgs A) {
    __shared__ float As[16][17], Bs[16][17];
    const int wg = blockIdx.x;
    const int tm = threadIdx.x >> 4, tn = threadIdx.x & 15;
    if (wg < A.n_w) {
        const int i0 = (wg / A.jt_n) * 16, j0 = (A.jt0 + wg % A.jt_n) * 16;
        const float acc = desc_tile16(TileOp{A.dy, 1, A.ld_dy, A.Hd}, TileOp{A.x, 1, A.ld_x, A.Hd + 1}, i0, j0, A.B,
                                      As, Bs);
        const int i = i0 + tm, j = j0 + tn;
        if (i >= A.Hd) return;
        if (j < A.Hd) {
            if (A.dW) A.dW[(size_t)i * A.Hd + j] = acc;
        } else if (j == A.Hd && A.db) {
            A.db[i] = acc;
        }
        return;
    }
    const int e = wg - A.n_w;
    const int b0 = (e / A.e_cols) * 16, h0 = (e % A.e_cols) * 16;
    const float acc = desc_tile16(TileOp{A.dy, A.ld_dy, 1, A.B}, TileOp{A.W, 1, A.Hd, A.H}, b0, h0, A.Hd, As, Bs);
    const int b = b0 + tm, h = h0 + tn;
    if (b < A.B && h < A.H) A.demb[(size_t)b * A.ld_demb + h] = acc;
}

// ---------------------------------------------------------------------------------------------
// The padded per-atom array [rows][ld] of the per-atom path: atom_desc[mol_start_b + a][j] = table[row0_b + a][j],
// everything else 0 (the pad row 0, rows outside every molecule, the tail rows, the pad columns).  One thread
// per element; an atom row finds its molecule by bisection over mol_start (non-decreasing, as a_scope is).
// ---------------------------------------------------------------------------------------------
struct DescRowsArgs {
    const uint32_t *table;
    const int64_t *row0;
    const int32_t *mol_start, *mol_size;
    uint32_t *out;
    int B, d, ld_table, rows, ld, n_atoms;
};

__global__ __launch_bounds__(256) void desc_rows_kernel(const DescRowsArgs A) {
    const size_t total = (size_t)A.rows * A.ld;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(t / A.ld), c = (int)(t % A.ld);
        uint32_t v = 0u;
        if (c < A.d && r >= 1 && r < A.n_atoms) {
            int lo = 0, hi = A.B;  // the last molecule with mol_start <= r, if any
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (A.mol_start[mid] <= r) lo = mid + 1; else hi = mid;
            }
            // (molecules of size 0 share their start with the next one: step back over them)
            int m = lo - 1;
            while (m >= 0 && A.mol_size[m] == 0) --m;
            if (m >= 0) {
                const int a = r - A.mol_start[m];
                if (a >= 0 && a < A.mol_size[m]) v = A.table[(A.row0[m] + a) * A.ld_table + c];
            }
        }
        A.out[t] = v;
    }
}

}  // namespace wd
