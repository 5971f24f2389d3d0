// ------------------------------------------------------------------------------------------------
// The spectra head (wdmpnn_head_spectra): the head stack's FFN with a wide last layer (one output per
// spectrum bin, T <= WD_HEAD_MAX_SPECTRUM), the output activation s = act_s(z_L) (exp or softplus, model.py:
// 102-113) and the row losses of spectra_utils.py on the masked, row-normalised output p = m s / sum(m s):
//   SID          sum_t w_t (p_t - y_t) (log p_t - log y_t)
//   Wasserstein  sum_t w_t |cumsum(y)_t - cumsum(p)_t|
// with m_t = [y_t != 0] (the table's "0 = missing": every present target is > 0 after normalize_spectra).
// Launches:
//   head_stack_fwd_kernel, l = 1 .. L-1   (kernels.hpp, on a WdHeadStack view)
//   head_spectra_z_kernel                 z_L - b_L = a_{L-1} W_L^T as 16 x 16 tiles over (B, T)
//   head_spectra_rows_kernel              one workgroup per row: max, masked sum, p, log p, the loss terms,
//                                         gbar and dout = d loss / d z_L (scans for Wasserstein), out = act_s(z_L)
//   head_spectra_bwd_kernel               tiles of dz_{L-1} = (dout W_L) drop act' (L == 1: dx) with per-tile
//                                         dslope terms | tiles of dW_L = dout^T a_{L-1} | db_L, the loss
//   head_stack_bwd_kernel, l = L-1 .. 1   (kernels.hpp, StackWant.last = 0; slope = 2: site L-1 per tile)
// Scratch (floats): stack_layout's regions (its a_{L-1} region stays unused: a_{L-1} is rebuilt from z_{L-1}
// as it is staged), then z_L - b_L [B][T].  Reductions and scans: per-thread contiguous chunk, then wave, then
// workgroup, all in fixed order; no float atomics.  exp: p and log p come from the max-subtracted softmax over
// the present positions (finite for any finite logits).  A row without a present target gives loss 0, dout 0.
// ------------------------------------------------------------------------------------------------
#pragma once
namespace wd {
constexpr int HEAD_MAX_SPECTRUM = WD_HEAD_MAX_SPECTRUM;

__host__ __device__ inline size_t head_spectra_floats(int B, int F, int Hf, int T, int L) {
    return head_stack_floats(B, F, Hf, T, L) + (size_t)B * T;
}
__host__ __device__ inline size_t head_spectra_predict_floats(int B, int Hf, int T, int L) {
    return (size_t)(L - 1) * B * Hf + (size_t)B * T;
}

// z_L tiles without the bias: A = a_{L-1} rebuilt from z_{L-1} (L == 1: x) by the site functor, B = W_L, into
// zl [B][T] = a_{L-1} W_L^T.  b_L is added by the row kernels, which take the softmax's differences z_t - z_r as
// (zl_t - zl_r) + (b_t - b_r): a bias of 100 would otherwise round every logit to 7.6e-6 (ulp(100)), an error of
// that relative size in p and in every gradient
__global__ __launch_bounds__(256) void head_spectra_z_kernel(WdHeadStack P, float *zl) {
    __shared__ SmallGemmLds<HEAD_H_TS> L;
    const StackLayout S = stack_layout(P);
    const int Kin = P.L == 1 ? P.F : P.Hf;
    const float *zin = P.L == 1 ? P.x : S.z + (size_t)(P.L - 2) * P.B * P.Hf;
    const SmallGemm G{zin, P.L == 1 ? P.ld_x : P.Hf, 1, P.W[P.L - 1], 1, Kin, nullptr, zl, P.T, P.B, P.T, Kin};
    with_act(P.L == 1 ? (int)ACT_IDENTITY : P.act, [&](auto act_c) {
        constexpr int ACT = decltype(act_c)::value;
        const StackSite<ACT> site{stack_slope(P.slope, P.act), P.p, P.seed, (uint32_t)(P.L - 1)};
        SgIdentity id;
        small_gemm_tile_f<HEAD_H_TS, true, false>(G, blockIdx.x, L, site, id, id);
    });
}

// Workgroup reductions of 256 threads: the wave's butterfly, then the four waves in order.  Every thread
// gets the result.  red: 4 floats of LDS, reusable after the call's own barriers.
__device__ __forceinline__ float block_sum256(float v, float *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float block_max256(float v, float *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
// Exclusive scan of one value per thread in thread order (REV: from thread 255 down): the sum of the values
// of the threads before this one (REV: after it)
template <bool REV>
__device__ __forceinline__ float block_scan256(float v, float *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ll = REV ? 63 - lane : lane, lw = REV ? 3 - wave : wave;
    float x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float t = REV ? __shfl_down(x, off, 64) : __shfl_up(x, off, 64);
        if (ll >= off) x += t;
    }
    float e = REV ? __shfl_down(x, 1, 64) : __shfl_up(x, 1, 64);
    if (ll == 0) e = 0.f;
    __syncthreads();
    if (ll == 63) red[lw] = x;
    __syncthreads();
    float pre = 0.f;
    for (int i = 0; i < lw; ++i) pre += red[i];
    return pre + e;
}

__device__ __forceinline__ float softplus_f(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float sigmoid_f(float z) { return 1.f / (1.f + expf(-z)); }

// The reference position of a row's max-subtracted softmax: the first included position whose logit zl_t + b_t
// equals the row's max mx (position 0 if none does: NaN logits), as its product and bias parts
struct SpectraRef { float z, b; };
template <class INC>
__device__ __forceinline__ SpectraRef spectra_ref(const float *zl, const float *bias, int T, int t0, int t1, float mx,
                                                  float *red, const INC &included) {
    float cand = -INFINITY;  // minus the chunk's first index at the max (exact: T <= 8192)
    for (int t = t1 - 1; t >= t0; --t)
        if (included(t) && zl[t] + (bias ? bias[t] : 0.f) == mx) cand = -(float)t;
    cand = block_max256(cand, red);
    const int r = cand > -INFINITY ? min(T - 1, max(0, (int)-cand)) : 0;
    return {zl[r], bias ? bias[r] : 0.f};
}

struct SpectraRows {
    const float *zl;                       // [B][T]: z_L - b_L
    const float *bias;                     // b_L [T] or NULL
    const float *table; int ld_table;      // targets (0 = missing) | weights
    int B, T;
    float inv_n;
    int spectra_act, loss_kind;
    float *out;                            // [B][T] or NULL
    float *dout;                           // [B][T]: d loss / d z_L
    float *lossrow;                        // [B]
};

// One workgroup per row.  Thread t owns the contiguous chunk [t c, (t + 1) c) of the row, c = ceil(T / 256);
// the row's per-position products g_t p_t (g = d loss / d p) stay in LDS between the passes: with them no
// step divides by a p_t that has underflowed to 0 (logits 200 below the row's max).
__global__ __launch_bounds__(256) void head_spectra_rows_kernel(SpectraRows P) {
    __shared__ float gsh[HEAD_MAX_SPECTRUM];
    __shared__ float red[4];
    const int row = blockIdx.x, T = P.T, tid = threadIdx.x;
    const int c = (T + 255) / 256, t0 = min(T, tid * c), t1 = min(T, t0 + c);
    const float *zl = P.zl + (size_t)row * T, *bias = P.bias;
    const float *y = P.table + (size_t)row * P.ld_table, *w = y + T;
    float *dout = P.dout + (size_t)row * T;
    const bool ex = P.spectra_act == 0;
    auto bt = [&](int t) { return bias ? bias[t] : 0.f; };
    auto z = [&](int t) { return zl[t] + bt(t); };
    if (P.out)
        for (int t = t0; t < t1; ++t) P.out[(size_t)row * T + t] = ex ? expf(z(t)) : softplus_f(z(t));
    // the max over the present positions (-inf: none present)
    float mx = -INFINITY;
    for (int t = t0; t < t1; ++t)
        if (y[t] != 0.f) mx = fmaxf(mx, z(t));
    mx = block_max256(mx, red);
    if (!(mx > -INFINITY)) {
        for (int t = t0; t < t1; ++t) dout[t] = 0.f;
        if (tid == 0) P.lossrow[row] = 0.f;
        return;
    }
    // the reference position r: the first present one at the max
    const SpectraRef R = spectra_ref(zl, bias, T, t0, t1, mx, red, [&](int t) { return y[t] != 0.f; });
    auto dif = [&](int t) { return (zl[t] - R.z) + (bt(t) - R.b); };  // z_t - z_r
    // S = sum of the present act_s(z) (exp: of exp(z - z_r))
    float S = 0.f;
    for (int t = t0; t < t1; ++t)
        if (y[t] != 0.f) S += ex ? expf(dif(t)) : softplus_f(z(t));
    S = block_sum256(S, red);
    const float logS = logf(S), invS = 1.f / S;
    // p_t and log p_t of a present position
    auto prob = [&](int t, float &lp) {
        if (ex) {
            lp = dif(t) - logS;
            return expf(lp);
        }
        const float p = softplus_f(z(t)) * invS;
        lp = logf(p);
        return p;
    };
    float ls = 0.f, gb = 0.f;  // the row's loss, gbar = sum_t m_t g_t p_t
    if (P.loss_kind == 0) {
        // g_t = w_t (log(p_t / y_t) + 1 - y_t / p_t), kept as g_t p_t = w_t (p_t (log(p_t / y_t) + 1) - y_t)
        for (int t = t0; t < t1; ++t) {
            const float yt = y[t];
            float gp = 0.f;
            if (yt != 0.f) {
                float lp;
                const float p = prob(t, lp), d = lp - logf(yt), wt = w[t];
                ls = fmaf(wt * (p - yt), d, ls);
                gp = wt * fmaf(p, d + 1.f, -yt);
                gb += gp;
            }
            gsh[t] = gp;
        }
    } else {
        // cumsum(p) and cumsum(y) up to the chunk, then through it: q_t = w_t sign(cumsum(p)_t - cumsum(y)_t)
        float sp = 0.f, sy = 0.f;
        for (int t = t0; t < t1; ++t) {
            const float yt = y[t];
            float lp;
            if (yt != 0.f) sp += prob(t, lp);
            sy += yt;
        }
        float cp = block_scan256<false>(sp, red), cy = block_scan256<false>(sy, red);
        float sq = 0.f;
        for (int t = t0; t < t1; ++t) {
            const float yt = y[t], wt = w[t];
            float lp;
            if (yt != 0.f) cp += prob(t, lp);
            cy += yt;
            const float d = cp - cy;
            ls = fmaf(wt, fabsf(d), ls);
            const float q = d > 0.f ? wt : d < 0.f ? -wt : 0.f;
            gsh[t] = q;
            sq += q;
        }
        // g_u = sum_{t >= u} q_t: the chunks after this one, then the chunk from its end
        float g = block_scan256<true>(sq, red);
        for (int t = t1 - 1; t >= t0; --t) {
            g += gsh[t];
            float lp;
            const float gp = y[t] != 0.f ? g * prob(t, lp) : 0.f;
            gb += gp;
            gsh[t] = gp;
        }
    }
    ls = block_sum256(ls, red);
    gb = block_sum256(gb, red);
    if (tid == 0) P.lossrow[row] = ls;
    // d loss / d s_u = m_u (g_u - gbar) / S = (g_u p_u - gbar p_u) / s_u, times act_s'(z_u): s_u for exp
    for (int t = t0; t < t1; ++t) {
        float d = 0.f;
        if (y[t] != 0.f) {
            float lp;
            const float zt = z(t), p = prob(t, lp);
            d = fmaf(-gb, p, gsh[t]);
            if (!ex) d *= sigmoid_f(zt) / softplus_f(zt);
            d *= P.inv_n;
        }
        dout[t] = d;
    }
}

// The last layer's backward in one launch, the wanted ranges in this order: tiles of dz_{L-1} (L == 1: dx) with
// each tile's dslope term, tiles of dW_L, then one thread per element of db_L, the loss (and dslope = 0 for
// L == 1).  Q.dz / Q.dw / Q.db as in head_stack_bwd_kernel; a range nobody wants takes no workgroups.
__host__ __device__ inline long long spectra_bwd_tail(const WdHeadStack &P, const StackWant &Q) {
    return (Q.db ? P.T : 0) + 1;
}
__host__ __device__ inline long long spectra_bwd_blocks(const WdHeadStack &P, const StackWant &Q) {
    const int Kin = P.L == 1 ? P.F : P.Hf;
    return (Q.dz ? head_tiles(P.B, Kin, HEAD_H_TS) : 0) + (Q.dw ? head_tiles(P.T, Kin, HEAD_G_TS) : 0) +
           (spectra_bwd_tail(P, Q) + 255) / 256;
}
__global__ __launch_bounds__(256) void head_spectra_bwd_kernel(WdHeadStack P, StackWant Q) {
    __shared__ SmallGemmLds<HEAD_G_TS> L;
    __shared__ float red[256];
    const StackLayout S = stack_layout(P);
    const int B = P.B, T = P.T, Ln = P.L, Kin = Ln == 1 ? P.F : P.Hf;
    const float *prev = Ln == 1 ? P.x : S.z + (size_t)(Ln - 2) * B * P.Hf;  // site L-1's stored values
    const long long ldp = Ln == 1 ? P.ld_x : P.Hf;
    float *dzo = Ln == 1 ? P.dx : S.dz + (size_t)(Ln - 2) * B * P.Hf;
    const SmallGemm GX{S.dout, T, 1, P.W[Ln - 1], Kin, 1, nullptr, dzo, ldp, B, Kin, T};
    const SmallGemm GW{S.dout, 1, T, prev, ldp, 1, nullptr, P.dW[Ln - 1], Kin, T, Kin, B};
    const int n1 = Q.dz ? head_tiles(GX.M, GX.N, HEAD_H_TS) : 0, n2 = Q.dw ? head_tiles(GW.M, GW.N, HEAD_G_TS) : 0;
    const int b = blockIdx.x;
    if (b < n1 + n2) {
        with_act(Ln == 1 ? (int)ACT_IDENTITY : P.act, [&](auto act_c) {
            constexpr int ACT = decltype(act_c)::value;
            const StackSite<ACT> site{stack_slope(P.slope, P.act), P.p, P.seed, (uint32_t)(Ln - 1)};
            SgIdentity id;
            if (b >= n1) {
                small_gemm_tile_f<HEAD_G_TS, false, true>(GW, b - n1, L, id, site, id);
                return;
            }
            StackDz<ACT> dzf{site, prev, ldp, 0.f};
            small_gemm_tile_f<HEAD_H_TS, true, true>(GX, b, *reinterpret_cast<SmallGemmLds<HEAD_H_TS> *>(&L), id, id, dzf);
            if (ACT == ACT_PRELU) {  // the tile's dslope term: the 256 threads' terms in thread order
                red[threadIdx.x] = dzf.part;
                __syncthreads();
                if (threadIdx.x == 0) {
                    float t = 0.f;
                    for (int e = 0; e < 256; ++e) t += red[e];
                    S.spart[(size_t)(Ln - 2) * S.np + b] = t;
                }
            }
        });
        return;
    }
    const long long ndb = Q.db ? T : 0;
    const long long q = (long long)(b - n1 - n2) * 256 + threadIdx.x;
    if (q < ndb) {
        P.db[Ln - 1][q] = row_sum(S.dout + q, T, nullptr, 0, B);
    } else if (q == ndb) {
        P.loss[0] = row_sum(S.lossrow, 1, nullptr, 0, B) * P.inv_n;
        if (Ln == 1 && P.dslope) P.dslope[0] = 0.f;
    }
}

struct SpectraPredictRows {
    const float *zl;       // [B][T]: z_L - b_L
    const float *bias;     // b_L [T] or NULL
    float *out;            // [B][T]
    const uint8_t *mask;   // [B][T] or NULL (all included)
    int B, T, spectra_act, normalize;
};
// prediction, one workgroup per row: out = act_s(z_L), or (normalize) the included positions divided by their
// sum (exp: max-subtracted) and a quiet NaN at the excluded ones
__global__ __launch_bounds__(256) void head_spectra_predict_rows_kernel(SpectraPredictRows P) {
    __shared__ float red[4];
    const int row = blockIdx.x, T = P.T, tid = threadIdx.x;
    const int c = (T + 255) / 256, t0 = min(T, tid * c), t1 = min(T, t0 + c);
    const float *zl = P.zl + (size_t)row * T, *bias = P.bias;
    float *out = P.out + (size_t)row * T;
    const uint8_t *m = P.mask ? P.mask + (size_t)row * T : nullptr;
    const bool ex = P.spectra_act == 0;
    auto bt = [&](int t) { return bias ? bias[t] : 0.f; };
    auto z = [&](int t) { return zl[t] + bt(t); };
    if (!P.normalize) {
        for (int t = t0; t < t1; ++t) out[t] = ex ? expf(z(t)) : softplus_f(z(t));
        return;
    }
    float mx = -INFINITY;
    for (int t = t0; t < t1; ++t)
        if (!m || m[t]) mx = fmaxf(mx, z(t));
    mx = block_max256(mx, red);
    const SpectraRef R = spectra_ref(zl, bias, T, t0, t1, mx, red, [&](int t) { return !m || m[t]; });
    auto val = [&](int t) { return ex ? expf((zl[t] - R.z) + (bt(t) - R.b)) : softplus_f(z(t)); };
    float S = 0.f;
    for (int t = t0; t < t1; ++t)
        if (!m || m[t]) S += val(t);
    S = block_sum256(S, red);
    const float invS = 1.f / S;
    for (int t = t0; t < t1; ++t) out[t] = !m || m[t] ? val(t) * invS : __builtin_nanf("");
}
}  // namespace wd
