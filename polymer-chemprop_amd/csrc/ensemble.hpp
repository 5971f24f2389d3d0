// ------------------------------------------------------------------------------------------------
// Ensembles on the device (wdmpnn_ensemble_add, wdmpnn_ensemble_sid): the running mean and variance of the
// predictions of M models, and the pairwise SID of an ensemble of spectra (spectra_utils.py:211-241), in
// double precision like the numpy float64 sums they replace (make_predictions.py:129-201).
//   ensemble_add_kernel   one thread per cell of the [B][W] block, grid-stride: v = pred * std + mean_s (two
//                         separately rounded operations, as numpy's inverse_transform), then Welford's update
//                         of that cell's mean and m2; v kept in the model's slab when asked for
//   ensemble_sid_kernel   one workgroup per row; a thread takes positions t, t + 256, ...: the M values and
//                         their M logs once per position (registers: the loops over models are unrolled over
//                         the template bound MM >= M, so nothing is indexed dynamically and nothing spills),
//                         then the M (M - 1) / 2 pair terms (p_a - p_b) (log p_a - log p_b); per-thread sums,
//                         then a tree over LDS in a fixed order
// No atomics, fixed thread-to-element maps and reduction orders, plain vector stores.
// ------------------------------------------------------------------------------------------------
#pragma once
namespace wd {
constexpr int ENSEMBLE_MAX_MODELS = WD_ENSEMBLE_MAX_MODELS;

struct EnsembleAddArgs {
    const float *pred;
    const double *scale_mean, *scale_std;
    double *mean, *m2, *keep;
    long long row0;
    int B, W, ld_pred, ld_acc, k;
};

__global__ __launch_bounds__(256) void ensemble_add_kernel(const EnsembleAddArgs A) {
#pragma clang fp contract(off)  // pred * std + mean_s and Welford's terms round after every operation
    const size_t total = (size_t)A.B * A.W;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(t / A.W), c = (int)(t - (size_t)b * A.W);
        double v = (double)A.pred[(size_t)b * A.ld_pred + c];
        if (A.scale_std) {
            v = v * A.scale_std[c];
            v = v + A.scale_mean[c];
        }
        const size_t at = (size_t)(A.row0 + b) * A.ld_acc + c;
        if (A.keep) A.keep[at] = v;
        if (A.k == 0) {
            A.mean[at] = v;
            if (A.m2) A.m2[at] = 0.0;
        } else {
            double mean = A.mean[at];
            const double d = v - mean;
            mean = mean + d / (double)(A.k + 1);
            A.mean[at] = mean;
            if (A.m2) A.m2[at] = A.m2[at] + d * (v - mean);
        }
    }
}

struct EnsembleSidArgs {
    const double *preds;
    double *out;
    long long model_stride;
    double threshold;
    int ld, M, T;
};

template <int MM>
__global__ __launch_bounds__(256) void ensemble_sid_kernel(const EnsembleSidArgs A) {
    __shared__ double red[256];
    const double *row = A.preds + (size_t)blockIdx.x * A.ld;
    double acc = 0.0;
    for (int t = threadIdx.x; t < A.T; t += 256) {
        double p[MM], l[MM];
#pragma unroll
        for (int a = 0; a < MM; ++a) {
            p[a] = 1.0;
            if (a < A.M) p[a] = row[(size_t)a * A.model_stride + t];
        }
        if (p[0] != p[0]) continue;  // excluded for this row (model 0 holds NaN): contributes 0
#pragma unroll
        for (int a = 0; a < MM; ++a) {
            if (A.threshold > 0.0 && p[a] < A.threshold) p[a] = A.threshold;
            l[a] = a < A.M ? log(p[a]) : 0.0;
        }
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < MM - 1; ++a) {
#pragma unroll
            for (int b = a + 1; b < MM; ++b)
                if (b < A.M) s += (p[a] - p[b]) * (l[a] - l[b]);
        }
        acc += s;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    // the mean over the M (M - 1) / 2 pairs; one model: 0 / 0 = NaN, numpy's mean over no pairs
    if (threadIdx.x == 0) A.out[blockIdx.x] = red[0] / (0.5 * (double)A.M * (double)(A.M - 1));
}

}  // namespace wd
