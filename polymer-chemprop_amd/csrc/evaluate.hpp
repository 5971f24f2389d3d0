// ------------------------------------------------------------------------------------------------
// Scoring a split on the device (wdmpnn_eval_add, wdmpnn_eval_spectra, wdmpnn_eval_auc): the sums behind the
// per-task metrics of evaluate.py:11-77, the per-row spectra terms (spectra_utils.py:42-159) and ROC AUC, from the
// fp32 predictions of the native heads against a resident double target table (NaN = missing), in double
// precision like the sklearn / numpy float64 arithmetic they replace.
//   eval_add_kernel      one workgroup per task; a thread takes rows b, b + 256, ... of the batch, the per-thread
//                        sums go through a tree over LDS in a fixed order, and thread 0 adds the batch's sums to
//                        the running partials (launches on one stream are sequenced: no atomics)
//   eval_spectra_kernel  one workgroup per row; a thread takes a contiguous chunk of the row: the row's sum, the
//                        chunk sums of p and y, their scan over LDS in index order, then the terms
//   eval_auc_kernel      grid (256-row block, task); a thread holds one positive row and streams all rows through
//                        LDS in tiles of 256, counting negatives below it (2) and tied with it (1): integers only
// No atomics, fixed thread-to-element maps and reduction orders, plain vector stores.
// ------------------------------------------------------------------------------------------------
#pragma once
namespace wd {
constexpr int EVAL_SLOTS = WD_EVAL_SLOTS;
constexpr double EVAL_EPS = 2.220446049250313e-16;  // 2^-52: numpy's float64 eps, sklearn's log_loss clip

struct EvalAddArgs {
    const float *pred;
    const double *targets, *scale_mean, *scale_std;
    double *partials;
    float *keep_f;
    double *keep_d;
    long long row0;
    int B, tasks, classes, kind, ld_pred, ld_targets, ld_keep;
};

__device__ __forceinline__ double eval_clip(double p) {
    // np.clip(p, eps, 1 - eps): minimum(maximum(p, eps), 1 - eps)
    p = p < EVAL_EPS ? EVAL_EPS : p;
    return p > 1.0 - EVAL_EPS ? 1.0 - EVAL_EPS : p;
}

__global__ __launch_bounds__(256) void eval_add_kernel(const EvalAddArgs A) {
#pragma clang fp contract(off)  // pred * std + mean_s, e * e and the sums round after every operation
    __shared__ double red[EVAL_SLOTS][256];
    const int task = blockIdx.x, C = A.classes;
    double s[EVAL_SLOTS] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < A.B; b += 256) {
        const float *prow = A.pred + (size_t)b * A.ld_pred + (size_t)task * C;
        const size_t row = (size_t)(A.row0 + b);
        const double t = A.targets[row * A.ld_targets + task];
        const bool present = t == t;
        const size_t kat = row * A.ld_keep + (size_t)task * C;
        if (A.kind == WD_EVAL_REGRESSION) {
            double v = (double)prow[0];
            if (A.scale_std) {
                v = v * A.scale_std[task];
                v = v + A.scale_mean[task];
            }
            if (A.keep_d) A.keep_d[kat] = v;
            if (A.keep_f) A.keep_f[kat] = (float)v;
            if (present) {
                const double e = v - t;
                s[0] = s[0] + e * e;
                s[1] = s[1] + fabs(e);
            }
        } else if (A.kind == WD_EVAL_CLASSIFICATION) {
            const double p = (double)prow[0];
            if (A.keep_d) A.keep_d[kat] = p;
            if (A.keep_f) A.keep_f[kat] = prow[0];
            if (present) {
                const bool one = t == 1.0;
                const double q = 1.0 - p;
                s[0] = s[0] + -log(eval_clip(one ? p : q));
                s[1] = s[1] + ((p > 0.5) == one ? 1.0 : 0.0);
                s[2] = s[2] + (p == 0.0 ? 1.0 : 0.0);
                s[3] = s[3] + (p == 1.0 ? 1.0 : 0.0);
            }
        } else {
            // the first maximum among the classes, as list.index(max(...)); NaN never wins a comparison
            int best = 0;
            float top = prow[0];
            for (int k = 0; k < C; ++k) {
                const float p = prow[k];
                if (A.keep_d) A.keep_d[kat + k] = (double)p;
                if (A.keep_f) A.keep_f[kat + k] = p;
                if (p > top) {
                    top = p;
                    best = k;
                }
            }
            if (present) {
                const int cls = (int)t;  // (checked on the host: an integer in [0, C))
                s[0] = s[0] + -log(eval_clip((double)prow[cls]));
                s[1] = s[1] + (best == cls ? 1.0 : 0.0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < EVAL_SLOTS; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int k = 0; k < EVAL_SLOTS; ++k) red[k][threadIdx.x] = red[k][threadIdx.x] + red[k][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x < EVAL_SLOTS) {
        double *at = A.partials + (size_t)task * EVAL_SLOTS + threadIdx.x;
        *at = *at + red[threadIdx.x][0];
    }
}

struct EvalSpectraArgs {
    const float *pred;
    const double *targets;
    double *sid, *wass;
    float *keep_f;
    double *keep_d;
    long long row0;
    int T, ld_pred, ld_targets, ld_keep;
};

__global__ __launch_bounds__(256) void eval_spectra_kernel(const EvalSpectraArgs A) {
#pragma clang fp contract(off)  // p log(p / y) + y log(y / p) rounds after every operation, as numpy's arrays do
    __shared__ double red[256], cp[256], cy[256];
    const int tid = threadIdx.x;
    const size_t row = (size_t)(A.row0 + blockIdx.x);
    const float *prow = A.pred + (size_t)blockIdx.x * A.ld_pred;
    const double *trow = A.targets + row * A.ld_targets;
    const int chunk = (A.T + 255) / 256;
    const int t0 = min(tid * chunk, A.T), t1 = min(t0 + chunk, A.T);
    // the row's sum over the present positions (excluded predictions are NaN: taken as 0, as _rows does)
    double sum = 0.0;
    for (int t = t0; t < t1; ++t) {
        const float p = prow[t];
        const double y = trow[t];
        if (A.keep_d) A.keep_d[row * A.ld_keep + t] = (double)p;
        if (A.keep_f) A.keep_f[row * A.ld_keep + t] = p;
        if (y == y && p == p) sum = sum + (double)p;
    }
    red[tid] = sum;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    const double total = red[0];
    // chunk sums of the normalised prediction and of the targets (missing = 0)
    double sp = 0.0, sy = 0.0;
    for (int t = t0; t < t1; ++t) {
        const float p = prow[t];
        const double y = trow[t];
        const bool present = y == y;
        sp = sp + (present && p == p ? (double)p : 0.0) / total;
        sy = sy + (present ? y : 0.0);
    }
    cp[tid] = sp;
    cy[tid] = sy;
    __syncthreads();
    // exclusive scans in index order, one lane each (two waves: the two scans run side by side)
    if (tid == 0 || tid == 64) {
        double *c = tid == 0 ? cp : cy;
        double run = 0.0;
        for (int k = 0; k < 256; ++k) {
            const double v = c[k];
            c[k] = run;
            run = run + v;
        }
    }
    __syncthreads();
    double rp = cp[tid], ry = cy[tid], sid = 0.0, wass = 0.0;
    for (int t = t0; t < t1; ++t) {
        const float pf = prow[t];
        const double y = trow[t];
        const bool present = y == y;
        const double p = (present && pf == pf ? (double)pf : 0.0) / total;
        rp = rp + p;
        ry = ry + (present ? y : 0.0);
        wass = wass + fabs(ry - rp);
        if (present) {
            const double a = p * log(p / y), b = y * log(y / p);
            sid = sid + (a + b);
        }
    }
    __syncthreads();  // (red[0] has been read by every thread)
    red[tid] = sid;
    cp[tid] = wass;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            red[tid] = red[tid] + red[tid + h];
            cp[tid] = cp[tid] + cp[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (A.sid) A.sid[row] = red[0];
        if (A.wass) A.wass[row] = cp[0];
    }
}

struct EvalAucArgs {
    const float *preds_f;
    const double *preds_d, *targets;
    long long *counts;
    long long N;
    int ld_preds, ld_targets, blocks;
};

__global__ __launch_bounds__(256) void eval_auc_kernel(const EvalAucArgs A) {
    __shared__ double sp[256];
    __shared__ int sneg[256];
    __shared__ long long red[256];
    const int task = blockIdx.y, tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    auto value = [&](long long r) {
        const size_t at = (size_t)r * A.ld_preds + task;
        return A.preds_f ? (double)A.preds_f[at] : A.preds_d[at];
    };
    double pi = 0.0;
    bool positive = false;
    if (i < A.N) {
        positive = A.targets[(size_t)i * A.ld_targets + task] == 1.0;
        pi = value(i);
    }
    long long count = 0;
    for (long long j0 = 0; j0 < A.N; j0 += 256) {
        const long long j = j0 + tid;
        int neg = 0;
        double pj = 0.0;
        if (j < A.N) {
            neg = A.targets[(size_t)j * A.ld_targets + task] == 0.0;
            pj = value(j);
        }
        sp[tid] = pj;
        sneg[tid] = neg;
        __syncthreads();
        if (positive) {
            for (int k = 0; k < 256; ++k)
                if (sneg[k]) count += 2 * (long long)(sp[k] < pi) + (long long)(sp[k] == pi);
        }
        __syncthreads();
    }
    red[tid] = count;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) A.counts[(size_t)task * A.blocks + blockIdx.x] = red[0];
}

}  // namespace wd
