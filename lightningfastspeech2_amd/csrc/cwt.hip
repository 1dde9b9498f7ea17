// CWT variance targets: CWT.decompose on the device (include/fs2.h "CWT and log variance targets"; DESIGN.md "CWT decomposition on
// the device").  What litfass/dataset/cwt.py:30-46 computes per item over scipy.signal.cwt / ricker as SciPy 1.14 published them,
// restated from that definition: zero replacement, log, mean / std, the normalised signal, and per scale a `same`-mode
// convolution with a Ricker wavelet of a NON-INTEGER point count (so the wavelet is not symmetric about its middle sample).
//
// One launch; a workgroup = one utterance x CWT_TILE consecutive outputs.
//   1. Every tile of an utterance reads the whole row, takes the log in fp64 (rounded to fp32, the reference's dtype) and reduces the
//      mean and the population variance in fp64: thread t adds the entries j = t, t + 256, ... in order, the 256 partials are added
//      by a binary tree.  The order depends on n alone, so every tile holds the same bits; tile 0 stores them.
//   2. x[j] = (signal - mean) / (std + 1e-7) in fp32, as the reference has it, goes into LDS as fp64 (exact) with CWT_TILE zeros on
//      either side.
//   3. Per scale the M wavelet values are generated into LDS once (fp64), then a thread runs the direct form for its two outputs
//      k and k + 256 on the fp64 VALU: one accumulator per output, taps in ascending order.  With h = M / 2 the definition's index
//      M - 1 - (k + (M - 1) / 2 - j) is m = j - k + h, so c[k] = sum_m x[k - h + m] r[m].  The loop's tap range is the union over the
//      tile's outputs; a tap outside an output's own range meets a zero of the padding and adds an exact zero to a finite sum (the
//      accumulator starts at +0 and so never is -0), which leaves the bits of "the valid taps in ascending order".
//      LDS traffic: lane l reads x[base + l], consecutive 8-byte words - conflict-free for ds_read_b64, whose 32-lane groups span
//      the 64 banks once - and r[m], one address for the whole wave (a broadcast).
// No sum's order depends on B, S or the row: results are bitwise batch-invariant.  Nothing at or past values[b][n] is read.
#include <math.h>

#include "fs2_host.h"

namespace fs2 {

static constexpr int CWT_MAX_S = 4096;     // entries of one utterance (fs2_op_contour_finish's cap)
static constexpr int CWT_MAX_SCALES = 16;
static constexpr int CWT_THREADS = 256;
static constexpr int CWT_TILE = 2 * CWT_THREADS;  // outputs one workgroup owns: the kernel's seams lie at its multiples
static constexpr int CWT_AHEAD = 8;               // taps whose LDS reads are issued together
static constexpr size_t CWT_LDS_DEFAULT = 64u * 1024u;

struct CwtKernelArgs {
    const float* values;     // (B, S)
    const int32_t* counts;   // (B) or null
    float* original;         // (B, S) or null
    float* signal;           // (B, S) or null
    float* spectrogram;      // (B, S, n_scales) or null
    float* mean_std;         // (B, 2) or null
    int S, n_scales;
    double width[CWT_MAX_SCALES];  // 2^(i + 1) tau
    double amp[CWT_MAX_SCALES];    // 2 / (sqrt(3 w) pi^(1/4))
    double gain[CWT_MAX_SCALES];   // (i + 2.5)^(-5/2)
};

// the sum of one double per thread over the workgroup: a binary tree over the thread index, the same bits in every thread
__device__ __forceinline__ double cwt_tree_sum(double v, double* __restrict__ red, int tid) {
    __syncthreads();
    red[tid] = v;
    for (int o = CWT_THREADS / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) red[tid] += red[tid + o];
    }
    __syncthreads();
    return red[0];
}

__global__ __launch_bounds__(CWT_THREADS) void cwt_decompose_kernel(const CwtKernelArgs a) {
    extern __shared__ double cwt_lds[];
    const int b = blockIdx.y, tid = threadIdx.x, S = a.S, ns = a.n_scales;
    const int k0 = blockIdx.x * CWT_TILE, k1 = k0 + CWT_TILE < S ? k0 + CWT_TILE : S;  // this tile's outputs [k0, k1)
    int n = a.counts ? a.counts[b] : S;
    n = n < 0 ? 0 : (n > S ? S : n);
    if (n == 0) {  // numpy's mean of nothing; nothing else is written
        if (blockIdx.x == 0 && tid == 0 && a.mean_std) a.mean_std[2 * b] = a.mean_std[2 * b + 1] = __builtin_nanf("");
        return;
    }
    const size_t row = (size_t)b * S;
    // ---- entries at or past the count: zeros
    for (int k = (k0 > n ? k0 : n) + tid; k < k1; k += CWT_THREADS) {
        if (a.original) a.original[row + k] = 0.0f;
        if (a.signal) a.signal[row + k] = 0.0f;
        if (a.spectrogram)
            for (int i = 0; i < ns; ++i) a.spectrogram[(row + k) * ns + i] = 0.0f;
    }
    if (k0 >= n) return;
    double* __restrict__ xs = cwt_lds;                     // CWT_TILE zeros, x[0 .. n), CWT_TILE zeros
    double* __restrict__ rs = cwt_lds + S + 2 * CWT_TILE;  // the wavelet of the scale at hand: M <= n values
    double* __restrict__ red = rs + S;                     // CWT_THREADS partials
    // ---- 1. original, signal, mean, std.  Thread t owns the entries j = t, t + 256, ... through step 2.
    double part = 0.0;
    for (int j = tid; j < n; j += CWT_THREADS) {
        const float v = a.values[row + j];
        const float o = v == 0.0f ? 1e-7f : v;
        const float s = (float)log((double)o);
        xs[CWT_TILE + j] = (double)s;
        part += (double)s;
        if (j >= k0 && j < k1) {
            if (a.original) a.original[row + j] = o;
            if (a.signal) a.signal[row + j] = s;
        }
    }
    const double mean = cwt_tree_sum(part, red, tid) / (double)n;
    part = 0.0;
    for (int j = tid; j < n; j += CWT_THREADS) {
        const double d = xs[CWT_TILE + j] - mean;
        part += d * d;
    }
    const double stdev = sqrt(cwt_tree_sum(part, red, tid) / (double)n);
    const float mean_f = (float)mean, std_f = (float)stdev;
    if (blockIdx.x == 0 && tid == 0 && a.mean_std) a.mean_std[2 * b] = mean_f, a.mean_std[2 * b + 1] = std_f;
    if (!a.spectrogram) return;
    // ---- 2. the normalised signal, fp32 arithmetic on fp32 operands
    const float den = __fadd_rn(std_f, 1e-7f);
    for (int j = tid; j < n; j += CWT_THREADS) xs[CWT_TILE + j] = (double)__fdiv_rn(__fsub_rn((float)xs[CWT_TILE + j], mean_f), den);
    for (int j = tid; j < CWT_TILE; j += CWT_THREADS) xs[j] = 0.0, xs[CWT_TILE + n + j] = 0.0;
    // ---- 3. the scales
    const int klast = (k1 < n ? k1 : n) - 1;  // the tile's last output below the count
    const int ka = k0 + tid, kb = ka + CWT_THREADS;
    for (int i = 0; i < ns; ++i) {
        const double w = a.width[i], amp = a.amp[i];
        const double N = fmin(10.0 * w, (double)n);  // a real number: an integer only when n truncates it
        const int M = (int)ceil(N), h = M / 2;
        const double centre = (N - 1.0) / 2.0, wsq = w * w;
        __syncthreads();  // the last scale's taps are read, x is written
        for (int m = tid; m < M; m += CWT_THREADS) {
            const double v = (double)m - centre, xsq = v * v;
            rs[m] = amp * (1.0 - xsq / wsq) * exp(-xsq / (2.0 * wsq));
        }
        __syncthreads();
        // taps any output of the tile has: 0 <= k - h + m < n for some k in [k0, klast]
        const int m_lo = h - klast > 0 ? h - klast : 0, m_hi = n + h - k0 < M ? n + h - k0 : M;
        const double* __restrict__ xa = xs + CWT_TILE + ka - h;  // indices: > CWT_TILE - (klast - k0) - 1 >= 0, < 2 CWT_TILE + n
        double acc_a = 0.0, acc_b = 0.0;
        int m = m_lo;
        for (; m + CWT_AHEAD <= m_hi; m += CWT_AHEAD) {  // the LDS reads of eight taps in flight before their multiply-adds, in tap order
            double r[CWT_AHEAD], va[CWT_AHEAD], vb[CWT_AHEAD];
#pragma unroll
            for (int u = 0; u < CWT_AHEAD; ++u) r[u] = rs[m + u], va[u] = xa[m + u], vb[u] = xa[m + u + CWT_THREADS];
#pragma unroll
            for (int u = 0; u < CWT_AHEAD; ++u) {
                acc_a = __builtin_fma(va[u], r[u], acc_a);
                acc_b = __builtin_fma(vb[u], r[u], acc_b);
            }
        }
        for (; m < m_hi; ++m) {
            const double r = rs[m];
            acc_a = __builtin_fma(xa[m], r, acc_a);
            acc_b = __builtin_fma(xa[m + CWT_THREADS], r, acc_b);
        }
        if (ka < n) a.spectrogram[(row + ka) * ns + i] = (float)(acc_a * a.gain[i]);
        if (kb < n && kb < k1) a.spectrogram[(row + kb) * ns + i] = (float)(acc_b * a.gain[i]);
    }
}

extern "C" {

int fs2_op_cwt_decompose(const float* values, const int32_t* counts, int32_t B, int32_t S, int32_t n_scales, double tau, float* original,
                         float* signal, float* spectrogram, float* mean_std, void* hip_stream) {
    if (!values || B < 1 || S < 1) return FS2_ERR_ARG;
    if (n_scales < 1 || n_scales > CWT_MAX_SCALES || !(tau >= 1e-100 && tau <= 1e100)) return FS2_ERR_ARG;  // (w^2 stays a normal number)
    if (S > CWT_MAX_S || B > 65535) return FS2_ERR_SHAPE;
    CwtKernelArgs a{values, counts, original, signal, spectrogram, mean_std, S, n_scales, {}, {}, {}};
    for (int i = 1; i <= n_scales; ++i) {
        const double w = ldexp(tau, i + 1);
        a.width[i - 1] = w;
        a.amp[i - 1] = 2.0 / (sqrt(3.0 * w) * pow(M_PI, 0.25));
        a.gain[i - 1] = pow((double)i + 2.5, -2.5);
    }
    const size_t lds = ((size_t)2 * S + 2 * CWT_TILE + CWT_THREADS) * sizeof(double);
    if (lds > CWT_LDS_DEFAULT &&
        hipFuncSetAttribute((const void*)cwt_decompose_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return FS2_ERR_HIP;
    hipLaunchKernelGGL(cwt_decompose_kernel, dim3((S + CWT_TILE - 1) / CWT_TILE, B), dim3(CWT_THREADS), lds, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

}  // extern "C"

}  // namespace fs2
