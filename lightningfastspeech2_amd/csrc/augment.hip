// Augmentation of the packed waveform on the device (include/fs2.h "Waveform augmentation", DESIGN.md "Augmentation"): rational
// resampling, convolution with a caller-supplied impulse response, Gaussian noise at a target SNR - the operations the reference's
// SpeechGenerator applies on the host per utterance (generate.py:82-104, generator.py:181,197-201), restated from their definitions.
// All three work on the layout fs2_op_wav_pack writes: utterance b's n_b = offsets[b + 1] - offsets[b] samples back to back.
//
// The two heavy operations are one framed GEMM (aug_framed_kernel):
//     out[i * P_out + j] = sum_q A[j][q] * span[i * stride + q - lead],   i = frame of the utterance, j < P_out
// run as exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: fp32 products, fp32 accumulate), rows = 32 frames, columns = 32 values of j.
//   table mode    (resampler)  A = tab (P_out = new rows of K), read through the caches like a weight; stride = orig, lead = width.
//                 One workgroup = 32 * RT frames of one utterance; its waves share out the (row tile, column tile) pairs.
//   Toeplitz mode (response)   A[j][q] = h[j + R - 1 - q], read from a zero-padded copy of h in LDS; P_out = stride = 32, lead = R - 1,
//                 K = R + 31.  One workgroup = AUG_CONV_TILE = 4096 consecutive outputs = 128 frames, a row tile per wave.
// The sample span the workgroup's frames cover goes into LDS once, zero outside the utterance's own [0, n_b): a neighbour's samples
// and whatever lies past offsets[B] are never read.  The Hankel operand "frame i, sample q" = span[i * stride + q] has a lane stride
// of `stride` words: with stride = 2^a m (m odd) and a >= 2, one pad word goes in after every 2^a samples (address s + (s >> a)), so
// that the lane stride becomes stride + m, odd: the 32 lanes of a ds_read_b32 group hit 32 banks.  An odd stride needs no pad; a = 1
// is left at its two-way conflict (the pad would cost half the span again).  The other operand is contiguous over the lanes.
// The sum over q runs in chunks of 8 in ascending q, even chunks into one accumulator and odd chunks into a second, added at the end:
// the order depends on (K, the position in the tile) only, never on B, an utterance's offset or its alignment - results are bitwise
// batch-invariant.  Tiles are counted from the utterance's own first sample.
//
// Noise: rms over the utterance in fp64 (a workgroup per 8192-sample chunk: lane-owned samples in order, shuffle tree, waves in
// order; then the chunk sums of an utterance in a fixed tree), scale = (float)(rms / 10^(snr / 20)) in fp64, y = x + scale * z as one
// rounded multiply and one rounded add.
#include "fs2_common.h"
#include "fs2_kernels.h"

namespace fs2 {

static constexpr int AUG_THREADS = 256;
static constexpr int AUG_WAVES = AUG_THREADS / 64;
static constexpr int AUG_CONV_TILE = 4096;            // outputs one workgroup owns in Toeplitz mode: 4 waves x 32 frames x 32
static constexpr int AUG_HPAD = 48;                   // zeros in front of the response's LDS copy (q runs to K rounded up to 16)
static constexpr size_t AUG_LDS_LIMIT = 160u * 1024u; // gfx950: 160 KiB per CU
static constexpr int AUG_MAX_RIR = 16384;
static constexpr int AUG_MAX_NEW = 640, AUG_MAX_K = 1024;
static constexpr long long AUG_MAX_LEN = 1LL << 30;   // samples of one utterance: positions inside a tile are ints
static constexpr int AUG_NOISE_CHUNK = 8192;          // samples per first-level partial

enum { AUG_OFF_RESAMPLE = 0, AUG_OFF_CONV = 1 };

struct AugFramedArgs {
    const float* in;
    const long long* in_off;
    float* out;
    const long long* out_off;
    const float* tab;          // table mode: (P_out, K); Toeplitz mode: the bank (n_rir, R_max)
    const int32_t* rir_len;    // Toeplitz mode
    const int32_t* rir_index;  // Toeplitz mode
    long long max_len;
    int P_out, stride, lead, K;  // table mode (Toeplitz mode derives them from R)
    int RT, NT;                  // 32-frame row tiles per workgroup, 32-wide column tiles of P_out
    int psh;                     // pad word after every 2^psh samples of the span (31: none)
    int R_max, n_rir;
};

__device__ __forceinline__ long long aug_len(const long long* off, int b, long long max_len) {
    const long long n = off[b + 1] - off[b];
    return n < 0 ? 0 : (n > max_len ? max_len : n);
}
// the response of utterance b: its row of the bank, or -1 (copy) for an index outside it
__device__ __forceinline__ int aug_rir(const int32_t* rir_index, int b, int n_rir) {
    const int i = rir_index[b];
    return (i < 0 || i >= n_rir) ? -1 : i;
}
__device__ __forceinline__ int aug_rir_len(const int32_t* rir_len, int idx, int R_max) {
    const int r = rir_len[idx];
    return r < 1 ? 1 : (r > R_max ? R_max : r);
}

// out_off[b] = sum of the output lengths in front of utterance b, out_off[B] = their total.  One workgroup: B is a batch size.
__global__ __launch_bounds__(AUG_THREADS) void aug_offsets_kernel(const long long* __restrict__ in_off, long long* __restrict__ out_off,
                                                                  int B, long long max_len, int kind, int p0, int p1,
                                                                  const int32_t* __restrict__ rir_len,
                                                                  const int32_t* __restrict__ rir_index, int n_rir, int R_max) {
    __shared__ long long ms[AUG_THREADS];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int c = 0; c < B; c += AUG_THREADS) {
        const int b = c + tid;
        long long m = 0;
        if (b < B) {
            const long long n = aug_len(in_off, b, max_len);
            if (kind == AUG_OFF_RESAMPLE) {
                m = ((long long)p1 * n + p0 - 1) / p0;  // ceil(new * n / orig), p0 = orig, p1 = new
            } else {
                m = n;
                if (p0 == FS2_CONV_FULL && n > 0) {
                    const int idx = aug_rir(rir_index, b, n_rir);
                    if (idx >= 0) m = n + aug_rir_len(rir_len, idx, R_max) - 1;
                }
            }
        }
        ms[tid] = m;
        __syncthreads();
        long long before = carry, all = carry;
        for (int u = 0; u < AUG_THREADS; ++u) {
            if (u == tid) before = all;
            all += ms[u];
        }
        if (b < B) out_off[b] = before;
        carry = all;
        __syncthreads();
    }
    if (tid == 0) out_off[B] = carry;
}

template <bool TOEP>
__global__ __launch_bounds__(AUG_THREADS) void aug_framed_kernel(const AugFramedArgs a) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y;
    const long long n = aug_len(a.in_off, b, a.max_len);
    const long long oo = a.out_off[b], m = a.out_off[b + 1] - oo;
    const float* __restrict__ x = a.in + a.in_off[b];
    float* __restrict__ y = a.out + oo;
    const int P = TOEP ? 32 : a.P_out, stride = TOEP ? 32 : a.stride;
    const int frames = 32 * a.RT;
    const long long f0 = (long long)blockIdx.x * frames;  // the workgroup's first frame, counted from the utterance's first sample
    const long long t0 = f0 * P;
    if (t0 >= m) return;  // uniform: a tile past the utterance's last output touches nothing
    int K = a.K, lead = a.lead, R = 0;
    const float* __restrict__ h = nullptr;
    if constexpr (TOEP) {
        const int idx = aug_rir(a.rir_index, b, a.n_rir);
        if (idx < 0) {  // no response: the utterance's own bits
            const long long end = t0 + AUG_CONV_TILE < m ? t0 + AUG_CONV_TILE : m;
            for (long long t = t0 + tid; t < end; t += AUG_THREADS) y[t] = x[t];
            return;
        }
        R = aug_rir_len(a.rir_len, idx, a.R_max);
        h = a.tab + (size_t)idx * a.R_max;
        K = R + 31;
        lead = R - 1;
    }
    const int Kp = (K + 15) & ~15;
    // ---- the span (and the response) -> LDS
    const int hp_words = TOEP ? a.R_max + 2 * AUG_HPAD : 0;
    float* __restrict__ sp = smem + hp_words;
    {
        const int L = (frames - 1) * stride + Kp;
        const long long g0 = f0 * stride - lead;
        for (int s = tid; s < L; s += AUG_THREADS) {
            const long long g = g0 + s;
            sp[s + (s >> a.psh)] = (g >= 0 && g < n) ? x[g] : 0.0f;
        }
        if constexpr (TOEP) {
            const int hl = R + 2 * AUG_HPAD;  // hp[u] = h[u - AUG_HPAD], zero outside [0, R): every q of the padded K finds a word
            for (int u = tid; u < hl; u += AUG_THREADS) {
                const int k = u - AUG_HPAD;
                smem[u] = (k >= 0 && k < R) ? h[k] : 0.0f;
            }
        }
    }
    __syncthreads();
    // ---- (row tile, column tile) pairs, wave by wave
    const int items = a.RT * a.NT;
    for (int item = wave; item < items; item += AUG_WAVES) {
        const int rt = item / a.NT, ct = item - rt * a.NT;
        const int fbase = (rt * 32 + li) * stride + hi * 4;  // this lane's frame, its four samples of chunk 0
        const int p = ct * 32 + li;                          // this lane's column
        const float* __restrict__ trow = a.tab + (size_t)(p < P ? p : 0) * K;
        const int hb = li + R - 1 + AUG_HPAD - hi * 4;       // Toeplitz: hp index of (j = li, q = hi * 4)
        auto load = [&](int kc, float (&av)[4], float (&bv)[4]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int s = fbase + kc * 8 + e;
                av[e] = sp[s + (s >> a.psh)];
                if constexpr (TOEP) {
                    bv[e] = smem[hb - kc * 8 - e];
                } else {
                    const int q = kc * 8 + hi * 4 + e;
                    bv[e] = (p < P && q < K) ? trow[q] : 0.0f;
                }
            }
        };
        f32x16_t acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
        const int KC = Kp / 8;  // even
        float a0[4], b0[4], a1[4], b1[4];
        load(0, a0, b0);
        load(1, a1, b1);
        for (int kc = 0; kc < KC; kc += 2) {
            // the next two chunks' operands are in flight under these chunks' MFMAs
            const int nx = kc + 2 < KC ? kc + 2 : kc;
            float na0[4], nb0[4], na1[4], nb1[4];
            load(nx, na0, nb0);
            load(nx + 1, na1, nb1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b0[e], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b1[e], acc1, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0[e] = na0[e];
                b0[e] = nb0[e];
                a1[e] = na1[e];
                b1[e] = nb1[e];
            }
        }
        // C layout: register r = frame (r & 3) + 8 (r >> 2) + 4 hi of the row tile, lane li = column
        if (p < P) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const long long t = (f0 + row) * P + p;
                if (t < m) y[t] = acc0[r] + acc1[r];
            }
        }
    }
}

// ---- noise
// partial[b][c] = sum of x^2 over chunk c of utterance b in fp64: thread t owns samples 4 t + 1024 k + e (e < 4, k < 8) of the chunk
// and adds them in that order; one 16-byte load where the address allows it, four 4-byte loads of the same samples where not.  Then
// a shuffle tree and the four waves in order.  A chunk past the utterance's end is 0.
__global__ __launch_bounds__(AUG_THREADS) void aug_sumsq_kernel(const float* __restrict__ in, const long long* __restrict__ off,
                                                                long long max_len, double* __restrict__ partial, int chunks) {
    __shared__ double red[AUG_WAVES];
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const long long n = aug_len(off, b, max_len);
    const float* __restrict__ x = in + off[b];
    const long long c0 = (long long)c * AUG_NOISE_CHUNK;
    double acc = 0.0;
    if (c0 < n) {
        const bool wide = (((uintptr_t)(x + c0)) & 15) == 0;
        for (int k = 0; k < AUG_NOISE_CHUNK / (4 * AUG_THREADS); ++k) {
            const long long i = c0 + (long long)k * 4 * AUG_THREADS + tid * 4;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (i + 4 <= n && wide) {
                const float4 q = *reinterpret_cast<const float4*>(x + i);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i + e < n) v[e] = x[i + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
        }
    }
    for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[(size_t)b * chunks + c] = ((red[0] + red[1]) + red[2]) + red[3];
}

// scale[b] = (float)(sqrt(sum / n) / 10^(snr / 20)) in fp64; thread t adds partials t, t + 256, ... in order, then a shuffle tree
// and the waves in order: chunks past the utterance's end add exact zeros, so the order depends on the utterance's chunks only.
__global__ __launch_bounds__(AUG_THREADS) void aug_scale_kernel(const double* __restrict__ partial, int chunks,
                                                                const long long* __restrict__ off, long long max_len,
                                                                const float* __restrict__ snr, float* __restrict__ scales) {
    __shared__ double red[AUG_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    double acc = 0.0;
    for (int c = tid; c < chunks; c += AUG_THREADS) acc += partial[(size_t)b * chunks + c];
    for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const long long n = aug_len(off, b, max_len);
        const double sum = ((red[0] + red[1]) + red[2]) + red[3];
        const float s = snr[b];
        float sc = 0.0f;
        if (n > 0 && !(s == INFINITY)) sc = (float)(sqrt(sum / (double)n) / pow(10.0, (double)s / 20.0));
        scales[b] = sc;
    }
}

// x + sc * z as a rounded product and a rounded sum: contraction into one fused multiply-add is switched off for these two operations
__device__ __forceinline__ float aug_axpy(float x, float sc, float z) {
#pragma clang fp contract(off)
    const float p = sc * z;
    return x + p;
}

// y = x + scale_b * z: one rounded multiply, one rounded add (no contraction); snr = +inf leaves the utterance's bits as they are
__global__ __launch_bounds__(AUG_THREADS) void aug_noise_kernel(const float* in, const long long* __restrict__ off,
                                                                long long max_len, const float* __restrict__ zbuf,
                                                                const float* __restrict__ snr, const float* __restrict__ scales,
                                                                float* out) {  // out may be in
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long n = aug_len(off, b, max_len), o = off[b];
    const float* x = in + o;
    const float* __restrict__ z = zbuf + o;
    float* y = out + o;
    const bool keep = snr[b] == INFINITY;
    if (keep && x == y) return;
    const float sc = scales[b];
    const bool wide = ((((uintptr_t)x) | ((uintptr_t)z) | ((uintptr_t)y)) & 15) == 0;
    for (long long c0 = (long long)blockIdx.x * (4 * AUG_THREADS); c0 < n; c0 += (long long)gridDim.x * (4 * AUG_THREADS)) {
        const long long i = c0 + tid * 4;
        if (wide && c0 + 4 * AUG_THREADS <= n) {
            const float4 xv = *reinterpret_cast<const float4*>(x + i);
            float4 r = xv;
            if (!keep) {
                const float4 zv = *reinterpret_cast<const float4*>(z + i);
                r.x = aug_axpy(xv.x, sc, zv.x);
                r.y = aug_axpy(xv.y, sc, zv.y);
                r.z = aug_axpy(xv.z, sc, zv.z);
                r.w = aug_axpy(xv.w, sc, zv.w);
            }
            *reinterpret_cast<float4*>(y + i) = r;
        } else {
            for (int e = 0; e < 4; ++e)
                if (i + e < n) y[i + e] = keep ? x[i + e] : aug_axpy(x[i + e], sc, z[i + e]);
        }
    }
}

// ---- launchers: every argument or shape error is answered before the first device call
static int aug_pad_shift(int stride) {
    int a = 0;
    while (!((stride >> a) & 1)) ++a;
    return a >= 2 ? a : 31;
}
static size_t aug_span_words(int frames, int stride, int Kp, int psh) {
    const size_t L = (size_t)(frames - 1) * stride + Kp;
    return L + (L >> psh) + 1;
}
// table mode: the most 32-frame row tiles (16 at most) whose span stays within 64 KiB (several workgroups per CU); one at least
static int aug_resample_row_tiles(int orig, int Kp, int psh) {
    int RT = 16;
    while (RT > 1 && aug_span_words(32 * RT, orig, Kp, psh) > 16384) RT >>= 1;
    return RT;
}
template <bool TOEP>
static int aug_reserve_lds(size_t lds) {
    static size_t attr = 64 * 1024;
    if (lds > attr) {
        if (hipFuncSetAttribute((const void*)aug_framed_kernel<TOEP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)AUG_LDS_LIMIT) != hipSuccess)
            return FS2_ERR_HIP;
        attr = AUG_LDS_LIMIT;
    }
    return FS2_OK;
}
static bool aug_bad_batch(int B, long long max_len, int* status) {
    if (B <= 0 || max_len < 0) return *status = FS2_ERR_ARG, true;
    if (B > 65535 || max_len > AUG_MAX_LEN) return *status = FS2_ERR_SHAPE, true;
    return false;
}

int launch_wav_resample(const float* in, const int64_t* in_off, int B, long long max_len, const float* tab, int orig, int nw,
                        int width, float* out, long long capacity, int64_t* out_off, hipStream_t st) {
    int status;
    if (!in || !in_off || !tab || !out || !out_off || orig <= 0 || nw <= 0 || width < 0) return FS2_ERR_ARG;
    if (aug_bad_batch(B, max_len, &status)) return status;
    const long long K = 2LL * width + orig;
    if (nw > AUG_MAX_NEW || K > AUG_MAX_K) return FS2_ERR_SHAPE;
    const long long m_max = ((long long)nw * max_len + orig - 1) / orig;
    if (capacity < 0 || (m_max > 0 && capacity / m_max < B)) return FS2_ERR_ARG;
    const int Kp = ((int)K + 15) & ~15, psh = aug_pad_shift(orig);
    const int RT = aug_resample_row_tiles(orig, Kp, psh);
    const size_t lds = aug_span_words(32 * RT, orig, Kp, psh) * sizeof(float);
    if (lds > AUG_LDS_LIMIT) return FS2_ERR_SHAPE;
    const long long frames = (m_max + nw - 1) / nw, tiles = (frames + 32 * RT - 1) / (32 * RT);
    if (tiles > 0x7fffffffLL) return FS2_ERR_SHAPE;
    if ((status = aug_reserve_lds<false>(lds)) != FS2_OK) return status;
    hipLaunchKernelGGL(aug_offsets_kernel, dim3(1), dim3(AUG_THREADS), 0, st, (const long long*)in_off, (long long*)out_off, B, max_len,
                       (int)AUG_OFF_RESAMPLE, orig, nw, (const int32_t*)nullptr, (const int32_t*)nullptr, 0, 0);
    if (tiles > 0) {
        AugFramedArgs a{in, (const long long*)in_off, out, (const long long*)out_off, tab, nullptr, nullptr, max_len,
                        nw, orig, width, (int)K, RT, (nw + 31) / 32, psh, 0, 0};
        hipLaunchKernelGGL(aug_framed_kernel<false>, dim3((unsigned)tiles, (unsigned)B), dim3(AUG_THREADS), lds, st, a);
    }
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

int launch_wav_convolve(const float* in, const int64_t* in_off, int B, long long max_len, const float* rir, const int32_t* rir_len,
                        const int32_t* rir_index, int n_rir, int R_max, int mode, float* out, long long capacity, int64_t* out_off,
                        hipStream_t st) {
    int status;
    if (!in || !in_off || !rir || !rir_len || !rir_index || !out || !out_off || n_rir <= 0 || R_max <= 0) return FS2_ERR_ARG;
    if (mode != FS2_CONV_SAME && mode != FS2_CONV_FULL) return FS2_ERR_ARG;
    if (aug_bad_batch(B, max_len, &status)) return status;
    if (R_max > AUG_MAX_RIR) return FS2_ERR_SHAPE;
    const long long m_max = (mode == FS2_CONV_FULL && max_len > 0) ? max_len + R_max - 1 : max_len;
    if (capacity < 0 || (m_max > 0 && capacity / m_max < B)) return FS2_ERR_ARG;
    const int Kp = (R_max + 31 + 15) & ~15;
    const size_t lds = ((size_t)R_max + 2 * AUG_HPAD + aug_span_words(AUG_CONV_TILE / 32, 32, Kp, 5)) * sizeof(float);
    if (lds > AUG_LDS_LIMIT) return FS2_ERR_SHAPE;
    const long long tiles = (m_max + AUG_CONV_TILE - 1) / AUG_CONV_TILE;
    if ((status = aug_reserve_lds<true>(lds)) != FS2_OK) return status;
    hipLaunchKernelGGL(aug_offsets_kernel, dim3(1), dim3(AUG_THREADS), 0, st, (const long long*)in_off, (long long*)out_off, B, max_len,
                       (int)AUG_OFF_CONV, mode, 0, rir_len, rir_index, n_rir, R_max);
    if (tiles > 0) {
        AugFramedArgs a{in, (const long long*)in_off, out, (const long long*)out_off, rir, rir_len, rir_index, max_len,
                        32, 32, 0, 0, AUG_CONV_TILE / 1024, 1, 5, R_max, n_rir};
        hipLaunchKernelGGL(aug_framed_kernel<true>, dim3((unsigned)tiles, (unsigned)B), dim3(AUG_THREADS), lds, st, a);
    }
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

int wav_convolve_tile() { return AUG_CONV_TILE; }
int wav_resample_tile(int orig, int nw, int width) {
    if (orig <= 0 || nw <= 0 || width < 0 || nw > AUG_MAX_NEW || 2LL * width + orig > AUG_MAX_K) return 0;
    const int Kp = (2 * width + orig + 15) & ~15;
    return 32 * aug_resample_row_tiles(orig, Kp, aug_pad_shift(orig)) * orig;
}

static long long aug_noise_chunks(long long max_len) {
    const long long c = (max_len + AUG_NOISE_CHUNK - 1) / AUG_NOISE_CHUNK;
    return c > 0 ? c : 1;
}
size_t wav_add_noise_ws_bytes(int B, long long max_len) {
    if (B <= 0 || max_len < 0 || max_len > AUG_MAX_LEN) return 0;
    return (size_t)B * (size_t)aug_noise_chunks(max_len) * sizeof(double);
}

int launch_wav_add_noise(const float* in, const int64_t* off, int B, long long max_len, const float* z, const float* snr, void* ws,
                         size_t ws_bytes, float* out, float* scales_out, hipStream_t st) {
    int status;
    if (!in || !off || !z || !snr || !ws || !out || !scales_out || (((uintptr_t)ws) & 7)) return FS2_ERR_ARG;
    if (aug_bad_batch(B, max_len, &status)) return status;
    if (ws_bytes < wav_add_noise_ws_bytes(B, max_len)) return FS2_ERR_NOMEM;
    const int chunks = (int)aug_noise_chunks(max_len);
    hipLaunchKernelGGL(aug_sumsq_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(AUG_THREADS), 0, st, in, (const long long*)off, max_len,
                       (double*)ws, chunks);
    hipLaunchKernelGGL(aug_scale_kernel, dim3((unsigned)B), dim3(AUG_THREADS), 0, st, (const double*)ws, chunks, (const long long*)off,
                       max_len, snr, scales_out);
    if (max_len > 0) {
        long long gx = (max_len + 4 * AUG_THREADS - 1) / (4 * AUG_THREADS);
        const long long cap = (4096 + B - 1) / B;  // ~16 workgroups per CU over the batch, the rest by stride
        if (gx > cap) gx = cap;
        hipLaunchKernelGGL(aug_noise_kernel, dim3((unsigned)gx, (unsigned)B), dim3(AUG_THREADS), 0, st, in, (const long long*)off, max_len,
                           z, snr, (const float*)scales_out, out);
    }
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

}  // namespace fs2
