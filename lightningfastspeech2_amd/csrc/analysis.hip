// Analysis front end: waveform -> log-mel spectrogram and frame energy on the device (DESIGN.md "Analysis front end").
// What TTSDataset.__getitem__ / _create_variances compute on the CPU with torchaudio and librosa (litfass/dataset/datasets.py:
// 183-199, 369-380, 600-618, 630-648), restated from the semantics: a centred Hann STFT magnitude times a mel basis, clamp, log;
// the RMS of un-centred windows; the phone-level mean of a frame-level variance.
//
// The heavy launch (mel_stft_kernel): one workgroup = one utterance x TM consecutive frames.
//   1. The one contiguous sample span those frames cover, (TM - 1) * hop + n_fft samples, goes into LDS once, scaled by the peak
//      factor, zero outside [0, n) - samples at or past the utterance's length are never read.  Layout: rows of `hop` samples with one
//      pad word per row (address s + s / hop), so that the A operand "frame i, sample k" = span[i * hop + k], whose lane stride is hop
//      words, lands on bank i + const instead of one bank (hop is a power of two: hop + 1 is odd, every stride is conflict-free).
//   2. The real DFT is an fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate) of the frames against a table
//      of window[k] * cos / window[k] * sin built in float64 at create and rounded once.  Only the bins the basis weighs are columns.
//      A wave owns 32 bins at a time and holds their real and imaginary accumulators for all TM frames: the C layout gives a lane
//      column j = lane & 31 in both, so |X| is formed in registers.
//   3. |X| of the wave's 32 bins goes through a per-wave LDS stage (C layout -> A layout) into a second small MFMA GEMM against the
//      basis columns of those bins; the mel accumulators stay in registers across the wave's bin tiles.
//   4. The four waves' partial mels are added in wave order in LDS (the span is dead by then), clamped, logged and stored for rows
//      t < T_b; rows past the utterance's count are written as zeros.
// The order of every sum depends on (t mod TM, bin, mel) only, never on the batch: results are bitwise batch-invariant.
#include <math.h>

#include <new>
#include <vector>

#include "fs2_host.h"

namespace fs2 {

static constexpr int MEL_THREADS = 256;
static constexpr int MEL_WAVES = MEL_THREADS / 64;
static constexpr int MEL_STAGE_LD = 33;                // |X| stage row: 32 bins + 1 pad word
static constexpr size_t MEL_LDS_LIMIT = 160u * 1024u;  // gfx950: 160 KiB per CU

struct MelKernelArgs {
    const float* wav;         // (B, S)
    const int32_t* lengths;   // (B)
    const uint32_t* peak;     // (B) bits of max |x| (mel_peak_kernel) or null: scale 1
    const float4* table;      // [bin tile][k chunk][re, im][64 lanes] x 4 k-values
    const float4* btab;       // [bin tile][4 chunks of 8 bins][mel tile][64 lanes] x 4 bins
    float* mel;               // (B, T_max, n_mels)
    int32_t* mel_frames;      // (B)
    int32_t* energy_frames;   // (B) or null
    int S, T_max, n_fft, hop, lh /* log2 hop */, n_mels, nbt /* bin tiles */, tm /* frames per workgroup */, log_kind;
    float clip;
};

__device__ __forceinline__ float mel_scale(const uint32_t* __restrict__ peak, int b) {
    if (!peak) return 1.0f;
    const float m = __uint_as_float(peak[b]);
    return m > 0.0f ? 1.0f / m : 1.0f;  // an all-zero utterance keeps scale 1 (the reference divides and gives NaN)
}

__device__ __forceinline__ int mel_len(const int32_t* __restrict__ lengths, int b, int S) {
    const int n = lengths[b];
    return n < 0 ? 0 : (n > S ? S : n);
}

// max |x| over each utterance's own samples -> peak[b] (bits of a non-negative float order as unsigned; zero-filled by the caller)
__global__ __launch_bounds__(256) void mel_peak_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lengths,
                                                      uint32_t* __restrict__ peak, int S) {
    const int b = blockIdx.y, n = mel_len(lengths, b, S);
    const float* __restrict__ x = wav + (size_t)b * S;
    // the samples in front of the row's first 16-byte boundary and behind its last one by 4-byte loads, the rest by 16-byte loads
    // (a maximum does not depend on the order)
    const int to_boundary = (int)((4 - ((reinterpret_cast<uintptr_t>(x) >> 2) & 3)) & 3);
    const int head = to_boundary < n ? to_boundary : n;
    const int nv = (n - head) >> 2, tail0 = head + 4 * nv;
    const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + head);
    float m = 0.0f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
        const float4 q = xv[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(q.x), fabsf(q.y))), fmaxf(fabsf(q.z), fabsf(q.w)));
    }
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < head) m = fmaxf(m, fabsf(x[threadIdx.x]));
        if (tail0 + (int)threadIdx.x < n) m = fmaxf(m, fabsf(x[tail0 + threadIdx.x]));  // at most three
    }
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_down(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(peak + b, __float_as_uint(m));
}

// e[t] = sqrt(sum_{j = t hop}^{min(t hop + win, n) - 1} (s x[j])^2 / win), one wave per frame; rows t >= ceil(n / hop) are zeros
__global__ __launch_bounds__(256) void mel_energy_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lengths,
                                                        const uint32_t* __restrict__ peak, float* __restrict__ energy, int S,
                                                        int Te_max, int hop, int win) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= Te_max) return;
    const int n = mel_len(lengths, b, S);
    const int te = (int)(((long long)n + hop - 1) / hop);
    float* __restrict__ dst = energy + (size_t)b * Te_max + t;
    if (t >= te) {
        if (lane == 0) *dst = 0.0f;
        return;
    }
    const float s = mel_scale(peak, b);
    const float* __restrict__ x = wav + (size_t)b * S;
    const long long lo = (long long)t * hop;
    const int cnt = (int)((lo + win < n ? lo + win : (long long)n) - lo);
    float acc = 0.0f;
    for (int j = lane; j < cnt; j += 64) {
        const float v = x[lo + j] * s;
        acc = fmaf(v, v, acc);
    }
    for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0) *dst = sqrtf(acc / (float)win);
}

// Orders a wave's LDS stores before its own later LDS loads (other lanes' words included): a fence at wavefront scope and a
// scheduling barrier for the compiler; the LDS serves one wave's instructions in order.
__device__ __forceinline__ void mel_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// MT = 32-row MFMA tiles per workgroup (frames per workgroup tm <= 32 * MT), NT = 32-column mel tiles
template <int MT, int NT>
__global__ __launch_bounds__(MEL_THREADS) void mel_stft_kernel(const MelKernelArgs a) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * a.tm;
    const int n = mel_len(a.lengths, b, a.S);
    const int Tb = n > 0 ? 1 + n / a.hop : 0;
    if (blockIdx.x == 0 && tid == 0) {
        a.mel_frames[b] = Tb;
        if (a.energy_frames) a.energy_frames[b] = (int)(((long long)n + a.hop - 1) / a.hop);
    }
    const int rows = a.T_max - t0 < a.tm ? a.T_max - t0 : a.tm;  // rows of this tile that exist in the output
    float* __restrict__ dst = a.mel + ((size_t)b * a.T_max + t0) * a.n_mels;
    if (t0 >= Tb) {  // uniform: a tile past the utterance's last frame is zeros
        for (int i = tid; i < rows * a.n_mels; i += MEL_THREADS) dst[i] = 0.0f;
        return;
    }
    // ---- 1. the sample span -> LDS (row of hop samples + 1 pad word)
    const int span = (a.tm - 1) * a.hop + a.n_fft;
    const int span_words = span + (span >> a.lh) + 1;
    const int out_ld = NT * 32 + 1;
    const int out_words = MT * 32 * out_ld;  // the cross-wave sum reuses the span's words
    float* __restrict__ stage = smem + (span_words > out_words ? span_words : out_words) + wave * (MT * 32 * MEL_STAGE_LD);
    {
        const float s = mel_scale(a.peak, b);
        const float* __restrict__ x = a.wav + (size_t)b * a.S;
        const long long g0 = (long long)t0 * a.hop - a.n_fft / 2;
        for (int i = tid; i < span; i += MEL_THREADS) {
            const long long g = g0 + i;
            smem[i + (i >> a.lh)] = (g >= 0 && g < n) ? x[g] * s : 0.0f;
        }
    }
    __syncthreads();
    // ---- 2 + 3. bin tile by bin tile: DFT GEMM, |X|, mel GEMM
    f32x16_t macc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) macc[mt][nt][r] = 0.0f;
    const int KC = a.n_fft / 8;
    int fbase[MT];  // first sample of this lane's frame in each row tile (clamped: rows past tm are computed and dropped)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int f = mt * 32 + li;
        fbase[mt] = (f < a.tm ? f : a.tm - 1) * a.hop + hi * 4;
    }
    const int rounds = (a.nbt + MEL_WAVES - 1) / MEL_WAVES;
    for (int rd = 0; rd < rounds; ++rd) {
        const int bt = rd * MEL_WAVES + wave;
        const bool live = bt < a.nbt;  // uniform per wave
        if (live) {
            f32x16_t re[MT], im[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) re[mt][r] = im[mt][r] = 0.0f;
            const float4* __restrict__ tb = a.table + (size_t)bt * KC * 128 + lane;
            // this lane's four samples of chunk kc in every row tile (four consecutive samples share a row when hop >= 4)
            auto load_a = [&](int kc, float (&av)[MT][4]) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int s0 = fbase[mt] + kc * 8;
                    if (a.lh >= 2) {
                        const float* p = smem + s0 + (s0 >> a.lh);
#pragma unroll
                        for (int e = 0; e < 4; ++e) av[mt][e] = p[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) av[mt][e] = smem[s0 + e + ((s0 + e) >> a.lh)];
                    }
                }
            };
            float4 bre = tb[0], bim = tb[64];
            float av[MT][4];
            load_a(0, av);
            for (int kc = 0; kc < KC; ++kc) {
                // the next chunk's table columns and samples are in flight under this chunk's MFMAs
                const int nx = kc + 1 < KC ? kc + 1 : kc;
                const float4 nre = tb[(size_t)nx * 128], nim = tb[(size_t)nx * 128 + 64];
                float nav[MT][4];
                load_a(nx, nav);
                const float br[4] = {bre.x, bre.y, bre.z, bre.w}, bi[4] = {bim.x, bim.y, bim.z, bim.w};
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        re[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][e], br[e], re[mt], 0, 0, 0);
                        im[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][e], bi[e], im[mt], 0, 0, 0);
                    }
                bre = nre;
                bim = nim;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[mt][e] = nav[mt][e];
            }
            // |X| in registers (one lane holds both parts of bin li), C layout -> this wave's stage
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    stage[row * MEL_STAGE_LD + li] = sqrtf(fmaf(re[mt][r], re[mt][r], im[mt][r] * im[mt][r]));
                }
        }
        mel_wave_sync();  // the stage is private to the wave: its own writes before its own reads, no workgroup barrier
        if (live) {
            const float4* __restrict__ bb = a.btab + (size_t)bt * 4 * NT * 64 + lane;
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                float av[MT][4];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[mt][e] = stage[(mt * 32 + li) * MEL_STAGE_LD + kc * 8 + hi * 4 + e];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float4 w = bb[(kc * NT + nt) * 64];
                    const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            macc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][e], wv[e], macc[mt][nt], 0, 0, 0);
                }
            }
        }
        mel_wave_sync();  // the stage is rewritten in the next round
    }
    __syncthreads();  // every wave is done with the span: it is dead from here
    // ---- 4. partial mels of the four waves, added in wave order
    for (int w = 0; w < MEL_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int idx = (mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) * out_ld + nt * 32 + li;
                        smem[idx] = w == 0 ? macc[mt][nt][r] : smem[idx] + macc[mt][nt][r];
                    }
        }
        __syncthreads();
    }
    for (int i = tid; i < rows * a.n_mels; i += MEL_THREADS) {
        const int t = i / a.n_mels, m = i - t * a.n_mels;
        float v = 0.0f;
        if (t0 + t < Tb) {
            // the logarithm in fp64 and rounded once: a few million values per call, and an fp32 log's own error would be the
            // largest term of the log-domain figure
            v = smem[t * out_ld + m];
            if (a.log_kind != FS2_MEL_LINEAR) {
                const double x = (double)fmaxf(v, a.clip);
                v = (float)(a.log_kind == FS2_MEL_LN ? log(x) : log10(x));
            }
        }
        dst[i] = v;
    }
}

// out[b][j] = (mean(values[b][pos_j : pos_j + d_j]) - mean) / std, segments clipped to the utterance's frames; empty -> empty_value
// Thread j adds the j durations in front of its phone itself: O(L^2) loads per row, fine for phone counts (hundreds), no scan launch.
__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ values, const int32_t* __restrict__ frames,
                                                          const int32_t* __restrict__ dur, float* __restrict__ out, int T, int L,
                                                          float empty_value, float mean, float stdev) {
    const int b = blockIdx.x;
    int F = frames ? frames[b] : T;
    F = F < 0 ? 0 : (F > T ? T : F);
    const int32_t* __restrict__ d = dur + (size_t)b * L;
    const float* __restrict__ v = values + (size_t)b * T;
    for (int j = threadIdx.x; j < L; j += 256) {
        long long pos = 0;
        for (int i = 0; i < j; ++i) pos += d[i] > 0 ? d[i] : 0;
        const long long end = pos + (d[j] > 0 ? d[j] : 0);
        const int lo = (int)(pos < F ? pos : F), hi = (int)(end < F ? end : F);
        float m = empty_value;
        if (hi > lo) {
            float s = 0.0f;
            for (int t = lo; t < hi; ++t) s += v[t];
            m = s / (float)(hi - lo);
        }
        out[(size_t)b * L + j] = (m - mean) / stdev;
    }
}

// ---- training targets: windowed WADA, contour finishing, masked row mean (include/fs2.h "Training targets from audio")
static constexpr int SNR_TILE = 32;        // windows one workgroup owns: the kernel's seams lie at multiples of 32 windows
static constexpr int SNR_MAX_TABLE = 512;  // table entries held in LDS
static constexpr float SNR_EPS = 1e-20f;

// the per-hop partials of one workgroup: sums in fp64, the two "anything there" flags as bits 0 (|x~| > 0) and 1 (fp32 x~^2 > 0)
__host__ __device__ inline size_t snr_lds_bytes(int partials, int K) {
    return (size_t)K * sizeof(double) + (size_t)partials * (2 * sizeof(double) + sizeof(int));
}

// Windowed WADA (Kim & Stern): out[t] = i* + (v3 - g[i*]) / (g[i* + 1] - g[i*]) with v3 = ln(mean a) - mean(ln a), a = max(|x~|, 1e-20)
// over window t = [t hop, min(t hop + win, n)), i* = max{i : g[i] < v3}.  One workgroup = one utterance x SNR_TILE consecutive
// windows.  Phase 1: the tile's hops and the win / hop - 1 after them are reduced once each, a wave per hop: lane l owns samples
// 4 l + 256 k + e (e < 4; one 16-byte load where the address allows it, four 4-byte loads of the same samples where not), adds its
// own in that order in fp64 (the terms |x~| and logf(a) are fp32), then a shuffle tree; the partials go to LDS.  Phase 2: a thread per
// window adds its win / hop consecutive partials in order, forms v3 in fp64 and looks it up in the table held in LDS.  A hop past
// the utterance's end has no samples; the last hops are short: a window's mean divides by the samples that exist.  No sum depends on
// the batch, on S or on the alignment of a row: results are bitwise batch-invariant.
__global__ __launch_bounds__(256) void mel_snr_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lengths,
                                                     const uint32_t* __restrict__ peak, const double* __restrict__ table, int K,
                                                     float* __restrict__ snr, int32_t* __restrict__ snr_frames, int S, int Te_max,
                                                     int hop, int win) {
    extern __shared__ double snr_smem[];
    const int r = win / hop, P = SNR_TILE + r - 1;
    double* __restrict__ g = snr_smem;      // [K]
    double* __restrict__ pa = g + K;        // [P] sum of a
    double* __restrict__ pl = pa + P;       // [P] sum of ln a
    int* __restrict__ pf = (int*)(pl + P);  // [P] flags
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * SNR_TILE;
    const int n = mel_len(lengths, b, S);
    const int te = (int)(((long long)n + hop - 1) / hop);
    if (blockIdx.x == 0 && tid == 0 && snr_frames) snr_frames[b] = te;
    const int rows = Te_max - t0 < SNR_TILE ? Te_max - t0 : SNR_TILE;
    float* __restrict__ dst = snr + (size_t)b * Te_max + t0;
    if (t0 >= te) {  // uniform: a tile past the utterance's last window is zeros
        for (int i = tid; i < rows; i += 256) dst[i] = 0.0f;
        return;
    }
    for (int i = tid; i < K; i += 256) g[i] = table[i];
    const float s = mel_scale(peak, b);
    const float* __restrict__ x = wav + (size_t)b * S;
    for (int h = wave; h < P; h += 4) {
        const long long lo = (long long)(t0 + h) * hop;
        const int cnt = lo >= n ? 0 : (int)((lo + hop < n ? lo + hop : (long long)n) - lo);
        const float* __restrict__ p = x + (lo < n ? lo : 0);
        const bool vec = (((uintptr_t)p) & 15) == 0;  // uniform per wave
        double sa = 0.0, sl = 0.0;
        int fl = 0;
        for (int j = lane * 4; j < cnt; j += 256) {
            float v[4];
            if (vec && j + 4 <= cnt) {
                const float4 q = *reinterpret_cast<const float4*>(p + j);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = j + e < cnt ? p[j + e] : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < cnt) {
                    const float xs = v[e] * s, m = fabsf(xs), a = m < SNR_EPS ? SNR_EPS : m;  // a NaN sample stays NaN
                    sa += (double)a;
                    sl += (double)logf(a);
                    fl |= (m > 0.0f ? 1 : 0) | (xs * xs > 0.0f ? 2 : 0);
                }
        }
        for (int o = 32; o; o >>= 1) {
            sa += __shfl_down(sa, o);
            sl += __shfl_down(sl, o);
            fl |= __shfl_down(fl, o);
        }
        if (lane == 0) pa[h] = sa, pl[h] = sl, pf[h] = fl;
    }
    __syncthreads();
    if (tid < rows) {
        const int t = t0 + tid;
        float out = 0.0f;
        if (t < te) {
            double sa = 0.0, sl = 0.0;
            int fl = 0;
            for (int i = 0; i < r; ++i) sa += pa[tid + i], sl += pl[tid + i], fl |= pf[tid + i];
            const long long lo = (long long)t * hop;
            const double cnt = (double)((lo + win < n ? lo + win : (long long)n) - lo);
            out = __builtin_nanf("");
            if (fl == 3) {
                const double mean_a = sa / cnt;
                const double v3 = log(mean_a > (double)SNR_EPS ? mean_a : (double)SNR_EPS) - sl / cnt;
                int i = K - 1;
                while (i >= 0 && !(g[i] < v3)) --i;  // the largest index below v3: the table need not be monotone
                if (i >= 0 && i < K - 1) {
                    const double o = (double)i + (v3 - g[i]) / (g[i + 1] - g[i]);
                    if (o < (double)(K - 1)) out = (float)o;
                }
            }
        }
        dst[tid] = out;
    }
}

static constexpr int FIN_MAX_T = 4096;  // frames of one utterance (the reference caps one at 2756)
static constexpr int FIN_MAX_L = 2048;  // phones of one utterance

// inclusive scan of one int per thread over the workgroup's 256 threads in the order of `pos` (a permutation of 0..255)
template <class Op>
__device__ __forceinline__ int fin_scan(int v, int pos, int* __restrict__ sc, Op op) {
    __syncthreads();
    sc[pos] = v;
    for (int o = 1; o < 256; o <<= 1) {
        __syncthreads();
        const int u = pos >= o ? sc[pos - o] : v;
        __syncthreads();
        if (pos >= o) sc[pos] = v = op(u, v);
    }
    __syncthreads();
    return v;
}

// Contour finishing (datasets.py:576-598, 831-837): one workgroup = one utterance.  The contour, the durations' prefix sums
// (saturated at T: only comparisons with t < F <= T are made), the frame flags and the nearest present frame to either side are in
// LDS.  A thread owns T / 256 (rounded up) consecutive frames; the nearest present frame on the left is an inclusive max-scan
// over the workgroup, the one on the right a min-scan from the other end.  The fill reads present frames only.
__global__ __launch_bounds__(256) void contour_finish_kernel(const float* __restrict__ values, const int32_t* __restrict__ frames,
                                                            const int32_t* __restrict__ dur, const int32_t* __restrict__ silent,
                                                            float* __restrict__ out, int32_t* __restrict__ frames_out,
                                                            float* __restrict__ prior, int T, int L, int zero_is_missing,
                                                            float all_missing_value, float mean, float stdev) {
    __shared__ float y[FIN_MAX_T];
    __shared__ int cum[FIN_MAX_L];
    __shared__ short left[FIN_MAX_T], right[FIN_MAX_T];
    __shared__ unsigned char flag[FIN_MAX_T];  // bit 0: missing, bit 1: frame of a silent phone
    __shared__ int sc[256];
    __shared__ double psum[256];
    __shared__ int pcnt[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t* __restrict__ d = dur + (size_t)b * L;
    const int32_t* __restrict__ sil = silent ? silent + (size_t)b * L : nullptr;
    const float* __restrict__ v = values + (size_t)b * T;
    auto sat_add = [T](int p, int q) { return p + q < T ? p + q : T; };  // both in [0, T]: no overflow
    // ---- prefix sums of the durations, each clamped to [0, T]
    const int cl = (L + 255) / 256, j0 = tid * cl, j1 = j0 + cl < L ? j0 + cl : L;
    int own = 0;
    for (int j = j0; j < j1; ++j) own = sat_add(own, d[j] < 0 ? 0 : (d[j] > T ? T : d[j]));
    fin_scan(own, tid, sc, sat_add);  // inclusive over the threads
    int run = tid ? sc[tid - 1] : 0;
    const int total = sc[255];
    for (int j = j0; j < j1; ++j) cum[j] = run = sat_add(run, d[j] < 0 ? 0 : (d[j] > T ? T : d[j]));
    int F = frames ? frames[b] : T;
    F = F < 0 ? 0 : (F > T ? T : F);
    F = total < F ? total : F;
    __syncthreads();
    // ---- this thread's frames: value, phone (first j with cum[j] > t), flags, nearest present frame on either side within the chunk
    const int ct = (T + 255) / 256, f0 = tid * ct, f1 = f0 + ct < F ? f0 + ct : F;
    int last = -1;
    for (int t = f0; t < f1; ++t) {
        int lo = 0, hi = L - 1;  // cum[L - 1] = total > t: the search ends on a phone of positive duration
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] > t) hi = mid; else lo = mid + 1;
        }
        const float x = v[t];
        const bool s = sil && sil[lo] != 0;
        const bool miss = s || isnan(x) || (zero_is_missing && x == 0.0f);
        y[t] = x;
        flag[t] = (unsigned char)((miss ? 1 : 0) | (s ? 2 : 0));
        if (!miss) last = t;
        left[t] = (short)last;  // -1: none in this chunk so far
    }
    int first = FIN_MAX_T;
    for (int t = f1 - 1; t >= f0; --t) {
        if (!(flag[t] & 1)) first = t;
        right[t] = (short)first;  // FIN_MAX_T: none in this chunk from here on
    }
    fin_scan(last, tid, sc, [](int p, int q) { return p > q ? p : q; });
    const int before = tid ? sc[tid - 1] : -1;  // nearest present frame in the chunks before this one
    const bool any = sc[255] >= 0;
    fin_scan(first, 255 - tid, sc, [](int p, int q) { return p < q ? p : q; });
    const int after = tid < 255 ? sc[254 - tid] : FIN_MAX_T;  // ... in the chunks after it
    // ---- the fill
    double ps = 0.0;
    int pc = 0;
    for (int t = f0; t < f1; ++t) {
        float o = y[t];
        if (!any) {
            o = all_missing_value;
        } else if (flag[t] & 1) {
            const int l = left[t] >= 0 ? left[t] : before, r = right[t] < FIN_MAX_T ? right[t] : after;
            if (l < 0) o = y[r];
            else if (r >= FIN_MAX_T) o = y[l];
            else o = (float)((double)y[l] + (double)(t - l) * ((double)y[r] - (double)y[l]) / (double)(r - l));
        }
        if (!(flag[t] & 2)) ps += (double)o, ++pc;
        out[(size_t)b * T + t] = (float)(((double)o - (double)mean) / (double)stdev);
    }
    for (int t = f0 > F ? f0 : F; t < (f0 + ct < T ? f0 + ct : T); ++t) out[(size_t)b * T + t] = 0.0f;  // the tail, from F on
    psum[tid] = ps, pcnt[tid] = pc;
    __syncthreads();
    if (tid == 0) {
        frames_out[b] = F;
        if (prior) {
            double sum = 0.0;
            long long c = 0;
            for (int i = 0; i < 256; ++i) sum += psum[i], c += pcnt[i];  // chunk sums in frame order
            prior[b] = c ? (float)(sum / (double)c) : __builtin_nanf("");
        }
    }
}

// out[b] = mean of values[b][j] over j < counts[b] with skip[b][j] == 0, NaN for none: chunks of consecutive entries summed in order
// in fp64, the chunk sums added in order
__global__ __launch_bounds__(256) void masked_row_mean_kernel(const float* __restrict__ values, const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ skip, float* __restrict__ out, int N) {
    __shared__ double psum[256];
    __shared__ int pcnt[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int c = counts ? counts[b] : N;
    c = c < 0 ? 0 : (c > N ? N : c);
    const int ch = (N + 255) / 256;
    const long long j0 = (long long)tid * ch;
    const long long j1 = j0 + ch < c ? j0 + ch : c;
    double s = 0.0;
    int k = 0;
    for (long long j = j0; j < j1; ++j)
        if (!skip || skip[(size_t)b * N + j] == 0) s += (double)values[(size_t)b * N + j], ++k;
    psum[tid] = s, pcnt[tid] = k;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        long long cnt = 0;
        for (int i = 0; i < 256; ++i) sum += psum[i], cnt += pcnt[i];
        out[b] = cnt ? (float)(sum / (double)cnt) : __builtin_nanf("");
    }
}

// ---- F0 tracking: YIN (include/fs2.h "F0 tracking"; DESIGN.md "F0 tracking on the device")
static constexpr int PITCH_MAX_LAGS = 1024;           // tau_max + 2 at the most
static constexpr size_t PITCH_LDS_TARGET = 64u * 1024u;  // at least two workgroups per CU where a tile fits this; no LDS reservation needed

struct PitchGeom {
    int blk, r;    // a frame is r blocks of blk samples, block h of a tile starting h * hop samples into its span
    int nl, lc;    // lags 0 .. nl - 1 = tau_max + 1; lag capacity: nl rounded up to 64 (a 16-lane group owns 64 lags)
    int tile, P;   // frames one workgroup owns; blocks it reduces = tile + r - 1
    int span;      // floats of the staged span, the slack behind the last lag's last sample included (a multiple of 4)
    size_t lds;
};

// W % hop == 0: per-hop partial sums, shared by the W / hop frames that overlap a hop.  Otherwise a frame is its own single block.
static PitchGeom pitch_geom(int win, int hop, int tau_max, int tile) {
    PitchGeom g;
    g.r = win % hop == 0 ? win / hop : 1;
    g.blk = win % hop == 0 ? hop : win;
    g.nl = tau_max + 2;
    g.lc = (g.nl + 63) & ~63;
    g.tile = tile;
    g.P = tile + g.r - 1;
    g.span = (g.P - 1) * hop + ((g.blk + 3) & ~3) + g.lc + 8;  // (+ 8: the window word and the word read one step ahead)
    g.lds = ((size_t)g.span + (size_t)g.P * g.lc + (size_t)MEL_WAVES * g.lc) * sizeof(float);
    return g;
}

struct PitchKernelArgs {
    const float* wav;        // (B, S)
    const int32_t* lengths;  // (B)
    float* f0;               // (B, Tf_max)
    int32_t* f0_frames;      // (B) or null
    float* dmin;             // (B, Tf_max) or null
    float* cmnd;             // (B, Tf_max, nl) or null
    int S, Tf_max, hop, win, blk, r, nl, lc, tile, P, span, tau_min, tau_max;
    float threshold;
    double sr;
};

// One workgroup = one utterance x `tile` consecutive frames.
//   1. The sample span of the tile - (tile - 1) hop + W + tau_max + 1 samples from t0 hop - W / 2, zero outside [0, n) - goes into
//      LDS once (plus slack that only lags past tau_max + 1 and the read one step ahead touch).
//   2. Block partials p(h, tau) = sum_{j < blk} (x[h hop + j] - x[h hop + j + tau])^2 in the direct form on the VALU.  A 16-lane
//      group owns one block and 64 lags, a lane four consecutive lags 4 q .. 4 q + 3.  Per four samples j0 .. j0 + 3 a lane reads
//      one 16-byte word the whole group shares (x[j0 ..], a broadcast) and one of its own (x[j0 + 4 q + 4 ..], consecutive lanes in
//      consecutive 16-byte slots: conflict-free within a block and across blocks where hop is a multiple of 64; DESIGN.md has the other cases), both one step ahead of their use; with the word kept from the step before that
//      is the seven-sample window the sixteen pairs need - LDS is read once per sample per group, not once per pair.  Sixteen independent fp32 accumulators
//      (j mod 4, lag); a lag's four are added as (0 + 1) + (2 + 3).
//   3. A wave per frame: d(tau) = the frame's r partials added left to right in fp32; the running sum over the lags is an fp64
//      wave scan with a carry from one 64-lag chunk to the next; d' = d tau / sum formed in fp64 and rounded once, into the wave's
//      own LDS row (and the diagnostic output).
//   4. The same wave picks (first lag under the threshold by a wave minimum, the walk and the refinement uniformly) and stores.
// Nothing depends on B, S or the row: the order of every sum is a function of (t mod tile, tau) alone.
__global__ __launch_bounds__(MEL_THREADS) void mel_pitch_kernel(const PitchKernelArgs a) {
    extern __shared__ float4 pitch_smem[];
    float* span = reinterpret_cast<float*>(pitch_smem);  // (stage 2 reads the same words through pitch_smem: no __restrict__)
    float* __restrict__ part = span + a.span;        // [P][lc]
    float* __restrict__ rows = part + a.P * a.lc;    // [wave][lc]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * a.tile;
    const int n = mel_len(a.lengths, b, a.S);
    const int Tf = n > 0 ? 1 + n / a.hop : 0;
    if (blockIdx.x == 0 && tid == 0 && a.f0_frames) a.f0_frames[b] = Tf;
    const int nrows = a.Tf_max - t0 < a.tile ? a.Tf_max - t0 : a.tile;  // frames of this tile that exist in the outputs
    const size_t out0 = (size_t)b * a.Tf_max + t0;
    if (t0 >= Tf) {  // uniform: a tile past the utterance's last frame is zeros
        for (int i = tid; i < nrows; i += MEL_THREADS) {
            a.f0[out0 + i] = 0.0f;
            if (a.dmin) a.dmin[out0 + i] = 0.0f;
        }
        if (a.cmnd)
            for (size_t i = tid; i < (size_t)nrows * a.nl; i += MEL_THREADS) a.cmnd[out0 * a.nl + i] = 0.0f;
        return;
    }
    // ---- 1. the sample span -> LDS
    {
        const float* __restrict__ x = a.wav + (size_t)b * a.S;
        const long long g0 = (long long)t0 * a.hop - a.win / 2;
        for (int i = tid; i < a.span; i += MEL_THREADS) {
            const long long g = g0 + i;
            span[i] = (g >= 0 && g < n) ? x[g] : 0.0f;
        }
    }
    __syncthreads();
    // ---- 2. block partials
    {
        const int nqg = a.lc >> 6, units = a.P * nqg;
        const int full = a.blk >> 2, rest = a.blk & 3;  // steps of four samples; the samples of a last, short step
        for (int u = wave * 4 + (lane >> 4); u < units; u += MEL_THREADS / 16) {
            const int h = u / nqg, q = (u - h * nqg) * 16 + (lane & 15);
            // 16-byte words: hop is a multiple of 4, so a block starts on one
            const float4* __restrict__ xb = pitch_smem + ((h * a.hop) >> 2);
            const float4* __restrict__ xw = xb + q;
            float acc[4][4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) acc[jj][tt] = 0.0f;
            auto pairs = [&acc](const float4& c, const float4& lo, const float4& hi, int live) {
                const float xs[4] = {c.x, c.y, c.z, c.w};
                const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    if (jj < live) {
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) {
                            const float d = xs[jj] - w[jj + tt];
                            acc[jj][tt] = fmaf(d, d, acc[jj][tt]);
                        }
                    }
            };
            float4 c = xb[0], lo = xw[0], hi = xw[1];
            for (int k = 0; k < full; ++k) {
                const float4 cn = xb[k + 1], hn = xw[k + 2];  // the next step's words are in flight under this step's pairs
                pairs(c, lo, hi, 4);
                c = cn, lo = hi, hi = hn;
            }
            if (rest) pairs(c, lo, hi, rest);  // (a block whose length is no multiple of 4)
            float4 p;
            p.x = (acc[0][0] + acc[1][0]) + (acc[2][0] + acc[3][0]);
            p.y = (acc[0][1] + acc[1][1]) + (acc[2][1] + acc[3][1]);
            p.z = (acc[0][2] + acc[1][2]) + (acc[2][2] + acc[3][2]);
            p.w = (acc[0][3] + acc[1][3]) + (acc[2][3] + acc[3][3]);
            *reinterpret_cast<float4*>(part + h * a.lc + 4 * q) = p;
        }
    }
    __syncthreads();
    // ---- 3 + 4. a wave per frame
    float* __restrict__ row = rows + wave * a.lc;
    for (int f = wave; f < nrows; f += MEL_WAVES) {
        const int t = t0 + f;
        float* __restrict__ cm = a.cmnd ? a.cmnd + (out0 + f) * a.nl : nullptr;
        if (t >= Tf) {  // uniform per wave
            if (lane == 0) {
                a.f0[out0 + f] = 0.0f;
                if (a.dmin) a.dmin[out0 + f] = 0.0f;
            }
            if (cm)
                for (int tau = lane; tau < a.nl; tau += 64) cm[tau] = 0.0f;
            continue;
        }
        double carry = 0.0;
        for (int c0 = 0; c0 < a.nl; c0 += 64) {
            const int tau = c0 + lane;
            float d = 0.0f;
            if (tau < a.nl) {
                d = part[f * a.lc + tau];
                for (int i = 1; i < a.r; ++i) d += part[(f + i) * a.lc + tau];
            }
            double s = (tau >= 1 && tau < a.nl) ? (double)d : 0.0;
            for (int o = 1; o < 64; o <<= 1) {
                const double up = __shfl_up(s, o);
                if (lane >= o) s += up;
            }
            const double cum = carry + s;
            carry = __shfl(cum, 63);
            if (tau < a.nl) {
                const float v = (tau == 0 || cum == 0.0) ? 1.0f : (float)((double)d * (double)tau / cum);
                row[tau] = v;
                if (cm) cm[tau] = v;
            }
        }
        mel_wave_sync();  // the row is the wave's own: its stores before its loads, no workgroup barrier
        int tau = 0x7fffffff;
        for (int k = a.tau_min + lane; k <= a.tau_max; k += 64)
            if (row[k] < a.threshold) {
                tau = k;
                break;
            }
        for (int o = 32; o; o >>= 1) {
            const int other = __shfl_xor(tau, o);
            tau = other < tau ? other : tau;
        }
        float f0 = 0.0f, dm;
        if (tau <= a.tau_max) {  // uniform from here: every lane walks the same lags
            while (tau + 1 <= a.tau_max && row[tau + 1] < row[tau]) ++tau;
            const double p = row[tau - 1], q = row[tau], r = row[tau + 1];
            const double curv = p - 2.0 * q + r;
            double delta = 0.0;
            if (curv > 0.0) {
                delta = (p - r) / (2.0 * curv);
                delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
            }
            f0 = (float)(a.sr / ((double)tau + delta));
            dm = (float)q;
        } else {
            dm = __builtin_inff();
            for (int k = a.tau_min + lane; k <= a.tau_max; k += 64) dm = fminf(dm, row[k]);
            for (int o = 32; o; o >>= 1) dm = fminf(dm, __shfl_xor(dm, o));
        }
        if (lane == 0) {
            a.f0[out0 + f] = f0;
            if (a.dmin) a.dmin[out0 + f] = dm;
        }
        mel_wave_sync();  // the row is rewritten for the wave's next frame
    }
}

typedef void (*MelKernelFn)(const MelKernelArgs);

static MelKernelFn mel_kernel_for(int mt, int nt) {
    switch (mt * 10 + nt) {
        case 11: return mel_stft_kernel<1, 1>;
        case 12: return mel_stft_kernel<1, 2>;
        case 13: return mel_stft_kernel<1, 3>;
        case 14: return mel_stft_kernel<1, 4>;
        case 21: return mel_stft_kernel<2, 1>;
        case 22: return mel_stft_kernel<2, 2>;
        case 23: return mel_stft_kernel<2, 3>;
        case 24: return mel_stft_kernel<2, 4>;
    }
    return nullptr;
}

// LDS bytes of a workgroup of tm frames: max(padded span, cross-wave sum) + the four |X| stages
static size_t mel_lds_bytes(int n_fft, int hop, int tm, int nt) {
    const int mt = tm > 32 ? 2 : 1;
    const size_t span = (size_t)(tm - 1) * hop + n_fft;
    const size_t span_words = span + span / hop + 1;
    const size_t out_words = (size_t)mt * 32 * (nt * 32 + 1);
    return ((span_words > out_words ? span_words : out_words) + (size_t)MEL_WAVES * mt * 32 * MEL_STAGE_LD) * sizeof(float);
}

}  // namespace fs2

using namespace fs2;

struct fs2_mel : ErrorBase {
    int n_fft = 0, win = 0, hop = 0, lh = 0, n_mels = 0, log_kind = 0;
    float clip = 0.0f;
    int f_lo = 0, nbt = 0, tm = 0, mt = 0, nt = 0;
    size_t lds = 0;
    MelKernelFn kernel = nullptr;
    DevAllocs tables, snr_alloc;  // owners of table + btab / of snr_table (replaced whole by fs2_mel_set_snr_table)
    float4* table = nullptr;
    float4* btab = nullptr;
    double* snr_table = nullptr;  // the WADA table (fs2_mel_set_snr_table), snr_k entries for db_lo, db_lo + 1, ...
    int snr_k = 0;
    float snr_db_lo = 0.0f;
    bool ready = false;
};

namespace {

size_t mel_ws_need(int B) { return (((size_t)B * sizeof(uint32_t)) + 255) & ~(size_t)255; }

// The lag range and the tile of a (sample_rate, f0_floor, f0_ceil) on this handle's geometry, or the FS2_ERR_SHAPE that refuses it
int pitch_plan(fs2_mel* m, int sample_rate, float f0_floor, float f0_ceil, int* tau_min, int* tau_max, PitchGeom* geom) {
    if (m->hop < 1) return m->fail(FS2_ERR_STATE, "fs2_mel_create did not succeed");  // no geometry to judge
    if (sample_rate <= 0 || !(f0_floor > 0.0f) || !(f0_ceil > 0.0f) || !isfinite(f0_floor) || !isfinite(f0_ceil))
        return m->fail(FS2_ERR_SHAPE, "sample_rate %d, f0_floor %g, f0_ceil %g: all three must be positive", sample_rate, (double)f0_floor,
                       (double)f0_ceil);
    const double hi = ceil((double)sample_rate / (double)f0_floor), lo = floor((double)sample_rate / (double)f0_ceil);
    if (hi + 2.0 > (double)PITCH_MAX_LAGS)
        return m->fail(FS2_ERR_SHAPE, "tau_max = ceil(%d / %g) = %.0f: tau_max + 2 exceeds %d lags", sample_rate, (double)f0_floor, hi, PITCH_MAX_LAGS);
    const int tmax = (int)hi, tmin = lo < 2.0 ? 2 : (lo > (double)PITCH_MAX_LAGS ? PITCH_MAX_LAGS : (int)lo);
    if (tmin >= tmax) return m->fail(FS2_ERR_SHAPE, "tau_min = %d is not below tau_max = %d: f0_ceil must lie above f0_floor", tmin, tmax);
    if (m->hop % 4) return m->fail(FS2_ERR_SHAPE, "hop %d is no multiple of 4: the tracker reads its span in 16-byte words", m->hop);
    PitchGeom g{};
    int tile = 64;  // the tallest tile of 64, 32, ... frames within the LDS target; a single frame may take the whole CU's LDS
    for (; tile >= 1; tile >>= 1) {
        g = pitch_geom(m->win, m->hop, tmax, tile);
        if (g.lds <= (tile > 1 ? PITCH_LDS_TARGET : MEL_LDS_LIMIT)) break;
    }
    if (tile < 1) return m->fail(FS2_ERR_SHAPE, "win_length %d with hop %d and %d lags does not fit one frame into LDS", m->win, m->hop, tmax + 2);
    if (tau_min) *tau_min = tmin;
    if (tau_max) *tau_max = tmax;
    if (geom) *geom = g;
    return FS2_OK;
}

}  // namespace

extern "C" {

int fs2_mel_create(int32_t abi_version, int32_t n_fft, int32_t win_length, int32_t hop, int32_t n_mels, float clip, int32_t log_kind,
                   const float* mel_basis_host, fs2_mel** out) {
    if (!out) return FS2_ERR_ARG;
    *out = nullptr;
    fs2_mel* m = new (std::nothrow) fs2_mel();
    if (!m) return FS2_ERR_NOMEM;
    *out = m;  // returned even on failure so the caller can read fs2_mel_last_error, then destroy
    if (abi_version != FS2_ABI_VERSION) return m->fail(FS2_ERR_ARG, "abi_version %d, this library is %d", abi_version, FS2_ABI_VERSION);
    if (!mel_basis_host) return m->fail(FS2_ERR_ARG, "mel_basis is null");
    if (log_kind != FS2_MEL_LOG10 && log_kind != FS2_MEL_LN && log_kind != FS2_MEL_LINEAR)
        return m->fail(FS2_ERR_ARG, "log_kind %d is none of FS2_MEL_LOG10, FS2_MEL_LN, FS2_MEL_LINEAR", log_kind);
    if (!(clip > 0.0f) || !isfinite(clip)) return m->fail(FS2_ERR_ARG, "clip must be a positive finite number");
    if (n_fft < 256 || n_fft > 2048 || (n_fft & (n_fft - 1))) return m->fail(FS2_ERR_SHAPE, "n_fft %d is not a power of two in [256, 2048]", n_fft);
    if (win_length < 1 || win_length > n_fft) return m->fail(FS2_ERR_SHAPE, "win_length %d is outside [1, n_fft = %d]", win_length, n_fft);
    if (hop < 1 || n_fft % hop) return m->fail(FS2_ERR_SHAPE, "hop %d does not divide n_fft %d", hop, n_fft);
    if (n_mels < 1 || n_mels > 128) return m->fail(FS2_ERR_SHAPE, "n_mels %d is outside [1, 128]", n_mels);
    const int nbins = n_fft / 2 + 1;
    int f_lo = nbins, f_hi = -1;
    for (int i = 0; i < n_mels; ++i)
        for (int f = 0; f < nbins; ++f) {
            const float w = mel_basis_host[(size_t)i * nbins + f];
            if (!isfinite(w)) return m->fail(FS2_ERR_ARG, "mel_basis[%d][%d] is not finite", i, f);
            if (w != 0.0f) {
                f_lo = f < f_lo ? f : f_lo;
                f_hi = f > f_hi ? f : f_hi;
            }
        }
    if (f_hi < 0) f_lo = f_hi = 0;  // an all-zero basis: one (zero-weight) bin tile, every mel is log(clip)
    m->n_fft = n_fft, m->win = win_length, m->hop = hop, m->n_mels = n_mels, m->log_kind = log_kind, m->clip = clip;
    while ((1 << m->lh) < hop) ++m->lh;
    m->f_lo = f_lo;
    m->nbt = (f_hi - f_lo + 1 + 31) / 32;
    m->nt = (n_mels + 31) / 32;
    for (int tm = 64; tm >= 16 && !m->tm; tm >>= 1)  // the tallest tile whose span fits the CU's LDS
        if (mel_lds_bytes(n_fft, hop, tm, m->nt) <= MEL_LDS_LIMIT) m->tm = tm;
    if (!m->tm) return m->fail(FS2_ERR_SHAPE, "n_fft %d with hop %d does not fit a 16-frame tile into LDS", n_fft, hop);
    m->mt = m->tm > 32 ? 2 : 1;
    m->lds = mel_lds_bytes(n_fft, hop, m->tm, m->nt);
    m->kernel = mel_kernel_for(m->mt, m->nt);
    // ---- the tables, in float64, rounded once
    const int KC = n_fft / 8;
    std::vector<double> win, cs, sn;
    std::vector<float> table, btab;
    try {
        win.assign(n_fft, 0.0), cs.resize(n_fft), sn.resize(n_fft);
        table.resize((size_t)m->nbt * KC * 2 * 64 * 4);
        btab.resize((size_t)m->nbt * 4 * m->nt * 64 * 4);
    } catch (const std::bad_alloc&) {  // no exception crosses the C ABI
        return m->fail(FS2_ERR_NOMEM, "out of host memory for the DFT table");
    }
    const double two_pi = 6.283185307179586476925286766559;
    const int left = (n_fft - win_length) / 2;  // torch.stft centres a short window
    for (int i = 0; i < win_length; ++i) win[left + i] = 0.5 - 0.5 * cos(two_pi * i / win_length);
    for (int r = 0; r < n_fft; ++r) cs[r] = cos(two_pi * r / n_fft), sn[r] = sin(two_pi * r / n_fft);
    for (int bt = 0; bt < m->nbt; ++bt)
        for (int kc = 0; kc < KC; ++kc)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int k = kc * 8 + (lane >> 5) * 4 + e, f = f_lo + bt * 32 + (lane & 31);
                    const size_t at = ((((size_t)bt * KC + kc) * 2) * 64 + lane) * 4 + e;
                    const int r = (int)(((long long)f * k) % n_fft);  // the phase reduced exactly
                    table[at] = f <= f_hi ? (float)(win[k] * cs[r]) : 0.0f;
                    table[at + 64 * 4] = f <= f_hi ? (float)(win[k] * sn[r]) : 0.0f;
                }
    for (int bt = 0; bt < m->nbt; ++bt)
        for (int kc = 0; kc < 4; ++kc)
            for (int nt = 0; nt < m->nt; ++nt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int f = f_lo + bt * 32 + kc * 8 + (lane >> 5) * 4 + e, mel = nt * 32 + (lane & 31);
                        btab[(((((size_t)bt * 4 + kc) * m->nt + nt) * 64) + lane) * 4 + e] =
                            (f <= f_hi && mel < n_mels) ? mel_basis_host[(size_t)mel * nbins + f] : 0.0f;
                    }
    FS2_TRY(upload_as(*m, m->tables, table.data(), table.size(), FS2_F32, (void**)&m->table, FS2_ERR_HIP));
    FS2_TRY(upload_as(*m, m->tables, btab.data(), btab.size(), FS2_F32, (void**)&m->btab, FS2_ERR_HIP));
    if (hipFuncSetAttribute((const void*)m->kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->lds) != hipSuccess)
        return m->fail(FS2_ERR_HIP, "cannot reserve %zu bytes of LDS: %s", m->lds, hipGetErrorString(hipGetLastError()));
    m->ready = true;
    return FS2_OK;
}

int fs2_mel_destroy(fs2_mel* m) {
    if (!m) return FS2_ERR_ARG;
    delete m;
    return FS2_OK;
}

const char* fs2_mel_last_error(const fs2_mel* m) { return m ? m->err : "null mel handle"; }

int32_t fs2_mel_tile_frames(const fs2_mel* m) { return m ? m->tm : 0; }

int fs2_mel_used_bins(const fs2_mel* m, int32_t* first_bin, int32_t* n_columns) {
    if (!m || !first_bin || !n_columns) return FS2_ERR_ARG;
    *first_bin = m->f_lo;
    *n_columns = m->nbt * 32;
    return FS2_OK;
}

size_t fs2_mel_ws_bytes(const fs2_mel* m, int32_t B, int32_t S) {
    (void)S;
    return m && B > 0 ? mel_ws_need(B) : 0;
}

int fs2_mel_run(fs2_mel* m, const float* wav, const int32_t* lengths, int32_t B, int32_t S, int32_t peak_normalize, float* mel,
                int32_t T_max, float* energy, int32_t Te_max, int32_t* mel_frames, int32_t* energy_frames, void* ws, size_t ws_bytes,
                void* hip_stream) {
    if (!m) return FS2_ERR_ARG;
    if (!m->ready) return m->fail(FS2_ERR_STATE, "fs2_mel_create did not succeed");
    if (!wav || !lengths || !mel || !mel_frames) return m->fail(FS2_ERR_ARG, "wav, lengths, mel and mel_frames must not be null");
    if (B < 1 || S < 1) return m->fail(FS2_ERR_ARG, "B = %d, S = %d: both must be at least 1", B, S);
    if (B > 65535) return m->fail(FS2_ERR_SHAPE, "B = %d exceeds the grid's 65535 utterances", B);
    if (T_max < 1 + S / m->hop) return m->fail(FS2_ERR_ARG, "T_max = %d < 1 + S / hop = %d", T_max, 1 + S / m->hop);
    const int te_need = (int)(((long long)S + m->hop - 1) / m->hop);
    if (energy && Te_max < te_need) return m->fail(FS2_ERR_ARG, "Te_max = %d < ceil(S / hop) = %d", Te_max, te_need);
    if ((long long)T_max * m->n_mels > 0x7fffffffLL) return m->fail(FS2_ERR_SHAPE, "T_max * n_mels exceeds 2^31");
    if (!ws || ws_bytes < mel_ws_need(B))  // asked for in every mode: a caller sizes one buffer, whatever it switches later
        return m->fail(FS2_ERR_NOMEM, "workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, mel_ws_need(B));
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t* peak = nullptr;
    if (peak_normalize) {
        peak = (uint32_t*)ws;
        if (hipMemsetAsync(peak, 0, (size_t)B * sizeof(uint32_t), st) != hipSuccess) return m->fail(FS2_ERR_HIP, "hipMemsetAsync failed");
        int chunks = (S + 4095) / 4096;
        chunks = chunks > 64 ? 64 : chunks;
        hipLaunchKernelGGL(mel_peak_kernel, dim3(chunks, B), dim3(256), 0, st, wav, lengths, peak, S);
    }
    MelKernelArgs a{wav, lengths, peak, m->table, m->btab, mel, mel_frames, energy_frames, S, T_max, m->n_fft, m->hop, m->lh,
                    m->n_mels, m->nbt, m->tm, m->log_kind, m->clip};
    void* kargs[] = {&a};
    if (hipLaunchKernel((const void*)m->kernel, dim3((T_max + m->tm - 1) / m->tm, B), dim3(MEL_THREADS), kargs, m->lds, st) != hipSuccess)
        return m->fail(FS2_ERR_HIP, "launch of the STFT kernel failed: %s", hipGetErrorString(hipGetLastError()));
    if (energy) hipLaunchKernelGGL(mel_energy_kernel, dim3((Te_max + 3) / 4, B), dim3(256), 0, st, wav, lengths, peak, energy, S, Te_max, m->hop, m->win);
    if (hipGetLastError() != hipSuccess) return m->fail(FS2_ERR_HIP, "a launch of fs2_mel_run failed");
    return FS2_OK;
}

int fs2_op_segment_mean(const float* values, const int32_t* frames, const int32_t* durations, int32_t B, int32_t T, int32_t L,
                        float empty_value, float mean, float stdev, float* out, void* hip_stream) {
    if (!values || !durations || !out || B < 1 || T < 1 || L < 1) return FS2_ERR_ARG;
    if (!(stdev != 0.0f) || !isfinite(stdev) || !isfinite(mean)) return FS2_ERR_ARG;
    hipLaunchKernelGGL(segment_mean_kernel, dim3(B), dim3(256), 0, (hipStream_t)hip_stream, values, frames, durations, out, T, L,
                       empty_value, mean, stdev);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

int fs2_mel_set_snr_table(fs2_mel* m, const double* table_host, int32_t n, float db_lo) {
    if (!m) return FS2_ERR_ARG;
    if (!table_host) return m->fail(FS2_ERR_ARG, "the SNR table is null");
    if (n < 2 || n > SNR_MAX_TABLE) return m->fail(FS2_ERR_ARG, "the SNR table has %d entries, outside [2, %d]", n, SNR_MAX_TABLE);
    if (!isfinite(db_lo)) return m->fail(FS2_ERR_ARG, "db_lo is not finite");
    for (int i = 0; i < n; ++i)
        if (!isfinite(table_host[i])) return m->fail(FS2_ERR_ARG, "SNR table entry %d is not finite", i);
    if (!m->ready) return m->fail(FS2_ERR_STATE, "fs2_mel_create did not succeed");
    double* dev = nullptr;
    DevAllocs fresh;  // (a failed upload leaves the old table in place)
    FS2_TRY(upload_bytes(*m, fresh, table_host, (size_t)n * sizeof(double), (void**)&dev, FS2_ERR_HIP));
    m->snr_alloc.swap(fresh);  // the old table goes with `fresh`: its hipFree waits for launches that still read it
    m->snr_table = dev, m->snr_k = n, m->snr_db_lo = db_lo;
    return FS2_OK;
}

int fs2_mel_snr(fs2_mel* m, const float* wav, const int32_t* lengths, int32_t B, int32_t S, int32_t peak_normalize, float* snr,
                int32_t Te_max, int32_t* snr_frames, void* ws, size_t ws_bytes, void* hip_stream) {
    if (!m) return FS2_ERR_ARG;
    if (m->hop < 1) return m->fail(FS2_ERR_STATE, "fs2_mel_create did not succeed");  // no geometry to judge
    if (m->win % m->hop) return m->fail(FS2_ERR_SHAPE, "win_length %d is not a multiple of hop %d: the windowed SNR needs one", m->win, m->hop);
    if (!m->ready) return m->fail(FS2_ERR_STATE, "fs2_mel_create did not succeed");
    if (!m->snr_table) return m->fail(FS2_ERR_STATE, "no SNR table: call fs2_mel_set_snr_table first (the library ships none)");
    if (!wav || !lengths || !snr) return m->fail(FS2_ERR_ARG, "wav, lengths and snr must not be null");
    if (B < 1 || S < 1) return m->fail(FS2_ERR_ARG, "B = %d, S = %d: both must be at least 1", B, S);
    if (B > 65535) return m->fail(FS2_ERR_SHAPE, "B = %d exceeds the grid's 65535 utterances", B);
    const int te_need = (int)(((long long)S + m->hop - 1) / m->hop);
    if (Te_max < te_need) return m->fail(FS2_ERR_ARG, "Te_max = %d < ceil(S / hop) = %d", Te_max, te_need);
    if (!ws || ws_bytes < mel_ws_need(B))
        return m->fail(FS2_ERR_NOMEM, "workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, mel_ws_need(B));
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t* peak = nullptr;
    if (peak_normalize) {
        peak = (uint32_t*)ws;
        if (hipMemsetAsync(peak, 0, (size_t)B * sizeof(uint32_t), st) != hipSuccess) return m->fail(FS2_ERR_HIP, "hipMemsetAsync failed");
        int chunks = (S + 4095) / 4096;
        chunks = chunks > 64 ? 64 : chunks;
        hipLaunchKernelGGL(mel_peak_kernel, dim3(chunks, B), dim3(256), 0, st, wav, lengths, peak, S);
    }
    const size_t lds = snr_lds_bytes(SNR_TILE + m->win / m->hop - 1, m->snr_k);
    hipLaunchKernelGGL(mel_snr_kernel, dim3((Te_max + SNR_TILE - 1) / SNR_TILE, B), dim3(256), lds, st, wav, lengths, peak, m->snr_table,
                       m->snr_k, snr, snr_frames, S, Te_max, m->hop, m->win);
    if (hipGetLastError() != hipSuccess) return m->fail(FS2_ERR_HIP, "a launch of fs2_mel_snr failed");
    return FS2_OK;
}

int fs2_mel_pitch_lags(fs2_mel* m, int32_t sample_rate, float f0_floor, float f0_ceil, int32_t* tau_min, int32_t* tau_max) {
    if (!m) return FS2_ERR_ARG;
    if (!tau_min || !tau_max) return m->fail(FS2_ERR_ARG, "tau_min and tau_max must not be null");
    return pitch_plan(m, sample_rate, f0_floor, f0_ceil, tau_min, tau_max, nullptr);
}

int32_t fs2_mel_pitch_tile_frames(fs2_mel* m, int32_t sample_rate, float f0_floor) {
    if (!m) return 0;
    PitchGeom g{};
    return pitch_plan(m, sample_rate, f0_floor, (float)sample_rate, nullptr, nullptr, &g) == FS2_OK ? g.tile : 0;
}

int fs2_mel_pitch(fs2_mel* m, const float* wav, const int32_t* lengths, int32_t B, int32_t S, int32_t sample_rate, float f0_floor,
                  float f0_ceil, float threshold, float* f0, int32_t Tf_max, int32_t* f0_frames, float* dmin, float* cmnd, int32_t n_lags,
                  void* hip_stream) {
    if (!m) return FS2_ERR_ARG;
    int tau_min = 0, tau_max = 0;
    PitchGeom g{};
    FS2_TRY(pitch_plan(m, sample_rate, f0_floor, f0_ceil, &tau_min, &tau_max, &g));
    if (!(threshold > 0.0f && threshold <= 1.0f)) return m->fail(FS2_ERR_SHAPE, "threshold %g lies outside (0, 1]", (double)threshold);
    if (!m->ready) return m->fail(FS2_ERR_STATE, "fs2_mel_create did not succeed");
    if (!wav || !lengths || !f0) return m->fail(FS2_ERR_ARG, "wav, lengths and f0 must not be null");
    if (B < 1 || S < 1) return m->fail(FS2_ERR_ARG, "B = %d, S = %d: both must be at least 1", B, S);
    if (B > 65535) return m->fail(FS2_ERR_SHAPE, "B = %d exceeds the grid's 65535 utterances", B);
    if (Tf_max < 1 + S / m->hop) return m->fail(FS2_ERR_ARG, "Tf_max = %d < 1 + S / hop = %d", Tf_max, 1 + S / m->hop);
    if (cmnd && n_lags != tau_max + 2) return m->fail(FS2_ERR_ARG, "n_lags = %d, cmnd holds tau_max + 2 = %d lags", n_lags, tau_max + 2);
    // the reservation belongs to the kernel, not to a handle: a single-frame tile above the default limit asks for its own each time
    if (g.lds > PITCH_LDS_TARGET &&
        hipFuncSetAttribute((const void*)mel_pitch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds) != hipSuccess)
        return m->fail(FS2_ERR_HIP, "cannot reserve %zu bytes of LDS: %s", g.lds, hipGetErrorString(hipGetLastError()));
    PitchKernelArgs a{wav, lengths, f0, f0_frames, dmin, cmnd, S, Tf_max, m->hop, m->win, g.blk, g.r, g.nl, g.lc, g.tile, g.P, g.span,
                      tau_min, tau_max, threshold, (double)sample_rate};
    hipLaunchKernelGGL(mel_pitch_kernel, dim3((Tf_max + g.tile - 1) / g.tile, B), dim3(MEL_THREADS), g.lds, (hipStream_t)hip_stream, a);
    if (hipGetLastError() != hipSuccess) return m->fail(FS2_ERR_HIP, "the launch of fs2_mel_pitch failed");
    return FS2_OK;
}

int fs2_op_contour_finish(const float* values, const int32_t* frames, const int32_t* durations, const int32_t* phone_silent, int32_t B,
                          int32_t T, int32_t L, int32_t zero_is_missing, float all_missing_value, float mean, float stdev, float* out,
                          int32_t* frames_out, float* prior, void* hip_stream) {
    if (!values || !durations || !out || !frames_out || B < 1 || T < 1 || L < 1) return FS2_ERR_ARG;
    if (!(stdev != 0.0f) || !isfinite(stdev) || !isfinite(mean)) return FS2_ERR_ARG;
    if (T > FIN_MAX_T || L > FIN_MAX_L) return FS2_ERR_SHAPE;
    hipLaunchKernelGGL(contour_finish_kernel, dim3(B), dim3(256), 0, (hipStream_t)hip_stream, values, frames, durations, phone_silent, out,
                       frames_out, prior, T, L, zero_is_missing, all_missing_value, mean, stdev);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

int fs2_op_masked_row_mean(const float* values, const int32_t* counts, const int32_t* skip, int32_t B, int32_t N, float* out,
                           void* hip_stream) {
    if (!values || !out || B < 1 || N < 1) return FS2_ERR_ARG;
    hipLaunchKernelGGL(masked_row_mean_kernel, dim3(B), dim3(256), 0, (hipStream_t)hip_stream, values, counts, skip, out, N);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

}  // extern "C"
