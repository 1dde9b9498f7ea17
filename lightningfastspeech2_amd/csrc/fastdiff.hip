// FastDiff vocoder at inference (reference: litfass/third_party/fastdiff/FastDiff.py:91-195, module/modules.py:116-343,
// module/util.py:158-237, 305-343): the eps network and the reverse sampler behind fs2_fd_* of include/fs2.h.
//
// Activations are time-major rows (samples or frames) with the channels contiguous; every utterance is computed alone, with zero
// padding at ITS ends in every layer (generator.py:163-168), and every launch tiles an utterance in FD_TILE rows from its own first
// row, so the bits of a result do not depend on the batch around it.
//
// Launches of one eps evaluation (71):
//   fd_first_conv_kernel                       first_audio_conv 1 -> 32, k7                                  (FastDiff.py:125)
//   3 x DiffusionDBlock = 4 x fd_conv_kernel   1x1 residual and k3 dil 1 read every factor-th row (nearest down-sampling of lengths
//                                              that are multiples of the factor), k3 dil 2, k3 dil 4 + residual  (modules.py:127-138)
//   per LVC block (3 x 19):
//     fd_cond_kernel                           mel + fc_t(step embedding); the 80 offsets are constants of (weights, step), computed
//                                              on the host in double and passed by value                        (modules.py:202-203)
//     9 x fd_conv_kernel                       kernel predictor: k5 80 -> 64, six k3 64 -> 64 with one residual around them,
//                                              kernel_conv 64 -> 24576 (rows permuted at finalize into the LVC launch's fragment
//                                              order) and bias_conv 64 -> 256                                   (modules.py:320-343)
//     fd_conv_kernel                           ConvTranspose1d(k = 2r, stride r, pad r/2) as a 3-tap conv to r * 32 phase-major
//                                              channels ((T, r*32) row-major IS (T*r, 32) row-major), + audio_down  (modules.py:205-209)
//     4 x (fd_conv_kernel, fd_lvc_kernel)      y = lrelu(conv_k3_dil(3^i)(lrelu(x))); the location-variable convolution with bias, the
//                                              sigmoid * tanh gate, the residual and the NEXT layer's `x += audio_down` in its
//                                              epilogue                                                         (modules.py:208-217)
//   fd_final_conv_kernel                       final_conv 32 -> 1, k7 = eps                                      (FastDiff.py:135)
// The sampler adds fd_update_kernel per step (util.py:228-231) and one fd_peak_scale_kernel (FastDiff.py:193).
//
// fd_conv_kernel: 256 threads = 4 waves x 16 rows; the (64 + halo)-row operand slab goes to LDS once (bounds, stride, input
// LeakyReLU applied while staging), weights stream from L2 in MFMA fragment order (packed at finalize), the bias rides in as the
// accumulators' initial value.  fp32 runs on the fp32 MFMA, bf16 on v_mfma_f32_16x16x32_bf16 (Mma16, fs2_common.h).
//
// fd_lvc_kernel: per (frame, layer) a `hop` x 96 x 64 product whose weight operand changes every frame.  A wave owns 16 rows; its
// weight fragments come straight from the predicted-kernel tensor, which kernel_conv wrote in fragment order (a frame's layer slice is
// 24 KiB fp32 / 12 KiB bf16, contiguous: one 1 KiB wave load per fragment).  The y rows of a tile and a one-sample halo on each side
// are staged once in LDS: a neighbour across a frame border is the real sample, zero only outside the utterance.  hop 64 and 256: the
// 16 rows lie inside one frame.  hop 8: the 16 rows span TWO frames; the wave runs the K loop once per frame with the rows of the other
// frame zeroed in the sample operand (K concatenation: 2 x 96), so both frames share the MFMA tile instead of leaving half of it idle.
// That doubles the MFMA work of the hop-8 block, which is 1/32 of the rows of the hop-256 block: +3 % of the LVC's arithmetic, in
// exchange for one code path and full-width loads of the kernels.
#include "fs2_host.h"

#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

namespace fs2 {
namespace {

constexpr int FD_TILE = 64;       // rows per workgroup of every tiled launch
constexpr int FD_CH = 32;         // inner_channels
constexpr int FD_KW = 24576;      // predicted kernel values per frame: 4 layers x 32 x 64 x 3
constexpr int FD_KL = 6144;       // ... per layer
constexpr int FD_NB = 256;        // predicted biases per frame: 4 x 64
constexpr int FD_MEL = 80, FD_MELP = 96, FD_HID = 64, FD_HOP = 256;

template <typename T> struct FdT;
template <> struct FdT<float> { static constexpr int KE = 16, E16 = 4; };  // elements per 64-byte k-step, per 16 bytes
template <> struct FdT<bf16> { static constexpr int KE = 32, E16 = 8; };

__device__ inline float fd_lrelu(float v, float s) { return v > 0.f ? v : v * s; }

template <typename T> __device__ inline void fd_load4(const T* p, float* f);
template <> __device__ inline void fd_load4<float>(const float* p, float* f) {
    const float4 v = *(const float4*)p;
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
}
template <> __device__ inline void fd_load4<bf16>(const bf16* p, float* f) {
    const uint2 u = *(const uint2*)p;
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
}
template <typename T> __device__ inline void fd_store4(T* p, const float* f);
template <> __device__ inline void fd_store4<float>(float* p, const float* f) { *(float4*)p = make_float4(f[0], f[1], f[2], f[3]); }
template <> __device__ inline void fd_store4<bf16>(bf16* p, const float* f) {
    *(uint2*)p = make_uint2(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]));
}

// ---- generic Conv1d on the MFMA: out[t, n] = act_out(bias[n] + sum_{tap, c} act_in(x[(t + (tap - c0) * dil) * stride, c]) W[n, c, tap]
//                                               + add1[t, n]) + add2[t, n] ----
struct FdConvArgs {
    const void* x; const void* w; const float* bias; const void* add1; const void* add2; void* out;
    const int* lengths;
    int B, T;               // utterances, padded frames (lengths == NULL: every utterance has T)
    int rows_in, rows_out;  // allocated rows per utterance of x and of out / add1 / add2
    int len_scale;          // valid output rows of an utterance = frames * len_scale
    int in_stride, taps, dil, n;
    int nrep;               // column tiles a workgroup walks with its slab in place (set by the launcher)
    float in_slope, out_slope;
};

// the (FD_TILE + halo)-row operand slab of a tile -> LDS: bounds, stride and input LeakyReLU applied on the way
template <typename T, int CIN>
__device__ inline void fd_stage_slab(const FdConvArgs& p, unsigned char* slab, int ub, int t0, int len, int tid) {
    constexpr int E16 = FdT<T>::E16, PPR = CIN / E16, ROWB = CIN * (int)sizeof(T) + 16;
    const int c0 = (p.taps - 1) / 2, rows = FD_TILE + (p.taps - 1) * p.dil;
    const T* xb = (const T*)p.x + (size_t)ub * p.rows_in * CIN;
    for (int q = tid; q < rows * PPR; q += 256) {
        const int i = q / PPR, s = q % PPR, t = t0 - c0 * p.dil + i;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (t >= 0 && t < len) {  // (t < len  =>  t * stride < rows_in: the launcher checks rows_in >= T * len_scale * stride)
            raw = *(const uint4*)(xb + (size_t)t * p.in_stride * CIN + s * E16);
            if (p.in_slope != 1.f) {
                float f[E16];
                Vec16<T>::unpack(raw, f);
#pragma unroll
                for (int e = 0; e < E16; ++e) f[e] = fd_lrelu(f[e], p.in_slope);
                raw = Vec16<T>::pack(f);
            }
        }
        *(uint4*)(slab + i * ROWB + s * 16) = raw;
    }
}

template <typename T, int CIN, int NT>
__global__ __launch_bounds__(256) void fd_conv_kernel(FdConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fd_slab[];
    constexpr int KE = FdT<T>::KE, NKC = CIN / KE;
    constexpr int ROWB = CIN * (int)sizeof(T) + 16;  // + 16: rows 16 apart do not share a bank group
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    const int tiles = (p.rows_out + FD_TILE - 1) / FD_TILE;
    const int ub = blockIdx.x / tiles, tm = blockIdx.x % tiles;
    const int len = (p.lengths ? p.lengths[ub] : p.T) * p.len_scale;
    const int t0 = tm * FD_TILE;
    if (t0 >= len) return;  // block-uniform
    fd_stage_slab<T, CIN>(p, fd_slab, ub, t0, len, tid);
    __syncthreads();

    const int nsteps = p.taps * NKC;
    const uint4* wp = (const uint4*)p.w;
    const int t = t0 + wave * 16 + fr;
    const size_t rowoff = ((size_t)ub * p.rows_out + t) * p.n;
    for (int rep = 0; rep < p.nrep; ++rep) {  // wide outputs (kernel_conv: 24576 columns) reuse the staged slab
        const int nt0 = (blockIdx.y * p.nrep + rep) * NT;
        f32x4_t acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const float4 b = *(const float4*)(p.bias + nt0 * 16 + fg * (4 * NT) + j * 4);
            acc[j] = (f32x4_t){b.x, b.y, b.z, b.w};
        }
        for (int tap = 0; tap < p.taps; ++tap) {
            const unsigned char* arow = fd_slab + (wave * 16 + fr + tap * p.dil) * ROWB + fg * 16;
#pragma unroll
            for (int kc = 0; kc < NKC; ++kc) {
                const uint4 a = *(const uint4*)(arow + kc * 64);
                const int step = tap * NKC + kc;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const uint4 b = wp[((size_t)(nt0 + j) * nsteps + step) * 64 + lane];
                    // weights = row operand: the lane ends with channels of sample row fr; fd_pack_conv places the rows so that
                    // acc[j][r] is column nt0 * 16 + fg * 4 * NT + j * 4 + r: 4 * NT consecutive columns per lane
                    Mma16<T>::step(b, a, acc[j]);
                }
            }
        }
        if (t >= len) continue;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const size_t at = rowoff + nt0 * 16 + fg * (4 * NT) + j * 4;
            float v[4] = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
            if (p.add1) {
                float a[4];
                fd_load4<T>((const T*)p.add1 + at, a);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += a[r];
            }
            if (p.out_slope != 1.f) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fd_lrelu(v[r], p.out_slope);
            }
            if (p.add2) {
                float a[4];
                fd_load4<T>((const T*)p.add2 + at, a);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += a[r];
            }
            fd_store4<T>((T*)p.out + at, v);
        }
    }
}

// The same convolution for wide outputs (kernel_conv: 64 -> 24576): a wave takes ALL 64 rows of the tile and one of the four
// 16-column MFMA tiles of a 64-column group, so a weight fragment is fetched once per workgroup and used for four MFMAs (with a
// wave per 16 rows every wave fetched every fragment: the launch ran at the L2's bandwidth).  Same columns, same order of summation
// per element as fd_conv_kernel<T, CIN, 4>.
template <typename T, int CIN>
__global__ __launch_bounds__(256) void fd_conv_wide_kernel(FdConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fd_slab[];
    constexpr int KE = FdT<T>::KE, NKC = CIN / KE, NT = 4;
    constexpr int ROWB = CIN * (int)sizeof(T) + 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    const int tiles = (p.rows_out + FD_TILE - 1) / FD_TILE;
    const int ub = blockIdx.x / tiles, tm = blockIdx.x % tiles;
    const int len = (p.lengths ? p.lengths[ub] : p.T) * p.len_scale;
    const int t0 = tm * FD_TILE;
    if (t0 >= len) return;  // block-uniform
    fd_stage_slab<T, CIN>(p, fd_slab, ub, t0, len, tid);
    __syncthreads();
    const int nsteps = p.taps * NKC;
    const uint4* wp = (const uint4*)p.w;
    for (int rep = 0; rep < p.nrep; ++rep) {
        const int nt0 = (blockIdx.y * p.nrep + rep) * NT, col = nt0 * 16 + fg * (4 * NT) + wave * 4;
        const float4 b4 = *(const float4*)(p.bias + col);
        f32x4_t acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = (f32x4_t){b4.x, b4.y, b4.z, b4.w};
        const uint4* wt = wp + (size_t)(nt0 + wave) * nsteps * 64 + lane;
        for (int tap = 0; tap < p.taps; ++tap) {
            const unsigned char* arow = fd_slab + (fr + tap * p.dil) * ROWB + fg * 16;
#pragma unroll
            for (int kc = 0; kc < NKC; ++kc) {
                const uint4 b = wt[(tap * NKC + kc) * 64];
#pragma unroll
                for (int m = 0; m < 4; ++m) Mma16<T>::step(b, *(const uint4*)(arow + m * 16 * ROWB + kc * 64), acc[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int t = t0 + m * 16 + fr;
            if (t >= len) continue;
            const size_t at = ((size_t)ub * p.rows_out + t) * p.n + col;
            float v[4] = {acc[m][0], acc[m][1], acc[m][2], acc[m][3]};
            if (p.add1) {
                float a[4];
                fd_load4<T>((const T*)p.add1 + at, a);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += a[r];
            }
            if (p.out_slope != 1.f) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fd_lrelu(v[r], p.out_slope);
            }
            if (p.add2) {
                float a[4];
                fd_load4<T>((const T*)p.add2 + at, a);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += a[r];
            }
            fd_store4<T>((T*)p.out + at, v);
        }
    }
}

// ---- the location-variable convolution with gate and residual (modules.py:214-217, 220-253) ----
struct FdLvcArgs {
    const void* y; const void* k; const void* bias; const void* x; const void* add; void* out;
    const int* lengths;
    int B, T, layer;
};

template <typename T, int HOP>
__global__ __launch_bounds__(256) void fd_lvc_kernel(FdLvcArgs p) {
    constexpr int KE = FdT<T>::KE, E16 = FdT<T>::E16, NKC = FD_CH / KE, NSTEP = 3 * NKC, PPR = FD_CH / E16;
    constexpr int ROWB = FD_CH * (int)sizeof(T) + 16;
    constexpr int FPW = HOP >= 16 ? 1 : 16 / HOP;  // frames under a wave's 16 rows
    __shared__ __attribute__((aligned(16))) unsigned char slab[(FD_TILE + 2) * ROWB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    const int S = p.T * HOP, tiles = (S + FD_TILE - 1) / FD_TILE;
    const int ub = blockIdx.x / tiles, tm = blockIdx.x % tiles;
    const int frames = p.lengths ? p.lengths[ub] : p.T, len = frames * HOP;
    const int t0 = tm * FD_TILE;
    if (t0 >= len) return;  // block-uniform
    const T* yb = (const T*)p.y + (size_t)ub * S * FD_CH;
    for (int q = tid; q < (FD_TILE + 2) * PPR; q += 256) {
        const int i = q / PPR, s = q % PPR, t = t0 - 1 + i;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (t >= 0 && t < len) raw = *(const uint4*)(yb + (size_t)t * FD_CH + s * E16);
        *(uint4*)(slab + i * ROWB + s * 16) = raw;
    }
    __syncthreads();
    const int tw = t0 + wave * 16;
    if (tw >= len) return;  // wave-uniform, behind the only barrier
    const int t = tw + fr;
    // this lane's sample row picks the bias.  acc[j][r] <-> output channel (j / 2) * 32 + fg * 8 + (j % 2) * 4 + r of sample row fr
    // (fd_kernel_index): tiles 0, 1 are the sigmoid half, 2, 3 the tanh half, and a lane owns 8 consecutive channels of each
    const int lmine = min(t / HOP, frames - 1);
    const T* bb = (const T*)p.bias + ((size_t)ub * p.T + lmine) * FD_NB + p.layer * 64 + fg * 8;
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float b[4];
        fd_load4<T>(bb + (j >> 1) * 32 + (j & 1) * 4, b);
        acc[j] = (f32x4_t){b[0], b[1], b[2], b[3]};
    }
#pragma unroll
    for (int f = 0; f < FPW; ++f) {
        const int l = (tw + f * HOP) / HOP;
        if (l >= frames) break;  // wave-uniform
        const bool mine = FPW == 1 || fr / HOP == f;
        const uint4* kb = (const uint4*)((const T*)p.k + ((size_t)ub * p.T + l) * FD_KW + p.layer * FD_KL);
#pragma unroll
        for (int step = 0; step < NSTEP; ++step) {
            const int tap = step / NKC, kc = step % NKC;
            uint4 a = *(const uint4*)(slab + (wave * 16 + fr + tap) * ROWB + kc * 64 + fg * 16);
            if (!mine) a = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int j = 0; j < 4; ++j) Mma16<T>::step(kb[(step * 4 + j) * 64 + lane], a, acc[j]);
        }
    }
    if (t >= len) return;
    const size_t rowoff = ((size_t)ub * S + t) * FD_CH;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const size_t at = rowoff + fg * 8 + j * 4;
        float v[4];
        fd_load4<T>((const T*)p.x + at, v);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (1.f / (1.f + expf(-acc[j][r]))) * tanhf(acc[j + 2][r]);
        if (p.add) {
            float a[4];
            fd_load4<T>((const T*)p.add + at, a);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += a[r];
        }
        fd_store4<T>((T*)p.out + at, v);
    }
}

// ---- the narrow ends and the row kernels ----
struct FdOffsets { float v[FD_MEL]; };

// cond[b, t, c] = mel[b, t, c] + fc_t(step embedding)[c] (modules.py:202-203), padded to 96 channels with zeros
template <typename T>
__global__ __launch_bounds__(256) void fd_cond_kernel(const float* mel, FdOffsets off, T* cond, const int* lengths, int B, int Tf) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * Tf * FD_MELP) return;
    const int c = (int)(i % FD_MELP);
    const size_t row = i / FD_MELP;
    const int b = (int)(row / Tf), t = (int)(row % Tf);
    if (t >= (lengths ? lengths[b] : Tf)) return;
    cond[i] = Num<T>::from_f32(c < FD_MEL ? mel[row * FD_MEL + c] + off.v[c] : 0.f);
}

// first_audio_conv: x (B, S) fp32 -> (B, S, 32); w (32, 1, 7) fp32.  8 lanes share a row, 4 channels each.
template <typename T>
__global__ __launch_bounds__(256) void fd_first_conv_kernel(const float* x, const float* w, const float* bias, T* out, const int* lengths,
                                                           int B, int Tf) {
    const int S = Tf * FD_HOP, tiles = (S + 31) / 32;
    const int ub = blockIdx.x / tiles, t = (blockIdx.x % tiles) * 32 + (threadIdx.x >> 3), c = (threadIdx.x & 7) * 4;
    const int len = (lengths ? lengths[ub] : Tf) * FD_HOP;
    if (t >= len) return;
    const float* xb = x + (size_t)ub * S;
    float xv[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int u = t + k - 3;
        xv[k] = (u >= 0 && u < len) ? xb[u] : 0.f;
    }
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float a = bias[c + r];
#pragma unroll
        for (int k = 0; k < 7; ++k) a = fmaf(xv[k], w[(c + r) * 7 + k], a);
        v[r] = a;
    }
    fd_store4<T>(out + ((size_t)ub * S + t) * FD_CH + c, v);
}

// final_conv: (B, S, 32) -> eps (B, S) fp32; w (1, 32, 7) fp32.  One thread per sample.
template <typename T>
__global__ __launch_bounds__(256) void fd_final_conv_kernel(const T* x, const float* w, const float* bias, float* eps, const int* lengths,
                                                           int B, int Tf) {
    __shared__ float wk[7 * FD_CH];
    if (threadIdx.x < 7 * FD_CH) wk[threadIdx.x] = w[(threadIdx.x % FD_CH) * 7 + threadIdx.x / FD_CH];  // [k][c]
    __syncthreads();
    const int S = Tf * FD_HOP, tiles = (S + 255) / 256;
    const int ub = blockIdx.x / tiles, t = (blockIdx.x % tiles) * 256 + threadIdx.x;
    const int len = (lengths ? lengths[ub] : Tf) * FD_HOP;
    if (t >= len) return;
    const T* xb = x + (size_t)ub * S * FD_CH;
    float a = bias[0];
    for (int k = 0; k < 7; ++k) {
        const int u = t + k - 3;
        if (u < 0 || u >= len) continue;
#pragma unroll
        for (int c = 0; c < FD_CH; c += 4) {
            float f[4];
            fd_load4<T>(xb + (size_t)u * FD_CH + c, f);
#pragma unroll
            for (int r = 0; r < 4; ++r) a = fmaf(f[r], wk[k * FD_CH + c + r], a);
        }
    }
    eps[(size_t)ub * S + t] = a;
}

// one reverse step (util.py:228-231): x -= c1 * eps; x /= d; x += sigma * z while n > 0 - each product and sum rounded as the
// reference's tensor ops round them
__global__ __launch_bounds__(256) void fd_update_kernel(const float* xin, const float* eps, const float* z, float* xout, float c1, float d,
                                                        float sigma, const int* lengths, int B, int Tf) {
#pragma clang fp contract(off)
    const int S = Tf * FD_HOP, tiles = (S + 255) / 256;
    const int ub = blockIdx.x / tiles, t = (blockIdx.x % tiles) * 256 + threadIdx.x;
    if (t >= (lengths ? lengths[ub] : Tf) * FD_HOP) return;
    const size_t i = (size_t)ub * S + t;
    const float m = c1 * eps[i];
    float v = (xin[i] - m) / d;
    if (z) {
        const float n = sigma * z[i];
        v = v + n;
    }
    xout[i] = v;
}

// wav = x / max|x| over the utterance's own samples (FastDiff.py:193): one workgroup per utterance
__global__ __launch_bounds__(1024) void fd_peak_scale_kernel(const float* x, float* wav, const int* lengths, int Tf) {
    __shared__ float red[16];
    const int S = Tf * FD_HOP, ub = blockIdx.x;
    const int len = (lengths ? lengths[ub] : Tf) * FD_HOP;
    const float* xb = x + (size_t)ub * S;
    float m = 0.f;
    for (int t = threadIdx.x; t < len; t += 1024) m = fmaxf(m, fabsf(xb[t]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
    float* wb = wav + (size_t)ub * S;
    for (int t = threadIdx.x; t < len; t += 1024) wb[t] = xb[t] / m;
}

// ---- launchers ----
int fd_conv_nt(int n, int cin_pad);

template <typename T, int CIN, int NT>
int fd_conv_launch_c(FdConvArgs a, hipStream_t st) {
    a.nrep = a.n % (16 * NT * 8) == 0 && a.n >= 2048 ? 8 : 1;
    const int rows = FD_TILE + (a.taps - 1) * a.dil;
    const size_t smem = (size_t)rows * (CIN * sizeof(T) + 16);
    if (smem > 64 * 1024) return FS2_ERR_SHAPE;
    const int tiles = (a.rows_out + FD_TILE - 1) / FD_TILE;
    const dim3 grid((unsigned)(tiles * a.B), (unsigned)(a.n / (16 * NT * a.nrep)));
    if constexpr (NT == 4 && CIN == 64) {
        if (a.nrep > 1) {  // kernel_conv
            hipLaunchKernelGGL((fd_conv_wide_kernel<T, CIN>), grid, dim3(256), smem, st, a);
            return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
        }
    }
    hipLaunchKernelGGL((fd_conv_kernel<T, CIN, NT>), grid, dim3(256), smem, st, a);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

template <typename T>
int fd_conv_launch_t(const FdConvArgs& a, int cin, hipStream_t st) {
    if (fd_conv_nt(a.n, cin) == 2) return fd_conv_launch_c<T, 32, 2>(a, st);
    if (a.n % 64) return FS2_ERR_SHAPE;
    if (cin == 32) return fd_conv_launch_c<T, 32, 4>(a, st);
    if (cin == 64) return fd_conv_launch_c<T, 64, 4>(a, st);
    if (cin == 96) return fd_conv_launch_c<T, 96, 4>(a, st);
    return FS2_ERR_SHAPE;
}

int fd_conv_launch(int dtype, const FdConvArgs& a, int cin, hipStream_t st) {
    if (a.B <= 0 || a.rows_out <= 0) return FS2_OK;
    if ((long long)a.T * a.len_scale > a.rows_out || (long long)a.T * a.len_scale * a.in_stride > a.rows_in) return FS2_ERR_SHAPE;
    return dtype == FS2_BF16 ? fd_conv_launch_t<bf16>(a, cin, st) : fd_conv_launch_t<float>(a, cin, st);
}

template <typename T>
int fd_lvc_launch_t(const FdLvcArgs& a, int hop, hipStream_t st) {
    const int tiles = (a.T * hop + FD_TILE - 1) / FD_TILE;
    const dim3 grid((unsigned)(tiles * a.B));
    if (hop == 8) hipLaunchKernelGGL((fd_lvc_kernel<T, 8>), grid, dim3(256), 0, st, a);
    else if (hop == 64) hipLaunchKernelGGL((fd_lvc_kernel<T, 64>), grid, dim3(256), 0, st, a);
    else if (hop == 256) hipLaunchKernelGGL((fd_lvc_kernel<T, 256>), grid, dim3(256), 0, st, a);
    else return FS2_ERR_SHAPE;
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

int fd_lvc_launch(int dtype, const FdLvcArgs& a, int hop, hipStream_t st) {
    if (a.B <= 0 || a.T <= 0) return FS2_OK;
    return dtype == FS2_BF16 ? fd_lvc_launch_t<bf16>(a, hop, st) : fd_lvc_launch_t<float>(a, hop, st);
}

// ---- host side: weights ----
// position of the reference's kernels[layer, c, o, k] inside a frame's FD_KW values: fragment order of fd_lvc_kernel
// ([layer][step = k * NKC + c / KE][n-tile][lane = ((c % KE) / E16) * 16 + row][c % E16]); output channel o = half * 32 + q * 8 + j * 4 + r
// sits in n-tile half * 2 + j at row q * 4 + r, so that a lane ends with 8 consecutive channels of both gate halves
long long fd_kernel_index(int dtype, int layer, int c, int o, int k) {
    const int KE = dtype == FS2_BF16 ? 32 : 16, E16 = dtype == FS2_BF16 ? 8 : 4, NKC = FD_CH / KE;
    const int oc = o % 32, tile = (o / 32) * 2 + (oc % 8) / 4, row = (oc / 8) * 4 + oc % 4;
    const int step = k * NKC + c / KE, lane = ((c % KE) / E16) * 16 + row;
    return (long long)layer * FD_KL + (((long long)step * 4 + tile) * 64 + lane) * E16 + c % E16;
}

// columns per wave pass of fd_conv_kernel: 16 * NT (fd_conv_launch_t picks NT the same way)
int fd_conv_nt(int n, int cin_pad) { return n == 32 && cin_pad == 32 ? 2 : 4; }

// w: n rows, each (cin, taps) as torch lays a Conv1d weight out -> [n / 16][step = tap * (cin_pad / KE) + kc][lane][E16] of the dtype.
// Inside a group of 16 * NT output columns, column q * 4 * NT + j * 4 + r sits in MFMA tile j at row q * 4 + r, so that the lane
// that ends with rows q * 4 .. q * 4 + 3 of every tile owns 4 * NT consecutive columns (one contiguous store per sample row).
void fd_pack_conv(const float* w, int n, int cin, int cin_pad, int taps, int dtype, unsigned char* dst) {
    const int KE = dtype == FS2_BF16 ? 32 : 16, E16 = dtype == FS2_BF16 ? 8 : 4, NKC = cin_pad / KE, nsteps = taps * NKC;
    const int NT = fd_conv_nt(n, cin_pad);
    for (int nt = 0; nt < n / 16; ++nt)
        for (int step = 0; step < nsteps; ++step)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < E16; ++e) {
                    const int tap = step / NKC, kc = step % NKC, fr = lane & 15, fg = lane >> 4;
                    const int c = kc * KE + fg * E16 + e;
                    const int row = (nt / NT) * 16 * NT + (fr / 4) * 4 * NT + (nt % NT) * 4 + fr % 4;
                    const float v = c < cin ? w[((size_t)row * cin + c) * taps + tap] : 0.f;
                    const size_t at = (((size_t)nt * nsteps + step) * 64 + lane) * E16 + e;
                    if (dtype == FS2_BF16) ((bf16*)dst)[at] = f32_to_bf16(v);
                    else ((float*)dst)[at] = v;
                }
}

struct FdConvW {  // a packed conv on the device
    size_t w = 0, b = 0;  // byte offsets into the weight block
    int n = 0, cin_pad = 0, taps = 0;
};

const int kFdRatios[3] = {8, 8, 4};
const int kFdHops[3] = {8, 64, 256};
const int kFdDown[3] = {4, 8, 8};  // upsample_ratios reversed (FastDiff.py:69)

}  // namespace
}  // namespace fs2

using namespace fs2;

struct fs2_fd : ErrorBase {
    int dtype = FS2_F32;
    bool ready = false, finalized = false;
    int chunk_limit = 0;
    WeightStore w;
    DevAllocs allocs;
    unsigned char* dev = nullptr;  // one block: every packed tensor
    // packed convs
    FdConvW db_res[3], db_conv[3][3];
    FdConvW kp_in[3], kp_res[3][6], kp_kernel[3], kp_bias[3];
    FdConvW up[3], lvc_conv[3][4];
    size_t first_w = 0, first_b = 0, final_w = 0, final_b = 0;
    // the step conditioning stays on the host (fc_t1, fc_t2, fc_t): 240 constants of (weights, step)
    std::vector<float> fc1_w, fc1_b, fc2_w, fc2_b, fct_w[3], fct_b[3];
    std::map<int, std::vector<FdOffsets>> sched_offsets;  // N -> per step n, per block
};

namespace {

bool fd_config_ok(int inner, int cond, const int32_t* ratios, int n_ratios, int layers, int lvc_k, int hid, int kp_k, int e_in, int e_mid,
                  int e_out) {
    return inner == FD_CH && cond == FD_MEL && ratios && n_ratios == 3 && ratios[0] == 8 && ratios[1] == 8 && ratios[2] == 4 &&
           layers == 4 && lvc_k == 3 && hid == FD_HID && kp_k == 3 && e_in == 128 && e_mid == 512 && e_out == 512;
}

void fd_add_conv(fs2_fd* h, const std::string& name, int n, int cin, int k) {
    h->w.expect(name + ".weight", {n, cin, k});
    h->w.expect(name + ".bias", {n});
}

// fc_t(swish(fc_t2(swish(fc_t1(emb(step)))))) per LVC block, in double (FastDiff.py:120-123, util.py:318-343, modules.py:202)
void fd_step_offsets(const fs2_fd* h, float step, FdOffsets out[3]) {
    double emb[128], a[512], b[512];
    for (int j = 0; j < 64; ++j) {
        const double f = std::exp(-(double)j * (std::log(10000.0) / 63.0));
        emb[j] = std::sin((double)step * f);
        emb[64 + j] = std::cos((double)step * f);
    }
    for (int o = 0; o < 512; ++o) {
        double s = h->fc1_b[o];
        for (int i = 0; i < 128; ++i) s += (double)h->fc1_w[(size_t)o * 128 + i] * emb[i];
        a[o] = s / (1.0 + std::exp(-s));
    }
    for (int o = 0; o < 512; ++o) {
        double s = h->fc2_b[o];
        for (int i = 0; i < 512; ++i) s += (double)h->fc2_w[(size_t)o * 512 + i] * a[i];
        b[o] = s / (1.0 + std::exp(-s));
    }
    for (int n = 0; n < 3; ++n)
        for (int o = 0; o < FD_MEL; ++o) {
            double s = h->fct_b[n][o];
            for (int i = 0; i < 512; ++i) s += (double)h->fct_w[n][(size_t)o * 512 + i] * b[i];
            out[n].v[o] = (float)s;
        }
}

// The reference's float32 arithmetic, operation by operation (FastDiff.py:88-89, 158-172; util.py:187-204, 276-316).
int fd_schedule(int N, float* beta, float* alpha, float* sigma, float* step) {
#pragma clang fp contract(off)
    static const double b8[8] = {6.689325005027058e-07, 1.0033881153503899e-05, 0.00015496854030061513, 0.002387222135439515,
                                 0.035597629845142365,  0.3681158423423767,     0.4735414385795593,     0.5};
    static const double b6[6] = {1.7838445955931093e-06, 2.7984189728158526e-05, 0.00043231004383414984,
                                 0.006634317338466644,   0.09357017278671265,    0.6000000238418579};
    static const double b4[4] = {3.2176e-04, 2.5743e-03, 2.5376e-02, 7.0414e-01};
    static const double b3[3] = {9.0000e-05, 9.0000e-03, 6.0000e-01};
    const double* src = N == 8 ? b8 : N == 6 ? b6 : N == 4 ? b4 : N == 3 ? b3 : nullptr;
    if (!src) return FS2_ERR_SHAPE;
    // the training schedule: torch.linspace(1e-6, 0.01, 1000) in float32, then alpha-bar
    float ta[1000];
    {
        const float start = 1e-6f, end = 0.01f;
        const float stp = (end - start) / 999.f;
        for (int i = 0; i < 1000; ++i) {
            const float b = i < 500 ? start + stp * (float)i : end - stp * (float)(999 - i);
            ta[i] = 1.f - b;
        }
        for (int i = 1; i < 1000; ++i) ta[i] *= ta[i - 1];
        for (int i = 0; i < 1000; ++i) ta[i] = sqrtf(ta[i]);
    }
    float a[8], s[8], b[8];
    for (int n = 0; n < N; ++n) {
        b[n] = (float)src[n];
        a[n] = 1.f - b[n];
        s[n] = b[n];
    }
    for (int n = 1; n < N; ++n) {
        a[n] *= a[n - 1];
        const float r = (1.f - a[n - 1]) / (1.f - a[n]);
        s[n] *= r;
    }
    for (int n = 0; n < N; ++n) {
        a[n] = sqrtf(a[n]);
        s[n] = sqrtf(s[n]);
    }
    for (int n = 0; n < N; ++n) {
        float st = -1.f;
        if (a[n] < ta[999]) st = 999.f;
        else if (a[n] > ta[0]) st = 0.f;
        else
            for (int t = 0; t < 999; ++t)
                if (ta[t + 1] <= a[n] && a[n] <= ta[t]) {
                    float d = ta[t] - a[n];
                    d /= ta[t] - ta[t + 1];
                    st = (float)((double)t + (double)d);
                    break;
                }
        if (st < 0.f) return FS2_ERR_SHAPE;  // (the reference would drop the step: none of the four tabulated schedules does)
        if (beta) beta[n] = b[n];
        if (alpha) alpha[n] = a[n];
        if (sigma) sigma[n] = s[n];
        if (step) step[n] = st;
    }
    return FS2_OK;
}

// ---- workspace layout of one chunk of Bc utterances of T frames ----
struct FdWs {
    size_t cond, kpa, kpb, kpc, K, kb, h0, h1, h2, h3, d0, d1, d2, xa, xb, y, xs, eps, total;
};

FdWs fd_layout(int dtype, size_t Bc, size_t T) {
    const size_t e = elem_bytes(dtype), S = T * FD_HOP;
    FdWs w{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += al(bytes); return o; };
    w.cond = take(Bc * T * FD_MELP * e);
    w.kpa = take(Bc * T * FD_HID * e);
    w.kpb = take(Bc * T * FD_HID * e);
    w.kpc = take(Bc * T * FD_HID * e);
    w.K = take(Bc * T * FD_KW * e);
    w.kb = take(Bc * T * FD_NB * e);
    w.h0 = take(Bc * S * FD_CH * e);
    w.h1 = take(Bc * (S / 4) * FD_CH * e);
    w.h2 = take(Bc * (S / 32) * FD_CH * e);
    w.h3 = take(Bc * T * FD_CH * e);
    w.d0 = take(Bc * (S / 4) * FD_CH * e);
    w.d1 = take(Bc * (S / 4) * FD_CH * e);
    w.d2 = take(Bc * (S / 4) * FD_CH * e);
    w.xa = take(Bc * S * FD_CH * e);
    w.xb = take(Bc * (S / 4) * FD_CH * e);
    w.y = take(Bc * S * FD_CH * e);
    w.xs = take(Bc * S * 4);
    w.eps = take(Bc * S * 4);
    w.total = at;
    return w;
}

int fd_chunk(const fs2_fd* h, int B, int T) {
    if (h->chunk_limit > 0) return B < h->chunk_limit ? B : h->chunk_limit;
    const size_t one = fd_layout(h->dtype, 1, (size_t)T).total, cap = (size_t)2 << 30;
    const size_t fit = cap / one;
    return (int)(fit < 1 ? 1 : (fit > (size_t)B ? (size_t)B : fit));
}

FdConvArgs fd_conv_args(const fs2_fd* h, const FdConvW& w, const void* x, void* out, const int* lengths, int B, int T, int rows_in,
                        int rows_out, int len_scale, int in_stride, int dil, float in_slope, float out_slope) {
    FdConvArgs a{};
    a.x = x; a.w = h->dev + w.w; a.bias = (const float*)(h->dev + w.b); a.out = out; a.lengths = lengths;
    a.B = B; a.T = T; a.rows_in = rows_in; a.rows_out = rows_out; a.len_scale = len_scale;
    a.in_stride = in_stride; a.taps = w.taps; a.dil = dil; a.n = w.n; a.in_slope = in_slope; a.out_slope = out_slope;
    return a;
}

// DiffusionDBlock (modules.py:127-138): x (B, rows_out * f, 32) -> out (B, rows_out, 32); tmp = 3 x (B, rows_out, 32)
int fd_dblock(const fs2_fd* h, int blk, const void* x, void* out, void* tmp, const int* lengths, int B, int T, int rows_out,
              int len_scale, hipStream_t st) {
    const int f = kFdDown[blk], rows_in = rows_out * f;
    const size_t tb = (size_t)B * rows_out * FD_CH * elem_bytes(h->dtype);
    void* r = tmp; void* a = (char*)tmp + tb; void* b = (char*)tmp + 2 * tb;
    FS2_TRY(fd_conv_launch(h->dtype, fd_conv_args(h, h->db_res[blk], x, r, lengths, B, T, rows_in, rows_out, len_scale, f, 1, 1.f, 1.f), FD_CH, st));
    FS2_TRY(fd_conv_launch(h->dtype, fd_conv_args(h, h->db_conv[blk][0], x, a, lengths, B, T, rows_in, rows_out, len_scale, f, 1, 0.2f, 1.f), FD_CH, st));
    FS2_TRY(fd_conv_launch(h->dtype, fd_conv_args(h, h->db_conv[blk][1], a, b, lengths, B, T, rows_out, rows_out, len_scale, 1, 2, 0.2f, 1.f), FD_CH, st));
    FdConvArgs c = fd_conv_args(h, h->db_conv[blk][2], b, out, lengths, B, T, rows_out, rows_out, len_scale, 1, 4, 0.2f, 1.f);
    c.add1 = r;
    return fd_conv_launch(h->dtype, c, FD_CH, st);
}

template <typename T>
void fd_cond_launch(const float* mel, const FdOffsets& off, void* cond, const int* lengths, int B, int Tf, hipStream_t st) {
    const size_t n = (size_t)B * Tf * FD_MELP;
    hipLaunchKernelGGL((fd_cond_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mel, off, (T*)cond, lengths, B, Tf);
}

// kernel predictor of LVC block n (modules.py:320-343) on cond = mel + off: K (B, T, 24576), kb (B, T, 256)
int fd_predict(const fs2_fd* h, int n, const float* mel, const FdOffsets& off, const int* lengths, int B, int T, char* ws, const FdWs& L,
               void* K, void* kb, hipStream_t st) {
    if (h->dtype == FS2_BF16) fd_cond_launch<bf16>(mel, off, ws + L.cond, lengths, B, T, st);
    else fd_cond_launch<float>(mel, off, ws + L.cond, lengths, B, T, st);
    auto conv = [&](const FdConvW& w, const void* x, void* out, float out_slope, const void* add2, int cin) {
        FdConvArgs a = fd_conv_args(h, w, x, out, lengths, B, T, T, T, 1, 1, 1, 1.f, out_slope);
        a.add2 = add2;
        return fd_conv_launch(h->dtype, a, cin, st);
    };
    void* ka = ws + L.kpa; void* kp[2] = {ws + L.kpb, ws + L.kpc};
    FS2_TRY(conv(h->kp_in[n], ws + L.cond, ka, 0.1f, nullptr, FD_MELP));
    const void* cur = ka;
    for (int i = 0; i < 6; ++i) {
        FS2_TRY(conv(h->kp_res[n][i], cur, kp[i & 1], 0.1f, i == 5 ? ka : nullptr, FD_HID));
        cur = kp[i & 1];
    }
    FS2_TRY(conv(h->kp_kernel[n], cur, K, 1.f, nullptr, FD_HID));
    return conv(h->kp_bias[n], cur, kb, 1.f, nullptr, FD_HID);
}

template <typename T>
void fd_ends_launch(bool first, const fs2_fd* h, const void* in, void* out, const int* lengths, int B, int Tf, hipStream_t st) {
    const int S = Tf * FD_HOP;
    if (first)
        hipLaunchKernelGGL((fd_first_conv_kernel<T>), dim3((unsigned)(((S + 31) / 32) * B)), dim3(256), 0, st, (const float*)in,
                           (const float*)(h->dev + h->first_w), (const float*)(h->dev + h->first_b), (T*)out, lengths, B, Tf);
    else
        hipLaunchKernelGGL((fd_final_conv_kernel<T>), dim3((unsigned)(((S + 255) / 256) * B)), dim3(256), 0, st, (const T*)in,
                           (const float*)(h->dev + h->final_w), (const float*)(h->dev + h->final_b), (float*)out, lengths, B, Tf);
}

// one eps evaluation of a chunk (FastDiff.py:120-135): 71 launches
int fd_eps(const fs2_fd* h, const float* x, const float* mel, const int* lengths, const FdOffsets off[3], float* eps, char* ws,
           const FdWs& L, int B, int T, hipStream_t st) {
    const int S = T * FD_HOP;
    const bool b16 = h->dtype == FS2_BF16;
    if (b16) fd_ends_launch<bf16>(true, h, x, ws + L.h0, lengths, B, T, st);
    else fd_ends_launch<float>(true, h, x, ws + L.h0, lengths, B, T, st);
    FS2_TRY(fd_dblock(h, 0, ws + L.h0, ws + L.h1, ws + L.d0, lengths, B, T, S / 4, 64, st));
    FS2_TRY(fd_dblock(h, 1, ws + L.h1, ws + L.h2, ws + L.d0, lengths, B, T, S / 32, 8, st));
    FS2_TRY(fd_dblock(h, 2, ws + L.h2, ws + L.h3, ws + L.d0, lengths, B, T, T, 1, st));
    const void* cur = ws + L.h3;
    int cur_scale = 1;  // rows of `cur` per frame
    void* const xbuf[3] = {ws + L.xa, ws + L.xb, ws + L.xa};
    void* const down[3] = {ws + L.h2, ws + L.h1, ws + L.h0};  // reversed(downsample), FastDiff.py:131
    for (int n = 0; n < 3; ++n) {
        const int hop = kFdHops[n], rows = T * hop;
        FS2_TRY(fd_predict(h, n, mel, off[n], lengths, B, T, ws, L, ws + L.K, ws + L.kb, st));
        // x = upsample(lrelu(x)); x += audio_down (the first of the four adds)
        FdConvArgs u = fd_conv_args(h, h->up[n], cur, xbuf[n], lengths, B, T, T * cur_scale, T * cur_scale, cur_scale, 1, 1, 0.2f, 1.f);
        u.add1 = down[n];
        FS2_TRY(fd_conv_launch(h->dtype, u, FD_CH, st));
        for (int i = 0, dil = 1; i < 4; ++i, dil *= 3) {
            FS2_TRY(fd_conv_launch(h->dtype, fd_conv_args(h, h->lvc_conv[n][i], xbuf[n], ws + L.y, lengths, B, T, rows, rows, hop, 1, dil, 0.2f, 0.2f),
                                  FD_CH, st));
            FdLvcArgs a{ws + L.y, ws + L.K, ws + L.kb, xbuf[n], i < 3 ? down[n] : nullptr, xbuf[n], lengths, B, T, i};
            FS2_TRY(fd_lvc_launch(h->dtype, a, hop, st));
        }
        cur = xbuf[n];
        cur_scale = hop;
    }
    if (b16) fd_ends_launch<bf16>(false, h, cur, eps, lengths, B, T, st);
    else fd_ends_launch<float>(false, h, cur, eps, lengths, B, T, st);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

int fd_call_checks(fs2_fd* h, const char* what, const void* ws, size_t ws_bytes, int B, int T) {
    if (!h->finalized) return h->fail(FS2_ERR_STATE, "%s before fs2_fd_finalize", what);
    if (B < 1 || T < 1) return h->fail(FS2_ERR_ARG, "B = %d, T = %d: both must be at least 1", B, T);
    if (T > 8192) return h->fail(FS2_ERR_SHAPE, "T = %d frames: at most 8192 per utterance", T);
    const int Bc = fd_chunk(h, B, T);
    const size_t need = fd_layout(h->dtype, (size_t)Bc, (size_t)T).total;
    if ((size_t)Bc * ((T * FD_HOP + 31) / 32) > 0x7fffffffull) return h->fail(FS2_ERR_SHAPE, "a chunk of %d utterances x %d frames exceeds the grid", Bc, T);
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 255))
        return h->fail(FS2_ERR_NOMEM, "workspace of %zu bytes, %zu needed (256-byte aligned)", ws_bytes, need);
    return FS2_OK;
}

}  // namespace

extern "C" {

int fs2_fd_supported(int32_t inner_channels, int32_t cond_channels, const int32_t* upsample_ratios, int32_t n_ratios, int32_t lvc_layers,
                     int32_t lvc_kernel, int32_t kpnet_hidden, int32_t kpnet_conv, int32_t embed_in, int32_t embed_mid, int32_t embed_out) {
    return fd_config_ok(inner_channels, cond_channels, upsample_ratios, n_ratios, lvc_layers, lvc_kernel, kpnet_hidden, kpnet_conv, embed_in,
                        embed_mid, embed_out) ? 1 : 0;
}

int fs2_fd_create(int32_t abi_version, int32_t dtype, int32_t inner_channels, int32_t cond_channels, const int32_t* upsample_ratios,
                  int32_t n_ratios, int32_t lvc_layers, int32_t lvc_kernel, int32_t kpnet_hidden, int32_t kpnet_conv, int32_t embed_in,
                  int32_t embed_mid, int32_t embed_out, fs2_fd** out) {
    if (!out) return FS2_ERR_ARG;
    *out = nullptr;
    fs2_fd* h = new (std::nothrow) fs2_fd();
    if (!h) return FS2_ERR_NOMEM;
    *out = h;
    if (abi_version != FS2_ABI_VERSION) return h->fail(FS2_ERR_ARG, "abi_version %d, this library is %d", abi_version, FS2_ABI_VERSION);
    if (dtype != FS2_F32 && dtype != FS2_BF16) return h->fail(FS2_ERR_ARG, "dtype %d: FS2_F32 or FS2_BF16", dtype);
    if (!fd_config_ok(inner_channels, cond_channels, upsample_ratios, n_ratios, lvc_layers, lvc_kernel, kpnet_hidden, kpnet_conv, embed_in,
                      embed_mid, embed_out))
        return h->fail(FS2_ERR_SHAPE,
                     "the FastDiff kernels cover the reference's default architecture only: inner 32, cond 80, upsample_ratios [8, 8, 4], "
                     "4 LVC layers of kernel 3, kpnet 64 / 3, step embedding 128 / 512 / 512");
    h->dtype = dtype;
    fd_add_conv(h, "first_audio_conv", FD_CH, 1, 7);
    h->w.expect("fc_t1.weight", {512, 128}); h->w.expect("fc_t1.bias", {512});
    h->w.expect("fc_t2.weight", {512, 512}); h->w.expect("fc_t2.bias", {512});
    for (int n = 0; n < 3; ++n) {
        const std::string d = "downsample." + std::to_string(n), l = "lvc_blocks." + std::to_string(n);
        fd_add_conv(h, d + ".residual_dense", FD_CH, FD_CH, 1);
        for (int i = 0; i < 3; ++i) fd_add_conv(h, d + ".conv." + std::to_string(i), FD_CH, FD_CH, 3);
        h->w.expect(l + ".upsample.weight", {FD_CH, FD_CH, 2 * kFdRatios[n]});
        h->w.expect(l + ".upsample.bias", {FD_CH});
        fd_add_conv(h, l + ".kernel_predictor.input_conv.0", FD_HID, FD_MEL, 5);
        for (int i : {1, 3, 6, 8, 11, 13}) fd_add_conv(h, l + ".kernel_predictor.residual_conv." + std::to_string(i), FD_HID, FD_HID, 3);
        fd_add_conv(h, l + ".kernel_predictor.kernel_conv", FD_KW, FD_HID, 3);
        fd_add_conv(h, l + ".kernel_predictor.bias_conv", FD_NB, FD_HID, 3);
        h->w.expect(l + ".fc_t.weight", {FD_MEL, 512}); h->w.expect(l + ".fc_t.bias", {FD_MEL});
        for (int i = 0; i < 4; ++i) fd_add_conv(h, l + ".convs." + std::to_string(i), FD_CH, FD_CH, 3);
    }
    fd_add_conv(h, "final_conv.0", 1, FD_CH, 7);
    h->ready = true;
    return FS2_OK;
}

int fs2_fd_destroy(fs2_fd* h) {
    if (!h) return FS2_ERR_ARG;
    delete h;
    return FS2_OK;
}

const char* fs2_fd_last_error(const fs2_fd* h) { return h ? h->err : "null fastdiff handle"; }

int fs2_fd_load_weight(fs2_fd* h, const char* name, const float* host_data, const int64_t* shape, int32_t ndim) {
    if (!h) return FS2_ERR_ARG;
    if (!h->ready) return h->fail(FS2_ERR_STATE, "fs2_fd_create did not succeed");
    if (h->finalized) return h->fail(FS2_ERR_STATE, "fs2_fd_load_weight after fs2_fd_finalize");
    if (!name || !host_data || !shape || ndim < 1) return h->fail(FS2_ERR_ARG, "name, host_data and shape must not be null");
    return h->w.load(*h, name, host_data, shape, ndim);
}

int fs2_fd_finalize(fs2_fd* h) {
    if (!h) return FS2_ERR_ARG;
    if (!h->ready) return h->fail(FS2_ERR_STATE, "fs2_fd_create did not succeed");
    if (h->finalized) return h->fail(FS2_ERR_STATE, "fs2_fd_finalize called twice");
    if (const char* missing = h->w.first_missing()) return h->fail(FS2_ERR_WEIGHT, "missing weight '%s'", missing);
    const int dt = h->dtype;
    const size_t e = elem_bytes(dt);
    WeightBlock wb;
    std::vector<unsigned char>& blk = wb.host;
    auto grow = [&](size_t bytes) { return wb.grow(bytes, 256); };
    auto W = [&](const std::string& n) -> const std::vector<float>& { return h->w.at(n).data; };
    // rows[i] = the source row (of w and bias) that packed row i holds
    auto pack = [&](const float* w, const float* bias, int n, int cin, int cin_pad, int taps) {
        FdConvW c;
        c.n = n; c.cin_pad = cin_pad; c.taps = taps;
        c.w = grow((size_t)n * cin_pad * taps * e);
        fd_pack_conv(w, n, cin, cin_pad, taps, dt, blk.data() + c.w);
        c.b = grow((size_t)n * 4);
        std::memcpy(blk.data() + c.b, bias, (size_t)n * 4);
        return c;
    };
    auto conv = [&](const std::string& name, int n, int cin, int cin_pad, int taps) {
        return pack(W(name + ".weight").data(), W(name + ".bias").data(), n, cin, cin_pad, taps);
    };
    h->first_w = grow(FD_CH * 7 * 4); std::memcpy(blk.data() + h->first_w, W("first_audio_conv.weight").data(), FD_CH * 7 * 4);
    h->first_b = grow(FD_CH * 4); std::memcpy(blk.data() + h->first_b, W("first_audio_conv.bias").data(), FD_CH * 4);
    h->final_w = grow(FD_CH * 7 * 4); std::memcpy(blk.data() + h->final_w, W("final_conv.0.weight").data(), FD_CH * 7 * 4);
    h->final_b = grow(4); std::memcpy(blk.data() + h->final_b, W("final_conv.0.bias").data(), 4);
    for (int n = 0; n < 3; ++n) {
        const std::string d = "downsample." + std::to_string(n), l = "lvc_blocks." + std::to_string(n), kp = l + ".kernel_predictor";
        h->db_res[n] = conv(d + ".residual_dense", FD_CH, FD_CH, FD_CH, 1);
        for (int i = 0; i < 3; ++i) h->db_conv[n][i] = conv(d + ".conv." + std::to_string(i), FD_CH, FD_CH, FD_CH, 3);
        for (int i = 0; i < 4; ++i) h->lvc_conv[n][i] = conv(l + ".convs." + std::to_string(i), FD_CH, FD_CH, FD_CH, 3);
        h->kp_in[n] = conv(kp + ".input_conv.0", FD_HID, FD_MEL, FD_MELP, 5);
        const int ri[6] = {1, 3, 6, 8, 11, 13};
        for (int i = 0; i < 6; ++i) h->kp_res[n][i] = conv(kp + ".residual_conv." + std::to_string(ri[i]), FD_HID, FD_HID, FD_HID, 3);
        h->kp_bias[n] = conv(kp + ".bias_conv", FD_NB, FD_HID, FD_HID, 3);
        {   // kernel_conv: row fd_kernel_index(layer, c, o, k) <- the reference's channel ((layer * 32 + c) * 64 + o) * 3 + k
            const auto& w = W(kp + ".kernel_conv.weight");
            const auto& b = W(kp + ".kernel_conv.bias");
            std::vector<float> pw((size_t)FD_KW * FD_HID * 3), pb(FD_KW);
            for (int layer = 0; layer < 4; ++layer)
                for (int c = 0; c < FD_CH; ++c)
                    for (int o = 0; o < 64; ++o)
                        for (int k = 0; k < 3; ++k) {
                            const size_t src = ((size_t)(layer * FD_CH + c) * 64 + o) * 3 + k, dst = (size_t)fd_kernel_index(dt, layer, c, o, k);
                            std::memcpy(&pw[dst * FD_HID * 3], &w[src * FD_HID * 3], FD_HID * 3 * 4);
                            pb[dst] = b[src];
                        }
            h->kp_kernel[n] = pack(pw.data(), pb.data(), FD_KW, FD_HID, FD_HID, 3);
        }
        {   // ConvTranspose1d(k = 2r, stride r, pad r/2) as a 3-tap conv: out[t*r + p] takes x[t + tp - 1] through w[.., p + r/2 + (1 - tp) * r]
            const int r = kFdRatios[n];
            const auto& w = W(l + ".upsample.weight");  // (Cin, Cout, 2r)
            const auto& b = W(l + ".upsample.bias");
            std::vector<float> w3((size_t)r * FD_CH * FD_CH * 3, 0.f), b3((size_t)r * FD_CH);
            for (int p = 0; p < r; ++p)
                for (int co = 0; co < FD_CH; ++co) {
                    b3[p * FD_CH + co] = b[co];
                    for (int ci = 0; ci < FD_CH; ++ci)
                        for (int tp = 0; tp < 3; ++tp) {
                            const int kk = p + r / 2 + (1 - tp) * r;
                            if (kk >= 0 && kk < 2 * r) w3[((size_t)(p * FD_CH + co) * FD_CH + ci) * 3 + tp] = w[((size_t)ci * FD_CH + co) * 2 * r + kk];
                        }
                }
            h->up[n] = pack(w3.data(), b3.data(), r * FD_CH, FD_CH, FD_CH, 3);
        }
        h->fct_w[n] = W(l + ".fc_t.weight"); h->fct_b[n] = W(l + ".fc_t.bias");
    }
    h->fc1_w = W("fc_t1.weight"); h->fc1_b = W("fc_t1.bias");
    h->fc2_w = W("fc_t2.weight"); h->fc2_b = W("fc_t2.bias");
    // the offsets of the four tabulated schedules: constants of (weights, N)
    for (int N : {3, 4, 6, 8}) {
        float steps[8];
        if (fd_schedule(N, nullptr, nullptr, nullptr, steps) != FS2_OK) return h->fail(FS2_ERR_SHAPE, "schedule N = %d does not map to steps", N);
        std::vector<FdOffsets> v((size_t)N * 3);
        for (int n = 0; n < N; ++n) fd_step_offsets(h, steps[n], &v[(size_t)n * 3]);
        h->sched_offsets[N] = v;
    }
    FS2_TRY(wb.upload(*h, h->allocs, (void**)&h->dev));
    h->w.drop();
    h->finalized = true;
    return FS2_OK;
}

int32_t fs2_fd_hop(const fs2_fd* h) { return h && h->ready ? FD_HOP : 0; }
int32_t fs2_fd_tile_rows(const fs2_fd* h) { return h && h->ready ? FD_TILE : 0; }

int fs2_fd_launches(const fs2_fd* h, int32_t N) {
    if (!h || !h->ready || N < 0) return 0;
    const int eps = 1 + 3 * 4 + 3 * (1 + 9 + 1 + 4 * 2) + 1;  // 71: first conv, DBlocks, per block (cond, 9 predictor convs, convT, 4 x (conv, LVC)), final conv
    return N == 0 ? eps : N * (eps + 1) + 1;
}

int fs2_fd_set_chunk(fs2_fd* h, int32_t max_utterances) {
    if (!h) return FS2_ERR_ARG;
    if (max_utterances < 0) return h->fail(FS2_ERR_ARG, "max_utterances = %d", max_utterances);
    h->chunk_limit = max_utterances;
    return FS2_OK;
}

int fs2_fd_workspace_bytes(const fs2_fd* h, int32_t B, int32_t T, size_t* bytes) {
    if (!h || !bytes || B < 1 || T < 1) return FS2_ERR_ARG;
    *bytes = fd_layout(h->dtype, (size_t)fd_chunk(h, B, T), (size_t)T).total;
    return FS2_OK;
}

int fs2_fd_schedule(int32_t N, float* beta, float* alpha, float* sigma, float* step) { return fd_schedule(N, beta, alpha, sigma, step); }

int fs2_fd_denoise(fs2_fd* h, const float* x, const float* mel, const int32_t* lengths, float step, float* eps, void* workspace,
                   size_t workspace_bytes, int32_t B, int32_t T, void* hip_stream) {
    if (!h) return FS2_ERR_ARG;
    FS2_TRY(fd_call_checks(h, "fs2_fd_denoise", workspace, workspace_bytes, B, T));
    if (!x || !mel || !eps) return h->fail(FS2_ERR_ARG, "x, mel and eps must not be null");
    if (!(step >= 0.f) || !std::isfinite(step)) return h->fail(FS2_ERR_ARG, "step must be finite and non-negative");
    FdOffsets off[3];
    fd_step_offsets(h, step, off);
    const int Bc = fd_chunk(h, B, T);
    const FdWs L = fd_layout(h->dtype, (size_t)Bc, (size_t)T);
    const size_t S = (size_t)T * FD_HOP;
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = B - b0 < Bc ? B - b0 : Bc;
        const int st = fd_eps(h, x + b0 * S, mel + (size_t)b0 * T * FD_MEL, lengths ? lengths + b0 : nullptr, off, eps + b0 * S,
                              (char*)workspace, L, nb, T, (hipStream_t)hip_stream);
        if (st != FS2_OK) return h->fail(st, "launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    return FS2_OK;
}

int fs2_fd_sample(fs2_fd* h, const float* mel, const int32_t* lengths, const float* noise, int32_t N, float* wav, void* workspace,
                  size_t workspace_bytes, int32_t B, int32_t T, void* hip_stream) {
    if (!h) return FS2_ERR_ARG;
    float beta[8], alpha[8], sigma[8], steps[8];
    if (fd_schedule(N, beta, alpha, sigma, steps) != FS2_OK)
        return h->fail(FS2_ERR_SHAPE, "N = %d reverse steps: the tabulated schedules are 3, 4, 6 and 8", N);
    FS2_TRY(fd_call_checks(h, "fs2_fd_sample", workspace, workspace_bytes, B, T));
    if (!mel || !noise || !wav) return h->fail(FS2_ERR_ARG, "mel, noise and wav must not be null");
    const std::vector<FdOffsets>& offs = h->sched_offsets[N];
    hipStream_t st = (hipStream_t)hip_stream;
    const int Bc = fd_chunk(h, B, T);
    const FdWs L = fd_layout(h->dtype, (size_t)Bc, (size_t)T);
    const size_t S = (size_t)T * FD_HOP;
    char* ws = (char*)workspace;
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = B - b0 < Bc ? B - b0 : Bc;
        const int* len = lengths ? lengths + b0 : nullptr;
        const float* cmel = mel + (size_t)b0 * T * FD_MEL;
        float* xs = (float*)(ws + L.xs);
        float* eps = (float*)(ws + L.eps);
        const float* xin = noise + b0 * S;  // x_T
        for (int n = N - 1; n >= 0; --n) {
            const int s = fd_eps(h, xin, cmel, len, &offs[(size_t)n * 3], eps, ws, L, nb, T, st);
            if (s != FS2_OK) return h->fail(s, "launch failed: %s", hipGetErrorString(hipGetLastError()));
            float c1, d;
            {
#pragma clang fp contract(off)
                const float a2 = alpha[n] * alpha[n];
                c1 = beta[n] / sqrtf(1.f - a2);
                d = sqrtf(1.f - beta[n]);
            }
            const float* z = n > 0 ? noise + ((size_t)(N - n) * B + b0) * S : nullptr;
            hipLaunchKernelGGL(fd_update_kernel, dim3((unsigned)(((S + 255) / 256) * nb)), dim3(256), 0, st, xin, eps, z, xs, c1, d, sigma[n],
                               len, nb, T);
            xin = xs;
        }
        hipLaunchKernelGGL(fd_peak_scale_kernel, dim3((unsigned)nb), dim3(1024), 0, st, xs, wav + b0 * S, len, T);
    }
    return hipGetLastError() == hipSuccess ? FS2_OK : h->fail(FS2_ERR_HIP, "launch failed: %s", hipGetErrorString(hipGetLastError()));
}

int fs2_fd_predict_kernels(fs2_fd* h, int32_t block, const float* mel, const int32_t* lengths, float step, void* kernels, void* bias,
                           void* workspace, size_t workspace_bytes, int32_t B, int32_t T, void* hip_stream) {
    if (!h) return FS2_ERR_ARG;
    FS2_TRY(fd_call_checks(h, "fs2_fd_predict_kernels", workspace, workspace_bytes, B, T));
    if (block < 0 || block > 2 || !mel || !kernels || !bias) return h->fail(FS2_ERR_ARG, "block 0 .. 2; mel, kernels and bias must not be null");
    FdOffsets off[3];
    fd_step_offsets(h, step, off);
    const int Bc = fd_chunk(h, B, T);
    const FdWs L = fd_layout(h->dtype, (size_t)Bc, (size_t)T);
    const size_t e = elem_bytes(h->dtype);
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = B - b0 < Bc ? B - b0 : Bc;
        const int st = fd_predict(h, block, mel + (size_t)b0 * T * FD_MEL, off[block], lengths ? lengths + b0 : nullptr, nb, T, (char*)workspace, L,
                                  (char*)kernels + (size_t)b0 * T * FD_KW * e, (char*)bias + (size_t)b0 * T * FD_NB * e, (hipStream_t)hip_stream);
        if (st != FS2_OK) return h->fail(st, "launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    return FS2_OK;
}

int64_t fs2_fd_kernel_index(int32_t dtype, int32_t layer, int32_t in_channel, int32_t out_channel, int32_t k) {
    if ((dtype != FS2_F32 && dtype != FS2_BF16) || layer < 0 || layer > 3 || in_channel < 0 || in_channel >= FD_CH || out_channel < 0 ||
        out_channel >= 64 || k < 0 || k > 2)
        return -1;
    return fd_kernel_index(dtype, layer, in_channel, out_channel, k);
}

int fs2_op_lvc(int32_t dtype, int32_t hop, int32_t layer, const void* y, const void* kernels, const void* bias, const void* x,
               const void* add, void* out, const int32_t* lengths, int32_t B, int32_t T, void* hip_stream) {
    if (dtype != FS2_F32 && dtype != FS2_BF16) return FS2_ERR_ARG;
    if (!y || !kernels || !bias || !x || !out || layer < 0 || layer > 3 || B < 0 || T < 0) return FS2_ERR_ARG;
    if (hop != 8 && hop != 64 && hop != 256) return FS2_ERR_SHAPE;
    if ((long long)B * ((T * (long long)hop + FD_TILE - 1) / FD_TILE) > 0x7fffffffll) return FS2_ERR_SHAPE;
    FdLvcArgs a{y, kernels, bias, x, add, out, lengths, B, T, layer};
    return fd_lvc_launch(dtype, a, hop, (hipStream_t)hip_stream);
}

int fs2_op_fd_dblock(fs2_fd* h, int32_t block, const void* x, void* out, void* tmp, const int32_t* lengths, int32_t B, int32_t T,
                     void* hip_stream) {
    if (!h) return FS2_ERR_ARG;
    if (!h->finalized) return h->fail(FS2_ERR_STATE, "fs2_op_fd_dblock before fs2_fd_finalize");
    if (block < 0 || block > 2 || !x || !out || !tmp || B < 1 || T < 1 || T > 8192) return h->fail(FS2_ERR_ARG, "block 0 .. 2, x / out / tmp not null, B, T >= 1");
    static const int rows_per_frame[3] = {64, 8, 1};  // output rows per frame
    return fd_dblock(h, block, x, out, tmp, lengths, B, T, T * rows_per_frame[block], rows_per_frame[block], (hipStream_t)hip_stream);
}

}  // extern "C"
