// Stochastic duration predictor at inference (reference: litfass/third_party/stochastic_duration_predictor/sdp.py:249-349 with
// reverse=True, wrapped at litfass/fastspeech2/model.py:463-479): the VITS spline-flow predictor that replaces the conv + LayerNorm
// duration predictor when duration_stochastic=True.
//
//   g    = proj(DDS(pre(x), m)) * m                                       text conditioning, one launch (sdp_encoder_kernel)
//   z    = noise;  for flow in CF_n .. CF_2:  z = flip(z);  z = CF(z)     one launch per ConvFlow (sdp_flow_kernel)
//   logw = ((flip(z))[0] - translation[0]) * exp(-log_scale[0]) * m       the ElementwiseAffine, folded into the last flow launch
//                                                                        (n = 1: a row kernel, nothing else runs)
// DDS = 3 x [depth-wise conv k = 3, dilation 3^i on x * m -> LayerNorm -> GELU -> 1x1 conv -> LayerNorm -> GELU -> residual add].
//
// One workgroup (4 waves) keeps a 64-row tile of ONE utterance in LDS as two fp32 planes: X (the residual stream) and Y (the branch).
// A layer is
//   [VALU] a wave walks rows wv, wv + 4, ..: a lane owns 4 channels, reads X[i - d], X[i], X[i + d], the depth-wise sum, LayerNorm over the
//          row by whole-wave reductions, GELU -> Y[i]                      (rows outside the tile read zeros: they only feed halo rows)
//   [MFMA] Y (64 x 256) x W^T on v_mfma_f32_16x16x4_f32: wave wv owns output channels 64 wv .. + 63 of ALL rows (its weight fragments are
//          private, streamed from L2 in fragment order, 16 B per lane and four k-steps); accumulators seeded with the bias
//   [VALU] LayerNorm over the row needs the other waves' partial sums: two exchanges through LDS (sum, centred squares), GELU,
//          X += y for the rows inside the utterance.
// Rows at or beyond the utterance (pad mask set, or t outside [0, L)) are ZERO in X at all times: that is the reference's x * m on the
// conv input and its zero "same" padding at once.  One DDS reaches 1 + 3 + 9 = 13 rows to each side, so a tile finishes 64 - 26 = 38
// rows; tiles are anchored at multiples of 38 from the utterance's start.  Every sum (K order of the MFMA chain, the wave and cross-wave
// reduction trees) is fixed per row and independent of the row's place in the tile, of B and of L: the bits of logw do not depend on
// how an utterance is batched or padded.
// LDS: 2 planes x 64 rows x 260 floats (1040-byte rows: the MFMA operand reads of 16 rows spread over the banks) = 133 KB, + 3 KB.
// That, not the register file, bounds the tile height: 80 rows x 2 planes would be 166 KB.
// fp32 storage, accurate expf / logf / log1pf / erff / sqrtf everywhere: a duration is a decision.
#include "fs2_host.h"

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace fs2 {
namespace {

constexpr int SF = 256;                 // hidden channels (the only supported width)
constexpr int SR = 64;                  // tile rows
constexpr int SHALO = 13;               // 1 + 3 + 9
constexpr int SV = SR - 2 * SHALO;      // finished rows per tile
constexpr int SLD = SF + 4;             // floats per slab row
constexpr int SNB = 10, SNP = 3 * SNB - 1;  // spline bins, parameters per row
constexpr float S_LN_EPS = 1e-5f;

struct DdsW {
    const float* dw_w;  // [3 layers][3 taps][256]
    const float* dw_b;  // [3][256]
    const float* g1;    // [3][256]
    const float* b1;
    const float* pw;    // [3] packed 256 x 256 (pack_1x1)
    const float* pb;    // [3][256]
    const float* g2;
    const float* b2;
};

struct SdpEncArgs {
    const void* x;  // (B, L, H)
    int x_dtype;
    const uint8_t* pad;  // (B, L) 1 = pad
    float* g;            // (B, L, 256) out
    const float* pre_w;  // packed 256 x H
    const float* pre_b;
    DdsW d;
    const float* proj_w;  // packed 256 x 256
    const float* proj_b;
    int B, L, H;
};

struct SdpFlowArgs {
    const float* zin;  // (B, 2, L): the flow reads it flipped (x0 = channel 1, x1 = channel 0)
    float* zout;       // (B, 2, L) = cat(x0, x1') * m      (last == 0)
    float* logw;       // (B, L) = (x1' - ea_t) * exp(-ea_ls) * m  (last != 0: the flip and the ElementwiseAffine's channel 0)
    const float* g;    // (B, L, 256)
    const uint8_t* pad;
    const float* pre_w;  // [256]
    const float* pre_b;
    DdsW d;
    const float* proj_w;  // packed 32 x 256 (rows 29.. zero)
    const float* proj_b;  // [32]
    float ea_t, ea_ls;
    int last;
    int B, L;
};

__device__ inline float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__device__ inline float4 load_row4(const void* x, int dtype, size_t elem) {
    if (dtype == FS2_F32) return *(const float4*)((const float*)x + elem);
    const uint2 u = *(const uint2*)((const uint16_t*)x + elem);
    if (dtype == FS2_BF16)
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                           __uint_as_float(u.y & 0xffff0000u));
    const _Float16* hp = (const _Float16*)&u;
    return make_float4((float)hp[0], (float)hp[1], (float)hp[2], (float)hp[3]);
}

// acc[f][rf] (+)= W[oc][:] . src[row][:] for this wave's NF output fragments (16 channels each) and the tile's four row fragments.
// wp: this wave's first fragment in pack_1x1 order [fragment][kq][lane] x float4 (lane: oc = 16 f + (lane & 15), k = 16 kq + 4 (lane >> 4) + s).
// Lane (r = lane & 15, q = lane >> 4) ends up with rows 16 rf + r, channels 16 f + 4 q + j (j = the accumulator's component).
template <int NF>
__device__ inline void conv1x1(const float* src, const float4* __restrict__ wp, int KQ, int lane, f32x4_t (&acc)[NF][4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float* arow = src + (lane & 15) * SLD + (lane >> 4) * 4;
    // the next k-group's weight fragments (L2) and rows (LDS) are requested before this group's MFMAs (one wave per SIMD: nothing
    // else would cover their latency); the loop itself waits on the MFMAs (profiles/sdp.md)
    float4 wn[NF], an[4];
    auto fetch = [&](int kq) {
#pragma unroll
        for (int f = 0; f < NF; ++f) wn[f] = wp[((size_t)f * KQ + kq) * 64 + lane];
#pragma unroll
        for (int rf = 0; rf < 4; ++rf) an[rf] = *(const float4*)(arow + rf * 16 * SLD + kq * 16);
    };
    fetch(0);
    for (int kq = 0; kq < KQ; ++kq) {
        float4 w[NF], a[4];
#pragma unroll
        for (int f = 0; f < NF; ++f) w[f] = wn[f];
#pragma unroll
        for (int rf = 0; rf < 4; ++rf) a[rf] = an[rf];
        fetch(kq + 1 < KQ ? kq + 1 : kq);  // past the end: a harmless re-read instead of a branch
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            // the four row fragments take turns, so that no MFMA waits for the one issued just before it; an accumulator still
            // receives its k-steps in ascending order
#pragma unroll
            for (int rf = 0; rf < 4; ++rf) acc[f][rf] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[f].x, a[rf].x, acc[f][rf], 0, 0, 0);
#pragma unroll
            for (int rf = 0; rf < 4; ++rf) acc[f][rf] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[f].y, a[rf].y, acc[f][rf], 0, 0, 0);
#pragma unroll
            for (int rf = 0; rf < 4; ++rf) acc[f][rf] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[f].z, a[rf].z, acc[f][rf], 0, 0, 0);
#pragma unroll
            for (int rf = 0; rf < 4; ++rf) acc[f][rf] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[f].w, a[rf].w, acc[f][rf], 0, 0, 0);
        }
    }
#else
    (void)src; (void)wp; (void)KQ; (void)lane; (void)acc;
#endif
}

template <int NF>
__device__ inline void seed_bias(const float* bias, int lane, f32x4_t (&acc)[NF][4]) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const float4 b = *(const float4*)(bias + f * 16 + (lane >> 4) * 4);
#pragma unroll
        for (int rf = 0; rf < 4; ++rf) acc[f][rf] = (f32x4_t){b.x, b.y, b.z, b.w};
    }
}

// The three layers of a DilatedDepthSeparableConv on the tile in X (sdp.py:55-72).  All 256 threads; X rows outside the utterance are
// zero on entry and stay zero.  Y and red are scratch.  Ends with a barrier: X holds the output (x * m).
__device__ inline void dds_layers(float* X, float* Y, float (*red)[4 * SR], const unsigned char* valid, const DdsW& w, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    int dil = 1;
    for (int l = 0; l < 3; ++l, dil *= 3) {
        {   // depth-wise conv (dilation dil) -> LayerNorm -> GELU -> Y
            const int c = lane * 4;
            const float4 w0 = *(const float4*)(w.dw_w + (l * 3 + 0) * SF + c), w1 = *(const float4*)(w.dw_w + (l * 3 + 1) * SF + c),
                         w2 = *(const float4*)(w.dw_w + (l * 3 + 2) * SF + c), bb = *(const float4*)(w.dw_b + l * SF + c),
                         gg = *(const float4*)(w.g1 + l * SF + c), ee = *(const float4*)(w.b1 + l * SF + c);
            for (int i = wv; i < SR; i += 4) {
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 xa = i - dil >= 0 ? *(const float4*)(X + (i - dil) * SLD + c) : zero;
                const float4 xb = *(const float4*)(X + i * SLD + c);
                const float4 xc = i + dil < SR ? *(const float4*)(X + (i + dil) * SLD + c) : zero;
                float y[4] = {w0.x * xa.x + w1.x * xb.x + w2.x * xc.x + bb.x, w0.y * xa.y + w1.y * xb.y + w2.y * xc.y + bb.y,
                              w0.z * xa.z + w1.z * xb.z + w2.z * xc.z + bb.z, w0.w * xa.w + w1.w * xb.w + w2.w * xc.w + bb.w};
                const float mean = wave_sum((y[0] + y[1]) + (y[2] + y[3])) * (1.0f / SF);
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] -= mean;
                const float var = wave_sum((y[0] * y[0] + y[1] * y[1]) + (y[2] * y[2] + y[3] * y[3])) * (1.0f / SF);
                const float rstd = 1.0f / sqrtf(var + S_LN_EPS);
                const float4 o = make_float4(gelu_erf(y[0] * rstd * gg.x + ee.x), gelu_erf(y[1] * rstd * gg.y + ee.y),
                                             gelu_erf(y[2] * rstd * gg.z + ee.z), gelu_erf(y[3] * rstd * gg.w + ee.w));
                *(float4*)(Y + i * SLD + c) = o;
            }
        }
        __syncthreads();
        // 1x1 conv on the MFMA, bias in the accumulators
        f32x4_t acc[4][4];
        const int cb = wv * 64;  // this wave's first output channel
        seed_bias<4>(w.pb + l * SF + cb, lane, acc);
        conv1x1<4>(Y, (const float4*)(w.pw + (size_t)l * SF * SF) + (size_t)(wv * 4) * 16 * 64, 16, lane, acc);
        // LayerNorm over the row: this wave holds 64 of its 256 channels
        const int r = lane & 15, q = lane >> 4;
#pragma unroll
        for (int rf = 0; rf < 4; ++rf) {
            float s = 0.f;
#pragma unroll
            for (int f = 0; f < 4; ++f) s += (acc[f][rf][0] + acc[f][rf][1]) + (acc[f][rf][2] + acc[f][rf][3]);
            s = group4_sum(s);
            if (q == 0) red[0][wv * SR + rf * 16 + r] = s;
        }
        __syncthreads();
        float rstd[4];
#pragma unroll
        for (int rf = 0; rf < 4; ++rf) {
            const int row = rf * 16 + r;
            const float mean = ((red[0][row] + red[0][SR + row]) + (red[0][2 * SR + row] + red[0][3 * SR + row])) * (1.0f / SF);
            float s = 0.f;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[f][rf][j] -= mean;
                    s += acc[f][rf][j] * acc[f][rf][j];
                }
            }
            s = group4_sum(s);
            if (q == 0) red[1][wv * SR + row] = s;
        }
        __syncthreads();
#pragma unroll
        for (int rf = 0; rf < 4; ++rf) {
            const int row = rf * 16 + r;
            const float var = ((red[1][row] + red[1][SR + row]) + (red[1][2 * SR + row] + red[1][3 * SR + row])) * (1.0f / SF);
            rstd[rf] = 1.0f / sqrtf(var + S_LN_EPS);
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int c = cb + f * 16 + q * 4;
            const float4 gg = *(const float4*)(w.g2 + l * SF + c), ee = *(const float4*)(w.b2 + l * SF + c);
#pragma unroll
            for (int rf = 0; rf < 4; ++rf) {
                const int row = rf * 16 + r;
                if (valid[row]) {
                    float4* xp = (float4*)(X + row * SLD + c);
                    float4 xv = *xp;
                    xv.x += gelu_erf(acc[f][rf][0] * rstd[rf] * gg.x + ee.x);
                    xv.y += gelu_erf(acc[f][rf][1] * rstd[rf] * gg.y + ee.y);
                    xv.z += gelu_erf(acc[f][rf][2] * rstd[rf] * gg.z + ee.z);
                    xv.w += gelu_erf(acc[f][rf][3] * rstd[rf] * gg.w + ee.w);
                    *xp = xv;
                }
            }
        }
        __syncthreads();
    }
}

// valid[i] for the tile's rows (t = t0 + i inside [0, L) and not padded); returns whether any FINISHED row of the tile is valid
__device__ inline bool tile_valid(unsigned char* valid, const uint8_t* pad, int b, int t0, int L, int tid) {
    int fin = 0;
    if (tid < SR) {
        const int t = t0 + tid;
        const bool ok = t >= 0 && t < L && !pad[(size_t)b * L + t];
        valid[tid] = ok ? 1 : 0;
        fin = ok && tid >= SHALO && tid < SR - SHALO;
    }
    return __syncthreads_or(fin) != 0;
}

__global__ __launch_bounds__(256, 1) void sdp_encoder_kernel(SdpEncArgs p) {
    __shared__ __attribute__((aligned(16))) float X[SR * SLD];
    __shared__ __attribute__((aligned(16))) float Y[SR * SLD];
    __shared__ float red[2][4 * SR];
    __shared__ unsigned char valid[SR];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, t0 = (int)blockIdx.x * SV - SHALO;
    if (!tile_valid(valid, p.pad, b, t0, p.L, tid)) return;  // g is read at valid rows only
    // the encoder rows, converted to fp32, as the MFMA operand of `pre`
    const int h4 = p.H >> 2;
    for (int idx = tid; idx < SR * h4; idx += 256) {
        const int i = idx / h4, c4 = idx - i * h4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid[i]) v = load_row4(p.x, p.x_dtype, ((size_t)b * p.L + (t0 + i)) * p.H + c4 * 4);
        *(float4*)(Y + i * SLD + c4 * 4) = v;
    }
    __syncthreads();
    const int cb = wv * 64, r = lane & 15, q = lane >> 4;
    {
        f32x4_t acc[4][4];
        const int KQ = p.H >> 4;
        seed_bias<4>(p.pre_b + cb, lane, acc);
        conv1x1<4>(Y, (const float4*)p.pre_w + (size_t)(wv * 4) * KQ * 64, KQ, lane, acc);
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int rf = 0; rf < 4; ++rf) {
                const int row = rf * 16 + r;
                const float4 v = valid[row] ? make_float4(acc[f][rf][0], acc[f][rf][1], acc[f][rf][2], acc[f][rf][3])
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
                *(float4*)(X + row * SLD + cb + f * 16 + q * 4) = v;
            }
    }
    __syncthreads();
    dds_layers(X, Y, red, valid, p.d, tid);
    {
        f32x4_t acc[4][4];
        seed_bias<4>(p.proj_b + cb, lane, acc);
        conv1x1<4>(X, (const float4*)p.proj_w + (size_t)(wv * 4) * 16 * 64, 16, lane, acc);
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int rf = 0; rf < 4; ++rf) {
                const int row = rf * 16 + r, t = t0 + row;
                if (row >= SHALO && row < SR - SHALO && t < p.L) {
                    const float4 v = valid[row] ? make_float4(acc[f][rf][0], acc[f][rf][1], acc[f][rf][2], acc[f][rf][3])
                                                : make_float4(0.f, 0.f, 0.f, 0.f);
                    *(float4*)(p.g + ((size_t)b * p.L + t) * SF + cb + f * 16 + q * 4) = v;
                }
            }
    }
}

}  // namespace

// Inverse of the unconstrained rational-quadratic spline with linear tails, tail_bound 5, 10 bins (transforms.py:51-191 with
// inverse=True), in the reference's order of operations.  h: the row's 29 parameters, sqrt_f = sqrt(hidden channels).
// The discriminant is clamped at 0 where the reference asserts.
__device__ float rq_spline_inverse(float x, const float* h, float sqrt_f) {
    constexpr float TB = 5.0f, MINW = 1e-3f, MINH = 1e-3f, MIND = 1e-3f;
    if (!(x >= -TB && x <= TB)) return x;
    float cw[SNB + 1], ch[SNB + 1];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float u[SNB], mx = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < SNB; ++k) {
            u[k] = h[pass * SNB + k] / sqrt_f;
            mx = fmaxf(mx, u[k]);
        }
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < SNB; ++k) {
            u[k] = expf(u[k] - mx);
            sum += u[k];
        }
        float* cum = pass ? ch : cw;
        float run = 0.f;
        cum[0] = -TB;
#pragma unroll
        for (int k = 0; k < SNB; ++k) {
            run += (pass ? MINH : MINW) + (1.0f - (pass ? MINH : MINW) * SNB) * (u[k] / sum);
            cum[k + 1] = (2.0f * TB) * run + (-TB);
        }
        cum[SNB] = TB;
    }
    // bin search by >= on the cumulative heights, the last knot raised by 1e-6 (transforms.py:46-48)
    int idx = -1;
#pragma unroll
    for (int k = 0; k <= SNB; ++k) idx += x >= (k == SNB ? ch[SNB] + 1e-6f : ch[k]) ? 1 : 0;
    idx = idx < 0 ? 0 : (idx > SNB - 1 ? SNB - 1 : idx);
    float icw = 0.f, ibw = 1.f, ich = 0.f, ih = 1.f, u0 = 0.f, u1 = 0.f;
    const float edge = 0.5397424172369522f;  // log(exp(1 - 1e-3) - 1): the padded boundary derivatives
#pragma unroll
    for (int k = 0; k < SNB; ++k) {
        if (k == idx) {
            icw = cw[k];
            ibw = cw[k + 1] - cw[k];
            ich = ch[k];
            ih = ch[k + 1] - ch[k];
            u0 = k == 0 ? edge : h[2 * SNB + k - 1];
            u1 = k == SNB - 1 ? edge : h[2 * SNB + k];
        }
    }
    auto softplus = [](float v) { return v > 20.0f ? v : log1pf(expf(v)); };
    const float d0 = MIND + softplus(u0), d1 = MIND + softplus(u1);
    const float delta = ih / ibw;
    const float t = x - ich, s = d0 + d1 - 2.0f * delta;
    const float a = t * s + ih * (delta - d0);
    const float bq = ih * d0 - t * s;
    const float c = -delta * t;
    float disc = bq * bq - 4.0f * a * c;
    disc = disc > 0.f ? disc : 0.f;
    const float root = (2.0f * c) / (-bq - sqrtf(disc));
    return root * ibw + icw;
}

namespace {

__global__ __launch_bounds__(256, 1) void sdp_flow_kernel(SdpFlowArgs p) {
    __shared__ __attribute__((aligned(16))) float X[SR * SLD];
    __shared__ __attribute__((aligned(16))) float Y[SR * SLD];
    __shared__ float red[2][4 * SR];
    __shared__ float zs[2][SR];
    __shared__ unsigned char valid[SR];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, t0 = (int)blockIdx.x * SV - SHALO;
    const bool any = tile_valid(valid, p.pad, b, t0, p.L, tid);
    if (!any) {  // nothing but pad rows to finish: cat(x0, x1') * m = 0, logw = 0
        if (tid >= SHALO && tid < SR - SHALO && t0 + tid < p.L) {
            const int t = t0 + tid;
            if (p.last) p.logw[(size_t)b * p.L + t] = 0.f;
            else p.zout[((size_t)b * 2) * p.L + t] = p.zout[((size_t)b * 2 + 1) * p.L + t] = 0.f;
        }
        return;
    }
    if (tid < SR) {
        const int t = t0 + tid;
        const bool in = t >= 0 && t < p.L;
        zs[0][tid] = in ? p.zin[((size_t)b * 2 + 1) * p.L + t] : 0.f;  // the flip: x0 = channel 1
        zs[1][tid] = in ? p.zin[((size_t)b * 2) * p.L + t] : 0.f;
    }
    __syncthreads();
    // X = pre(x0) + g   (pre: Conv1d(1, 256, 1)), zero outside the utterance
    for (int idx = tid; idx < SR * (SF / 4); idx += 256) {
        const int i = idx >> 6, c = (idx & 63) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid[i]) {
            const float x0 = zs[0][i];
            const float4 w = *(const float4*)(p.pre_w + c), bb = *(const float4*)(p.pre_b + c);
            const float4 gv = *(const float4*)(p.g + ((size_t)b * p.L + (t0 + i)) * SF + c);
            v = make_float4((w.x * x0 + bb.x) + gv.x, (w.y * x0 + bb.y) + gv.y, (w.z * x0 + bb.z) + gv.z, (w.w * x0 + bb.w) + gv.w);
        }
        *(float4*)(X + i * SLD + c) = v;
    }
    __syncthreads();
    dds_layers(X, Y, red, valid, p.d, tid);
    // proj: Conv1d(256, 29, 1) as two 16-channel fragments (waves 0 and 1) -> Y[row][0 .. 31]
    if (wv < 2) {
        f32x4_t acc[1][4];
        seed_bias<1>(p.proj_b + wv * 16, lane, acc);
        conv1x1<1>(X, (const float4*)p.proj_w + (size_t)wv * 16 * 64, 16, lane, acc);
        const int r = lane & 15, q = lane >> 4;
#pragma unroll
        for (int rf = 0; rf < 4; ++rf)
            *(float4*)(Y + (rf * 16 + r) * SLD + wv * 16 + q * 4) = make_float4(acc[0][rf][0], acc[0][rf][1], acc[0][rf][2], acc[0][rf][3]);
    }
    __syncthreads();
    if (tid >= SHALO && tid < SR - SHALO && t0 + tid < p.L) {
        const int t = t0 + tid;
        float x0 = 0.f, x1 = 0.f;
        if (valid[tid]) {
            float h[SNP];
#pragma unroll
            for (int k = 0; k < SNP; ++k) h[k] = Y[tid * SLD + k];
            x0 = zs[0][tid];
            x1 = rq_spline_inverse(zs[1][tid], h, 16.0f);
        }
        if (p.last) {
            p.logw[(size_t)b * p.L + t] = valid[tid] ? (x1 - p.ea_t) * expf(-p.ea_ls) : 0.f;
        } else {
            p.zout[((size_t)b * 2) * p.L + t] = x0;
            p.zout[((size_t)b * 2 + 1) * p.L + t] = x1;
        }
    }
}

// n_flows = 1: only the ElementwiseAffine runs, on the flipped noise (channel 0 of the result = noise channel 1)
__global__ void sdp_affine_kernel(const float* noise, const uint8_t* pad, float* logw, float ea_t, float ea_ls, int B, int L) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * L) return;
    const size_t b = i / L, t = i - b * L;
    logw[i] = pad[i] ? 0.f : (noise[(b * 2 + 1) * L + t] - ea_t) * expf(-ea_ls);
}

__global__ void rq_spline_inverse_kernel(const float* x1, const float* h29, float sqrt_f, float* out, int rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    float h[SNP];
#pragma unroll
    for (int k = 0; k < SNP; ++k) h[k] = h29[(size_t)i * SNP + k];
    out[i] = rq_spline_inverse(x1[i], h, sqrt_f);
}

// W (rows x K, row-major; rows a multiple of 16, K a multiple of 16) -> [fragment = row / 16][kq = k / 16][lane][4]:
// lane (r = lane & 15, q = lane >> 4) holds W[16 fragment + r][16 kq + 4 q .. + 3]
void pack_1x1(const float* W, int rows_src, int rows, int K, float* out) {
    const int KQ = K / 16;
    for (int f = 0; f < rows / 16; ++f)
        for (int kq = 0; kq < KQ; ++kq)
            for (int lane = 0; lane < 64; ++lane) {
                const int oc = f * 16 + (lane & 15), k = kq * 16 + (lane >> 4) * 4;
                float* o = out + (((size_t)f * KQ + kq) * 64 + lane) * 4;
                for (int s = 0; s < 4; ++s) o[s] = oc < rows_src ? W[(size_t)oc * K + k + s] : 0.f;
            }
}

// The weight block indexed in floats.  The bytes of `host` are read as float: the vector's storage comes from operator new (aligned
// for any scalar) and every offset is a multiple of 16 bytes; a float reference is valid until the next grow().
struct SdpBlock : WeightBlock {
    size_t grow(size_t floats) { return WeightBlock::grow(floats * 4, 16) / 4; }
    float& operator[](size_t i) { return ((float*)host.data())[i]; }
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace
}  // namespace fs2

using namespace fs2;

struct fs2_sdp : ErrorBase {
    int H = 0, F = 0, k = 0, n = 0;
    bool ready = false;  // create succeeded
    bool finalized = false;
    WeightStore w;  // the training-only tensors with keep = false: checked, dropped, not required
    DevAllocs allocs;
    float* dev = nullptr;  // one block: every packed tensor
    // offsets (floats) into dev
    struct Dds { size_t dw_w, dw_b, g1, b1, pw, pb, g2, b2; };
    struct Flow { size_t pre_w, pre_b, proj_w, proj_b; Dds d; };
    size_t pre_w = 0, pre_b = 0, proj_w = 0, proj_b = 0;
    Dds enc{};
    std::vector<Flow> flows;  // index j - 2 <-> flows.j, j = 2 .. n
    float ea_t = 0.f, ea_ls = 0.f;
};

namespace {

void add_dds(fs2_sdp* h, const std::string& p, int F, int k, bool on) {
    for (int i = 0; i < 3; ++i) {
        const std::string s = std::to_string(i);
        h->w.expect(p + ".convs_sep." + s + ".weight", {F, 1, k}, on);
        h->w.expect(p + ".convs_sep." + s + ".bias", {F}, on);
        h->w.expect(p + ".convs_1x1." + s + ".weight", {F, F, 1}, on);
        h->w.expect(p + ".convs_1x1." + s + ".bias", {F}, on);
        for (const char* nm : {".norms_1.", ".norms_2."}) {
            h->w.expect(p + nm + s + ".gamma", {F}, on);
            h->w.expect(p + nm + s + ".beta", {F}, on);
        }
    }
}

void add_flows(fs2_sdp* h, const std::string& p, int F, int k, int n, bool inference_set) {
    h->w.expect(p + ".0.translation", {2, 1}, inference_set);
    h->w.expect(p + ".0.log_scale", {2, 1}, inference_set);
    for (int j = 1; j <= n; ++j) {
        const bool on = inference_set && j >= 2;  // flows.1 is the ConvFlow the inference loop drops (sdp.py:333-334)
        const std::string q = p + "." + std::to_string(j);
        h->w.expect(q + ".pre.weight", {F, 1, 1}, on);
        h->w.expect(q + ".pre.bias", {F}, on);
        add_dds(h, q + ".convs", F, k, on);
        h->w.expect(q + ".proj.weight", {SNP, F, 1}, on);
        h->w.expect(q + ".proj.bias", {SNP}, on);
    }
}

// one DDS's tensors into the block at `at` (floats); returns the end
size_t pack_dds(fs2_sdp* h, const std::string& p, SdpBlock& blk, fs2_sdp::Dds& o) {
    auto T = [&](const std::string& n) -> const std::vector<float>& { return h->w.at(p + n).data; };
    auto grow = [&](size_t n) { return blk.grow(n); };
    o.dw_w = grow(3 * 3 * SF); o.dw_b = grow(3 * SF); o.g1 = grow(3 * SF); o.b1 = grow(3 * SF);
    o.pw = grow((size_t)3 * SF * SF); o.pb = grow(3 * SF); o.g2 = grow(3 * SF); o.b2 = grow(3 * SF);
    for (int i = 0; i < 3; ++i) {
        const std::string s = std::to_string(i);
        const auto& w = T(".convs_sep." + s + ".weight");  // (F, 1, 3)
        for (int tp = 0; tp < 3; ++tp)
            for (int c = 0; c < SF; ++c) blk[o.dw_w + (i * 3 + tp) * SF + c] = w[c * 3 + tp];
        std::memcpy(&blk[o.dw_b + i * SF], T(".convs_sep." + s + ".bias").data(), SF * 4);
        std::memcpy(&blk[o.g1 + i * SF], T(".norms_1." + s + ".gamma").data(), SF * 4);
        std::memcpy(&blk[o.b1 + i * SF], T(".norms_1." + s + ".beta").data(), SF * 4);
        pack_1x1(T(".convs_1x1." + s + ".weight").data(), SF, SF, SF, &blk[o.pw + (size_t)i * SF * SF]);
        std::memcpy(&blk[o.pb + i * SF], T(".convs_1x1." + s + ".bias").data(), SF * 4);
        std::memcpy(&blk[o.g2 + i * SF], T(".norms_2." + s + ".gamma").data(), SF * 4);
        std::memcpy(&blk[o.b2 + i * SF], T(".norms_2." + s + ".beta").data(), SF * 4);
    }
    return blk.host.size() / 4;
}

DdsW dds_ptrs(const float* dev, const fs2_sdp::Dds& o) {
    return DdsW{dev + o.dw_w, dev + o.dw_b, dev + o.g1, dev + o.b1, dev + o.pw, dev + o.pb, dev + o.g2, dev + o.b2};
}

size_t sdp_ws_need(int B, int L) {
    // g (B, L, 256) + two z buffers (B, 2, L), each 256-byte aligned
    return align_up((size_t)B * L * SF * 4, 256) + 2 * align_up((size_t)B * 2 * L * 4, 256);
}

}  // namespace

extern "C" {

int fs2_sdp_supported(int32_t H, int32_t F, int32_t k, int32_t n_flows) {
    return F == SF && k == 3 && n_flows >= 1 && n_flows <= 8 && H >= 16 && H <= SF && H % 16 == 0;
}

int fs2_sdp_create(int32_t abi_version, int32_t H, int32_t F, int32_t k, int32_t n_flows, fs2_sdp** out) {
    if (!out) return FS2_ERR_ARG;
    *out = nullptr;
    fs2_sdp* h = new (std::nothrow) fs2_sdp();
    if (!h) return FS2_ERR_NOMEM;
    *out = h;  // returned even on failure so the caller can read fs2_sdp_last_error, then destroy
    if (abi_version != FS2_ABI_VERSION) return h->fail(FS2_ERR_ARG, "abi_version %d, this library is %d", abi_version, FS2_ABI_VERSION);
    if (F != SF) return h->fail(FS2_ERR_SHAPE, "filter size %d: the stochastic duration predictor's kernel is built for 256 channels", F);
    if (k != 3) return h->fail(FS2_ERR_SHAPE, "kernel size %d: the kernel's dilations 1 / 3 / 9 and its 13-row halo are those of k = 3", k);
    if (n_flows < 1 || n_flows > 8) return h->fail(FS2_ERR_SHAPE, "n_flows = %d: 1 .. 8 are supported", n_flows);
    if (H < 16 || H > SF || H % 16)
        return h->fail(FS2_ERR_SHAPE, "in_channels %d: `pre` runs inside the encoder launch for multiples of 16 up to 256", H);
    h->H = H; h->F = F; h->k = k; h->n = n_flows;
    h->w.expect("sdp.pre.weight", {F, H, 1}, true);
    h->w.expect("sdp.pre.bias", {F}, true);
    add_dds(h, "sdp.convs", F, k, true);
    h->w.expect("sdp.proj.weight", {F, F, 1}, true);
    h->w.expect("sdp.proj.bias", {F}, true);
    add_flows(h, "sdp.flows", F, k, n_flows, true);
    // the training-only half: the posterior encoder
    h->w.expect("sdp.post_pre.weight", {F, 1, 1}, false);
    h->w.expect("sdp.post_pre.bias", {F}, false);
    add_dds(h, "sdp.post_convs", F, k, false);
    h->w.expect("sdp.post_proj.weight", {F, F, 1}, false);
    h->w.expect("sdp.post_proj.bias", {F}, false);
    add_flows(h, "sdp.post_flows", F, k, n_flows, false);
    h->ready = true;
    return FS2_OK;
}

int fs2_sdp_destroy(fs2_sdp* h) {
    if (!h) return FS2_ERR_ARG;
    delete h;
    return FS2_OK;
}

const char* fs2_sdp_last_error(const fs2_sdp* h) { return h ? h->err : "null sdp handle"; }

int32_t fs2_sdp_tile_rows(const fs2_sdp* h) { return h && h->ready ? SV : 0; }

int fs2_sdp_load_weight(fs2_sdp* h, const char* name, const float* host_data, const int64_t* shape, int32_t ndim) {
    if (!h) return FS2_ERR_ARG;
    if (!h->ready) return h->fail(FS2_ERR_STATE, "fs2_sdp_create did not succeed");
    if (h->finalized) return h->fail(FS2_ERR_STATE, "fs2_sdp_load_weight after fs2_sdp_finalize");
    if (!name || !host_data || !shape || ndim < 1) return h->fail(FS2_ERR_ARG, "name, host_data and shape must not be null");
    return h->w.load(*h, name, host_data, shape, ndim);
}

int fs2_sdp_finalize(fs2_sdp* h) {
    if (!h) return FS2_ERR_ARG;
    if (!h->ready) return h->fail(FS2_ERR_STATE, "fs2_sdp_create did not succeed");
    if (h->finalized) return h->fail(FS2_ERR_STATE, "fs2_sdp_finalize called twice");
    if (const char* missing = h->w.first_missing()) return h->fail(FS2_ERR_WEIGHT, "missing weight '%s'", missing);
    SdpBlock blk;
    auto grow = [&](size_t n) { return blk.grow(n); };
    auto W = [&](const std::string& n) -> const std::vector<float>& { return h->w.at(n).data; };
    h->pre_w = grow((size_t)SF * h->H);
    pack_1x1(W("sdp.pre.weight").data(), SF, SF, h->H, &blk[h->pre_w]);
    h->pre_b = grow(SF);
    std::memcpy(&blk[h->pre_b], W("sdp.pre.bias").data(), SF * 4);
    pack_dds(h, "sdp.convs", blk, h->enc);
    h->proj_w = grow((size_t)SF * SF);
    pack_1x1(W("sdp.proj.weight").data(), SF, SF, SF, &blk[h->proj_w]);
    h->proj_b = grow(SF);
    std::memcpy(&blk[h->proj_b], W("sdp.proj.bias").data(), SF * 4);
    h->flows.clear();
    for (int j = 2; j <= h->n; ++j) {
        const std::string q = "sdp.flows." + std::to_string(j);
        fs2_sdp::Flow f{};
        f.pre_w = grow(SF);
        std::memcpy(&blk[f.pre_w], W(q + ".pre.weight").data(), SF * 4);
        f.pre_b = grow(SF);
        std::memcpy(&blk[f.pre_b], W(q + ".pre.bias").data(), SF * 4);
        pack_dds(h, q + ".convs", blk, f.d);
        f.proj_w = grow((size_t)32 * SF);
        pack_1x1(W(q + ".proj.weight").data(), SNP, 32, SF, &blk[f.proj_w]);
        f.proj_b = grow(32);
        std::memcpy(&blk[f.proj_b], W(q + ".proj.bias").data(), SNP * 4);
        h->flows.push_back(f);
    }
    h->ea_t = W("sdp.flows.0.translation")[0];
    h->ea_ls = W("sdp.flows.0.log_scale")[0];
    FS2_TRY(blk.upload(*h, h->allocs, (void**)&h->dev));
    h->w.drop();
    h->finalized = true;
    return FS2_OK;
}

int fs2_sdp_workspace_bytes(const fs2_sdp* h, int32_t B, int32_t L, size_t* bytes) {
    if (!h || !bytes) return FS2_ERR_ARG;
    if (B < 1 || L < 1) return FS2_ERR_ARG;
    *bytes = sdp_ws_need(B, L);
    return FS2_OK;
}

int fs2_sdp_launches(const fs2_sdp* h) { return h && h->ready ? (h->n == 1 ? 1 : h->n) : 0; }

int fs2_sdp_forward(fs2_sdp* h, int32_t x_dtype, const void* x, const uint8_t* pad_mask, const float* noise, float* logw, void* workspace,
                    size_t workspace_bytes, int32_t B, int32_t L, void* hip_stream) {
    if (!h) return FS2_ERR_ARG;
    if (!h->finalized) return h->fail(FS2_ERR_STATE, "fs2_sdp_forward before fs2_sdp_finalize");
    if (!x || !pad_mask || !noise || !logw) return h->fail(FS2_ERR_ARG, "x, pad_mask, noise and logw must not be null");
    if (x_dtype != FS2_F32 && x_dtype != FS2_BF16 && x_dtype != FS2_F16) return h->fail(FS2_ERR_ARG, "x_dtype %d: FS2_F32, FS2_BF16 or FS2_F16", x_dtype);
    if (B < 1 || L < 1) return h->fail(FS2_ERR_ARG, "B = %d, L = %d: both must be at least 1", B, L);
    if (B > 65535) return h->fail(FS2_ERR_SHAPE, "B = %d exceeds the grid's 65535 utterances", B);
    if ((uintptr_t)x & 15) return h->fail(FS2_ERR_ARG, "x must be 16-byte aligned");
    hipStream_t st = (hipStream_t)hip_stream;
    if (h->n == 1) {  // ElementwiseAffine alone: no conditioning is read
        const size_t n = (size_t)B * L;
        hipLaunchKernelGGL(sdp_affine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, noise, pad_mask, logw, h->ea_t, h->ea_ls, B, L);
        return hipGetLastError() == hipSuccess ? FS2_OK : h->fail(FS2_ERR_HIP, "launch failed");
    }
    const size_t need = sdp_ws_need(B, L);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))
        return h->fail(FS2_ERR_NOMEM, "workspace of %zu bytes, %zu needed (16-byte aligned)", workspace_bytes, need);
    float* g = (float*)workspace;
    float* z[2];
    z[0] = (float*)((char*)workspace + align_up((size_t)B * L * SF * 4, 256));
    z[1] = (float*)((char*)z[0] + align_up((size_t)B * 2 * L * 4, 256));
    const dim3 grid((unsigned)((L + SV - 1) / SV), (unsigned)B);
    SdpEncArgs e{};
    e.x = x; e.x_dtype = x_dtype; e.pad = pad_mask; e.g = g;
    e.pre_w = h->dev + h->pre_w; e.pre_b = h->dev + h->pre_b; e.d = dds_ptrs(h->dev, h->enc);
    e.proj_w = h->dev + h->proj_w; e.proj_b = h->dev + h->proj_b; e.B = B; e.L = L; e.H = h->H;
    hipLaunchKernelGGL(sdp_encoder_kernel, grid, dim3(256), 0, st, e);
    const float* zin = noise;
    for (int j = h->n; j >= 2; --j) {  // CF_n .. CF_2
        const fs2_sdp::Flow& f = h->flows[j - 2];
        SdpFlowArgs a{};
        a.zin = zin; a.zout = z[(h->n - j) & 1]; a.logw = logw; a.g = g; a.pad = pad_mask;
        a.pre_w = h->dev + f.pre_w; a.pre_b = h->dev + f.pre_b; a.d = dds_ptrs(h->dev, f.d);
        a.proj_w = h->dev + f.proj_w; a.proj_b = h->dev + f.proj_b;
        a.ea_t = h->ea_t; a.ea_ls = h->ea_ls; a.last = j == 2; a.B = B; a.L = L;
        hipLaunchKernelGGL(sdp_flow_kernel, grid, dim3(256), 0, st, a);
        zin = a.zout;
    }
    return hipGetLastError() == hipSuccess ? FS2_OK : h->fail(FS2_ERR_HIP, "launch failed: %s", hipGetErrorString(hipGetLastError()));
}

int fs2_op_rq_spline_inverse(const float* x1, const float* h29, int32_t F, float* out, int32_t rows, void* hip_stream) {
    if (!x1 || !h29 || !out || F < 1 || rows < 0) return FS2_ERR_ARG;
    if (rows == 0) return FS2_OK;
    hipLaunchKernelGGL(rq_spline_inverse_kernel, dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)hip_stream, x1, h29,
                       sqrtf((float)F), out, rows);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

int fs2_op_durations_stochastic(const float* logw, const uint8_t* src_mask, const int32_t* forced, int32_t* dur, int32_t* cum,
                                int32_t* totals, int32_t* guard, int32_t B, int32_t L, void* hip_stream) {
    if (!logw || !src_mask || !dur || !cum || !totals || !guard || B < 0 || L < 1) return FS2_ERR_ARG;
    DurationArgs a{logw, src_mask, forced, dur, cum, totals, guard, B, L, 1};  // the deterministic rule's kernel, its rounding swapped
    return launch_durations(a, (hipStream_t)hip_stream);
}

}  // extern "C"
