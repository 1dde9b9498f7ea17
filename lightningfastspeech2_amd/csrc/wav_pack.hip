// Waveform finishing behind the HiFi-GAN generator: the padded fp32 (B, T*hop) wav -> one packed buffer of int16 samples (or the
// float32 the reference's int16_samples_to_float32 makes of them) holding every utterance's own samples back to back, plus the
// offsets table, in one launch.  What SpeechGenerator.generate_samples / Synthesiser.__call__ did on the host with numpy
// (third_party/hifigan/__init__.py:39-43, synthesis/generator.py:24-33,163-170) over the pads as well.
//
// Memory-bound: 8 samples per lane = two 16 B loads and one (int16) or two (float32) 16 B stores.  The frame counts are read on the
// device only; every workgroup sums the clamped counts in front of its utterance itself (B is a batch size: tens of 4 B loads), so
// there is no scan launch and no workgroup waits for another.
#include "fs2_common.h"
#include "fs2_kernels.h"

namespace fs2 {

static constexpr int WP_THREADS = 256;
static constexpr int WP_CHUNK = WP_THREADS * 8;  // samples per workgroup and round

// (x * 32768.0).astype("int16") of numpy on the hosts the reference runs on: the product is exact (a power of two), the conversion
// truncates toward zero to int32 and keeps the low 16 bits - tanh's +1.0 becomes -32768.  |x| <= 1, so the int32 never saturates.
__device__ __forceinline__ int16_t wp_quantise(float x) { return (int16_t)(int32_t)(x * 32768.0f); }

template <int KIND> struct WpOut;
template <> struct WpOut<FS2_WAV_I16> {
    using T = int16_t;
    static __device__ __forceinline__ T make(float x) { return wp_quantise(x); }
};
template <> struct WpOut<FS2_WAV_F32> {
    using T = float;
    // int16_samples_to_float32: y.astype(float32) / 32767 - IEEE division (no fast-math in this build: correctly rounded)
    static __device__ __forceinline__ T make(float x) { return (float)wp_quantise(x) / 32767.0f; }
};

__device__ __forceinline__ int wp_clamp(int n, int T) { return n < 0 ? 0 : (n > T ? T : n); }

template <int KIND>
__global__ __launch_bounds__(WP_THREADS) void wav_pack_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lengths,
                                                              typename WpOut<KIND>::T* __restrict__ out,
                                                              long long* __restrict__ offsets, int B, int T, int hop) {
    using O = typename WpOut<KIND>::T;
    const int b = blockIdx.x, tid = threadIdx.x;
    long long frames_before;
    int len;
    if (lengths) {
        __shared__ long long red[WP_THREADS / 64];
        long long part = 0;
        for (int i = tid; i < b; i += WP_THREADS) part += wp_clamp(lengths[i], T);
        for (int o = 32; o; o >>= 1) part += __shfl_down(part, o);
        if ((tid & 63) == 0) red[tid >> 6] = part;
        __syncthreads();
        frames_before = red[0] + red[1] + red[2] + red[3];
        len = wp_clamp(lengths[b], T);
    } else {
        frames_before = (long long)b * T;
        len = T;
    }
    const long long off = frames_before * hop;
    const int n = len * hop;  // this utterance's samples; T * hop < 2^31 (launcher)
    if (blockIdx.y == 0 && tid == 0) {
        offsets[b] = off;
        if (b == B - 1) offsets[B] = off + n;
    }
    int base = blockIdx.y * WP_CHUNK;
    if (base >= n) return;  // uniform: workgroups past the utterance's end touch nothing
    const float* __restrict__ src = wav + (size_t)b * T * hop;
    O* __restrict__ dst = out + off;
    // offsets are multiples of hop: 16 B accesses where this utterance's two rows allow them (uniform per workgroup)
    const bool wide = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
    for (; base < n; base += gridDim.y * WP_CHUNK) {
        if (wide && base + WP_CHUNK <= n) {
            const int i = base + tid * 8;
            const float4 a = *reinterpret_cast<const float4*>(src + i);
            const float4 c = *reinterpret_cast<const float4*>(src + i + 4);
            const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
            if constexpr (KIND == FS2_WAV_I16) {
                uint32_t w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    w[j] = (uint32_t)(uint16_t)wp_quantise(v[2 * j]) | ((uint32_t)(uint16_t)wp_quantise(v[2 * j + 1]) << 16);
                *reinterpret_cast<uint4*>(dst + i) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                *reinterpret_cast<float4*>(dst + i) = make_float4(WpOut<KIND>::make(v[0]), WpOut<KIND>::make(v[1]),
                                                                  WpOut<KIND>::make(v[2]), WpOut<KIND>::make(v[3]));
                *reinterpret_cast<float4*>(dst + i + 4) = make_float4(WpOut<KIND>::make(v[4]), WpOut<KIND>::make(v[5]),
                                                                      WpOut<KIND>::make(v[6]), WpOut<KIND>::make(v[7]));
            }
        } else {  // a misaligned utterance (hop no multiple of 8 / 4) or the last, partial chunk: one sample per lane, coalesced
            const int end = base + WP_CHUNK < n ? base + WP_CHUNK : n;
            for (int i = base + tid; i < end; i += WP_THREADS) dst[i] = WpOut<KIND>::make(src[i]);
        }
    }
}

int launch_wav_pack(const WavPackArgs& a, hipStream_t st) {
    if (!a.wav || !a.out || !a.offsets || a.B <= 0 || a.T <= 0 || a.hop <= 0) return FS2_ERR_ARG;
    if (a.kind != FS2_WAV_I16 && a.kind != FS2_WAV_F32) return FS2_ERR_ARG;
    const long long row = (long long)a.T * a.hop;
    if (row > 0x7fffffffLL - 2048LL * WP_CHUNK) return FS2_ERR_SHAPE;  // a row is indexed with int, one stride of the grid beyond its end included
    if (a.capacity < 0 || a.capacity / row < a.B) return FS2_ERR_ARG;  // capacity < B * T * hop: the packed total is known on the device only
    long long chunks = (row + WP_CHUNK - 1) / WP_CHUNK;
    const long long cap = (2048 + a.B - 1) / a.B;  // ~8 workgroups per CU over the batch, the rest by stride
    if (chunks > cap) chunks = cap;
    const dim3 g((unsigned)a.B, (unsigned)chunks), blk(WP_THREADS);
    if (a.kind == FS2_WAV_I16)
        hipLaunchKernelGGL((wav_pack_kernel<FS2_WAV_I16>), g, blk, 0, st, a.wav, a.lengths, (int16_t*)a.out, (long long*)a.offsets, a.B, a.T, a.hop);
    else
        hipLaunchKernelGGL((wav_pack_kernel<FS2_WAV_F32>), g, blk, 0, st, a.wav, a.lengths, (float*)a.out, (long long*)a.offsets, a.B, a.T, a.hop);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

}  // namespace fs2
