// MFMA GEMM / implicit-GEMM Conv1d for gfx950.
//
//   C[m, n] = epilogue( sum_{tap, c} X[m + tap - pad, c] * W[n, tap*Cin + c] + bias[n] )
//
// replaces, on the FastSpeech2 forward path, every nn.Linear / pointwise Conv1d and the dense
// "same"-padded Conv1d of the reference (model.py:94-106 conv FFN, model.py:528-536 predictor
// conv, nn.MultiheadAttention in/out projections, fastspeech2.py:385-388 mel linear).
// Activations are (B*S, C) row-major; the zero "same" padding is applied per utterance (rows of
// different utterances are adjacent, the halo must not cross them) and is NOT masked by the
// padding mask, exactly as the reference's unmasked convs behave.
//
// Tiling: 128 (x rows) x 128 (W rows) per 256-thread workgroup, 4 waves as 2x2, each wave a
// 64x64 patch = 4x4 MFMA 16x16 fragments.  K advances in 128-byte chunks per row (64 bf16 /
// 32 fp32), double-buffered in LDS with an XOR-16B swizzle so every ds_read_b128 lane group is
// conflict free; the next chunk's global loads are issued before the current chunk's MFMAs and
// written to the other LDS buffer afterwards (one barrier per chunk).  MFMA operands are swapped
// (W is the row operand) so each lane ends up with 4 consecutive n of one output row: the
// epilogue is one 8/16-byte store per fragment.
#include <string.h>

#include "fs2_common.h"
#include "fs2_kernels.h"

namespace fs2 {

static constexpr int BM = 128, BN = 128, ROWB = 128;  // ROWB: bytes of K per LDS row
static constexpr int TILE_BYTES = BM * ROWB;           // 16 KiB per operand per buffer

__device__ inline int swz(int row, int slot) { return row * ROWB + ((slot ^ (row & 7)) << 4); }

template <typename T, typename OutT, bool ZR = false>
__global__ __launch_bounds__(256) void gemm_conv_kernel(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sX = smem;                   // [2][TILE_BYTES]
    unsigned char* sW = smem + 2 * TILE_BYTES;  // [2][TILE_BYTES]
    constexpr int E16 = Num<T>::kPer16B;        // elements per 16 bytes
    constexpr int KE = ROWB / (int)sizeof(T);   // k elements per chunk

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_n = (p.N + BN - 1) / BN;
    const int bm = blockIdx.x / tiles_n, bn = blockIdx.x % tiles_n;
    const int m0 = bm * BM, n0 = bn * BN;

    const T* __restrict__ X = (const T*)p.X;
    const T* __restrict__ W = (const T*)p.W;

    // staging assignment: 4 (row, slot) pairs per thread for each operand
    const int srow = tid >> 3, sslot = tid & 7;
    int xt[4];       // position of the row inside its utterance (conv zero padding)
    bool xin[4];     // row < M
    size_t xoff[4];  // element offset of (row, slot) at tap shift 0, channel 0
    size_t woff[4];
    bool win[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + srow + 32 * i;
        xin[i] = m < p.M;
        xt[i] = (p.taps > 1) ? (m % p.S) : 0;
        xoff[i] = (size_t)m * p.ldx + sslot * E16;
        const int n = n0 + srow + 32 * i;
        win[i] = n < p.N;
        woff[i] = (size_t)n * p.K + sslot * E16;
    }

    const int nk = p.K / KE;
    uint4 rx[4], rw[4];

    auto load_chunk = [&](int kc) {
        const int k0 = kc * KE;
        int tap = 0, c0 = k0;
        if (p.taps > 1) { tap = k0 / p.Cin; c0 = k0 - tap * p.Cin; }
        const int shift = tap - p.pad;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool ok = xin[i];
            if (p.taps > 1) { const int t = xt[i] + shift; ok = ok && t >= 0 && t < p.S; }
            rx[i] = ok ? *(const uint4*)(X + xoff[i] + (ptrdiff_t)shift * p.ldx + c0) : make_uint4(0, 0, 0, 0);
            rw[i] = win[i] ? *(const uint4*)(W + woff[i] + k0) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = srow + 32 * i;
            *(uint4*)(sX + buf * TILE_BYTES + swz(row, sslot)) = rx[i];
            *(uint4*)(sW + buf * TILE_BYTES + swz(row, sslot)) = rw[i];
        }
    };

    f32x4_t acc[4][4];  // [ni][mi]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;

    load_chunk(0);
    store_chunk(0);
    __syncthreads();

    for (int kc = 0; kc < nk; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < nk) load_chunk(kc + 1);
        const unsigned char* bx = sX + buf * TILE_BYTES;
        const unsigned char* bw = sW + buf * TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 fw[4], fx[4];
            const int slot = ks * 4 + fg;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                fw[i] = *(const uint4*)(bw + swz(wn * 64 + i * 16 + fr, slot));
                fx[i] = *(const uint4*)(bx + swz(wm * 64 + i * 16 + fr, slot));
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) Mma16<T>::step(fw[ni], fx[mi], acc[ni][mi]);
        }
        if (kc + 1 < nk) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // epilogue: lane holds, per fragment, out[m][n .. n+3]
    OutT* __restrict__ C = (OutT*)p.C;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + wn * 64 + ni * 16 + fg * 4;
        if (n >= p.N) continue;
        float bv[4] = {0.f, 0.f, 0.f, 0.f}, wgv[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) {
#pragma unroll
            for (int r = 0; r < 4; ++r) if (n + r < p.N) bv[r] = p.bias[n + r];
        }
        if (p.rs_stats) {
#pragma unroll
            for (int r = 0; r < 4; ++r) if (n + r < p.N) wgv[r] = p.rs_wg[n + r];
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int m = m0 + wm * 64 + mi * 16 + fr;
            if (m >= p.M) continue;
            const bool zr = ZR && p.zero_rows[m];
            float2 rq = make_float2(1.f, 0.f);
            if (p.rs_stats) rq = ((const float2*)p.rs_stats)[m];  // the row-scaled product (GemmArgs::rs_stats): narrow heads (N < 192) take it here
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = p.rs_stats ? __builtin_fmaf(acc[ni][mi][r], rq.x, __builtin_fmaf(-rq.y, wgv[r], bv[r])) : acc[ni][mi][r] + bv[r];
                if (p.relu) v[r] = fmaxf(v[r], 0.f);
                if (ZR) v[r] = zr ? 0.f : v[r];
            }
            OutT* dst = C + (size_t)m * p.ldc + n;
            if (n + 3 < p.N) {
                if constexpr (sizeof(OutT) == 4) {
                    *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    *(uint2*)dst = make_uint2(pack2<OutT>(v[0], v[1]), pack2<OutT>(v[2], v[3]));
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) if (n + r < p.N) dst[r] = Num<OutT>::from_f32(v[r]);
            }
        }
    }
}

// =================================================================================================
// Slab kernel: (MI*32) rows of ONE utterance x 256 output channels per 512-thread workgroup
// (8 waves as 2 x 4, wave patch (MI*16) x 64).  For a k-tap conv the x operand of all taps is the
// same (rows + k - 1) x 64-channel slab: it is DMA'd into LDS ONCE per channel block and the taps
// walk it with a row offset, so per output tile the activation traffic through L2 -> LDS drops
// k-fold; only the (256 x 64) weight tile changes every step.  Loop order: channel block (outer),
// tap (inner) - a pure re-association of the K sum.  Zero "same" padding = slab rows outside
// [0, S) of the utterance read the zero page.  Two slab buffers + two weight buffers, each its own
// LDS object; every step: explicit vmcnt(0) + __syncthreads, issue the
// next step's DMAs, multiply the current one.
// (LEAD = 1 / 2, 16-bit operands: a third weight buffer, the weight tile requested TWO steps ahead behind a counted vmcnt - the
// lead-2 K loop below; same MFMA sequence, same bits; taken for the launch classes slab_lead_form lists.)
// =================================================================================================
// Slab-kernel weight tile: MFMA row i (= lane group fg*4 + r in the accumulator) of fragment ni is
// mapped to output channel  (ni>>1)*32 + (i>>2)*8 + (ni&1)*4 + (i&3)  of the wave's 64, so that a lane
// ends up with 8 consecutive channels per fragment pair (wide, line-friendly stores).  wswz is the
// 16-byte XOR swizzle that keeps those fragment reads bank-conflict free.
__device__ inline int wcol(int ni, int fgq) { return (ni >> 1) * 32 + fgq * 8 + (ni & 1) * 4; }
__device__ inline int wswz(int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); }

template <int MI> struct SlabCfg {
    static constexpr int BM = MI * 32;
    static constexpr int SLAB_GROUPS = (BM + 30 + 7) / 8;          // 8-row (1 KiB) DMA groups, k <= 31
    static constexpr int SI = (SLAB_GROUPS + 7) / 8;                // slab DMA instructions per wave
    static constexpr int SLAB_BYTES = SI * 8 * 1024;
};
static constexpr int S_BN = 256;
template <bool B> struct BoolC { static constexpr bool value = B; };

// (r02 built an in-place WIDE fused LayerNorm epilogue for N > 256 - one workgroup per row tile walks the column tiles, stores pre-norm
// rows, re-reads and normalises its own rows - which only tied two launches at M = 49152, K = 768 (118 vs 120 us) and lost elsewhere
// (K = 3072: 357 vs 294 us; M = 8192 / 12288: 1.5-2.2x slower); r04 an operand RING of 3 / 4 stages for pointwise launches on short
// tiles, measured neutral (these launches are bound by what a CU ingests per second, not by a step's round trip).  Both removed in r05;
// profiles/HISTORY.md §4 keeps the measurements.)
// SPLIT (T = float only): fp32 operands, bf16 x 3 arithmetic.  Each fp32 value is split in registers into a bf16 head
// and a bf16 tail (x = hi + lo up to 2^-17 |x|) and a product becomes three bf16 MFMAs, hi*hi + hi*lo + lo*hi, accumulated
// in fp32 (the dropped lo*lo term is 2^-16 of the product): ~1e-5 relative, ~400x closer to fp32 than bf16 storage, at
// 3 x 16-cycle MFMAs per 32 k-values instead of the 8 x 32-cycle fp32 MFMAs - the arithmetic of the "front" (encoder +
// variance adaptor) in the mixed precision mode, where a discrete decision hangs on every output.
// DEFER (LN = false only): the deferred-LayerNorm epilogue (residual preload + pre-norm store + row statistics); its own
// instantiation so that the plain GEMM launches do not carry its registers (the in-projection measured +9 % with both in one).
#ifdef FS2_SLAB_PROBE  // tools/probes/slab_phase_stamps.py: s_memtime of waves 0 and 7 of workgroups 0 and 128 at the phase boundaries
__device__ unsigned long long g_slab_stamps[4][8];
#define SLAB_STAMP(i)                                                                                                   \
    do {                                                                                                                \
        if ((blockIdx.x == 0 || blockIdx.x == 128) && (threadIdx.x == 0 || threadIdx.x == 448))                          \
            g_slab_stamps[(blockIdx.x ? 2 : 0) + (threadIdx.x ? 1 : 0)][i] = __builtin_amdgcn_s_memtime();               \
    } while (0)
#else
#define SLAB_STAMP(i) do { } while (0)
#endif

template <typename T, typename OutT, int MI, bool LN, bool SPLIT = false, bool DEFER = false, bool XPRE = false, int LEAD = 0>
__global__ __launch_bounds__(512) void gemm_conv_slab_kernel(GemmArgs p) {
    static_assert(!XPRE || SPLIT, "XPRE: the split arithmetic's conv form (activation slab split in place when it lands)");
    static_assert(LEAD == 0 || (!SPLIT && sizeof(T) == 2), "the lead-2 K loop is the 16-bit kernels'");
    static_assert(LEAD >= 0 && LEAD <= 2 && (LEAD != 2 || MI <= 4), "lead-2: pointwise (1) up to 192 rows, conv (2) up to 128 - what three weight stages leave of the LDS");
    static_assert(!SPLIT || sizeof(T) == 4, "the split arithmetic takes fp32 operands");
    static_assert(!(DEFER && LN), "deferred LayerNorm is what a launch WITHOUT the fused epilogue leaves behind");
#if defined(__HIP_DEVICE_COMPILE__)  // the buffer-resource builtins only exist in the device pass
    using Cfg = SlabCfg<MI>;
    constexpr int BMs = Cfg::BM;
    constexpr int SI = Cfg::SI;
    // (the pointwise lead-2 form sizes a slab stage for what taps = 1 reads, BM rows: the k <= 31 halo is what does not fit beside a third weight stage at 192 rows)
    constexpr int SLAB_B = LEAD == 1 ? BMs * ROWB : Cfg::SLAB_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char slab0[SLAB_B];
    __shared__ __attribute__((aligned(16))) unsigned char slab1[SLAB_B];
    __shared__ __attribute__((aligned(16))) unsigned char wt0[S_BN * ROWB];  // 32 KiB weight tile per stage
    __shared__ __attribute__((aligned(16))) unsigned char wt1[S_BN * ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char wt2[LEAD ? S_BN * ROWB : 16];  // lead-2 forms: the third stage (never named otherwise: not allocated)
    // The column tile's per-channel epilogue constants - bias, and for the fused LayerNorm epilogue gamma, beta, the predictor head's
    // weights - fetched at the TOP of the kernel (one value per thread, their round trip under the first operand DMAs') and parked
    // in LDS.  (Until r05 the epilogues fetched them behind the K loop: sixteen bias loads per lane, then gamma / beta - the
    // "barrier 3.1 k" and part of the "row statistics 4.5 k" of a 48 k-tick out-projection + LayerNorm launch,
    // tools/probes/slab_phase_stamps.py, with nothing to hide the two round trips under.)
    __shared__ __attribute__((aligned(16))) float sprm[(LN ? 4 : 1) * S_BN];
    constexpr int KE = ROWB / (int)sizeof(T);
    SLAB_STAMP(0);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = p.S, nutt = p.M / S;
    const int tiles_n = (p.N + S_BN - 1) / S_BN;
    const int tiles_m = (S + BMs - 1) / BMs;
    int bid = blockIdx.x;
    if (p.xcd_remap == 2) {
        // Column PAIRS per XCD (the launcher checks the divisibilities): XCD x owns the column tiles {2 cg, 2 cg + 1}, cg = x % (tiles_n / 2),
        // and every (8 / (tiles_n / 2))-th row tile.  r05 counters on the decoder conv1 (4 column tiles, W = 4.7 MB, 4 MB of L2 per XCD): with
        // whole row tiles per XCD (mode 1) the slab is fetched once but every XCD streams the whole weight panel through its L2 once per
        // ROUND (25 + 113 MB fetched); with one column tile per XCD (what the plain order happens to give at 4 column tiles) the
        // weights stay (9 MB) and the slab is fetched four times (100 MB).  Pairs: 2.4 MB of weights per XCD stay resident, the slab
        // is fetched twice.
        const int ncg = tiles_n >> 1, xg = 8 / ncg, xcd = bid & 7, k = bid >> 3;
        bid = ((k >> 1) * xg + xcd / ncg) * tiles_n + (xcd % ncg) * 2 + (k & 1);
    } else if (p.xcd_remap) {
        // Workgroup i is dispatched to XCD i % 8.  Hand every XCD a CONTIGUOUS range of tiles, so that
        // the column tiles of one row tile (which read the same activation slab) run on the same XCD at
        // the same time and share it in that XCD's L2 instead of fetching it once per XCD.
        const int nt = gridDim.x, per = nt >> 3, rem = nt & 7, xcd = bid & 7;
        bid = xcd * per + (xcd < rem ? xcd : rem) + (bid >> 3);
    }
    // Split-K launches (p.ksplit > 1; plain epilogue, OutT = float): split ks owns a contiguous range of the Cin / KE channel blocks (all
    // taps) and stores its partial sums into plane ks of C, (ksplit, M, ldc); split_k_reduce_kernel adds the planes up.  ks is the
    // SLOWEST tile index, so an XCD's contiguous tile range reads one or two weight slices, not the whole panel.
    int ks = 0;
    if constexpr (!LN && !DEFER) {
        if (p.ksplit > 1) {
            const int per_split = gridDim.x / p.ksplit;
            ks = bid / per_split;
            bid -= ks * per_split;
        }
    }
    const int bn = bid % tiles_n;
    bid /= tiles_n;
    const int tm = bid % tiles_m, ub = bid / tiles_m;
    if (ub >= nutt) return;
    const int t0 = tm * BMs;
    int n0 = bn * S_BN;
    const int ntap = p.taps, ncc = p.Cin / KE / (p.ksplit > 1 ? p.ksplit : 1), cc0 = ks * ncc;
    const T* __restrict__ Xu = (const T*)p.X + (size_t)ub * S * p.ldx + cc0 * KE;  // this utterance's rows (this split's channels)
    // Operands are fetched with buffer loads straight into LDS: a descriptor per operand in SGPRs,
    // one 32-bit byte offset per lane per DMA, the channel/tap advance in the scalar offset.  Lanes
    // whose row must read as zero (outside the utterance, M/N tails) carry an out-of-range offset:
    // the hardware bounds check returns zeros for them.
    constexpr unsigned OOB = 0xFFFFF000u;
    const unsigned xbytes = (unsigned)(((size_t)(S - 1) * p.ldx + p.Cin - cc0 * KE) * sizeof(T));
    const unsigned wbytes = (unsigned)((size_t)p.N * p.K * sizeof(T));
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)Xu, 0, xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, wbytes, 0x00020000);
    // DMA duty is NOT shared evenly: only waves 0 .. DW-1 issue the operand DMAs (2x the pieces each).  The issue
    // arbiter serves the oldest wave of a SIMD first, so waves 0-3 finish a step's MFMAs ~1000 cycles before
    // waves 4-7 and idle at the barrier, while an LDS-DMA instruction costs its wave 100-150 issue cycles next to
    // MFMAs (tools/probes/slab_stamps.py, step_shape_mfma.hip): the ~500 cycles of DMA issue per step belong on
    // the waves that have the slack, off the critical ones.
    constexpr int DW = 4, DSI = LEAD == 1 ? MI : SI * 8 / DW, DWI = 32 / DW;
    const bool dma_wave = wave < DW;
    unsigned svoff[DSI];
#pragma unroll
    for (int i = 0; i < DSI; ++i) {
        const int P = (i * DW + (wave & (DW - 1))) * 64 + lane, row = P >> 3, ps = P & 7;
        const int t = t0 - p.pad + row;
        const bool ok = (t >= 0) & (t < S) & (row < BMs + ntap - 1);
        svoff[i] = ok ? (unsigned)t * (unsigned)(p.ldx * (int)sizeof(T)) + (unsigned)((ps ^ (row & 7)) << 4) : OOB;  // < 4 GiB (xbytes)
    }
    unsigned wvoff[DWI];
    auto set_wvoff = [&]() {
#pragma unroll
        for (int i = 0; i < DWI; ++i) {
            const int P = (i * DW + (wave & (DW - 1))) * 64 + lane, row = P >> 3, ps = P & 7;
            const int n = n0 + row;
            wvoff[i] = n < p.N ? (unsigned)n * (unsigned)(p.K * (int)sizeof(T)) + (unsigned)((ps ^ wswz(row)) << 4) : OOB;  // < 4 GiB (wbytes)
        }
    };
    set_wvoff();
    auto issue_slab = [&](unsigned char* dst, int cc) {
        if (!dma_wave) return;
#pragma unroll
        for (int i = 0; i < DSI; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(dst + (i * DW + wave) * 1024),
                                                     16, svoff[i], cc * ROWB, 0, 0);
    };
    auto issue_w = [&](unsigned char* dst, int cc, int tap) {
        if (!dma_wave) return;
        const int koff = (tap * p.Cin + (cc0 + cc) * KE) * (int)sizeof(T);
#pragma unroll
        for (int i = 0; i < DWI; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(dst + (i * DW + wave) * 1024),
                                                     16, wvoff[i], koff, 0, 0);
    };
    // The lead-2 K loop's requests: never under a branch (the caller is the DMA waves' copy of the loop) and never skipped - a
    // request past the last step goes out with every lane out of range (no memory traffic, zeros into a stage nobody reads
    // again), so that every step issues the SAME number of DMA instructions and its counted wait is a compile-time number.
    auto issue_slab_l = [&](unsigned char* dst, int cc, bool live) {
#pragma unroll
        for (int i = 0; i < DSI; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(dst + (i * DW + wave) * 1024),
                                                     16, live ? svoff[i] : OOB, live ? cc * ROWB : 0, 0, 0);
    };
    auto issue_w_l = [&](unsigned char* dst, int cc, int tap, bool live) {
        const int koff = live ? (tap * p.Cin + (cc0 + cc) * KE) * (int)sizeof(T) : 0;
#pragma unroll
        for (int i = 0; i < DWI; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(dst + (i * DW + wave) * 1024),
                                                     16, live ? wvoff[i] : OOB, koff, 0, 0);
    };

    f32x4_t acc[4][MI];  // [ni][mi]
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fg = lane >> 4;
    const int xrow0 = wm * (MI * 16) + fr;  // slab row of fragment 0 at tap 0
    // Residual without an activation in front of it: start the accumulators AT the residual, fetched
    // with 16-byte loads that land underneath the first operand DMAs instead of sitting, exposed,
    // between the K loop and the row statistics.
    // (the deferred-LayerNorm epilogue does the same with ITS residual, normalised first if that is a pre-norm tensor)
    // (with the epilogue's dropout the residual must stay OUT of the accumulators: the mask applies to the product alone)
    const bool res_in_acc = !p.relu && !(LN && p.drop_p > 0.f) && (LN ? p.res != nullptr : (DEFER && p.epi_res != nullptr));
    int woff[4][2];                          // weight fragment byte offsets (tap independent)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int wrow = wn * 64 + wcol(i, fr >> 2) + (fr & 3);  // MFMA row fr of fragment i <-> channel
            woff[i][ks] = wrow * ROWB + (((ks * 4 + fg) ^ wswz(wrow)) << 4);
        }

    // SPLIT: the weights ARRIVE as heads + tails (slot fg of a row's 128-byte chunk = the bf16 heads of lane group fg's eight k-values,
    // slot 4 + fg their tails: presplit_pack_kernel, once per weight tensor); the activations are fp32 and are split either in
    // registers as a fragment is read (pointwise launches) or - XPRE, conv launches - in place when the slab lands (split_rows
    // below: once per element instead of once per column wave and tap).
    auto compute = [&](const unsigned char* sl, const unsigned char* wt, int tap) {
        if constexpr (SPLIT) {
            // both 16-byte chunks of the step = 8 k-values per lane = the k-group one bf16 16x16x32 MFMA takes from it
            uint4 wh[4], wl[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { wh[i] = *(const uint4*)(wt + woff[i][0]); wl[i] = *(const uint4*)(wt + woff[i][1]); }
            if constexpr (XPRE) {
                // no VALU between the fragment reads and the MFMAs: left alone hipcc hoists all 2 MI reads to the top (64 more live
                // registers next to 128 accumulators) - one row block ahead, pinned
                uint4 xh[2], xl[2];
                xh[0] = *(const uint4*)(sl + swz(xrow0 + tap, fg));
                xl[0] = *(const uint4*)(sl + swz(xrow0 + tap, 4 + fg));
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    if (mi + 1 < MI) {
                        xh[(mi + 1) & 1] = *(const uint4*)(sl + swz(xrow0 + (mi + 1) * 16 + tap, fg));
                        xl[(mi + 1) & 1] = *(const uint4*)(sl + swz(xrow0 + (mi + 1) * 16 + tap, 4 + fg));
                    }
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        Mma16<bf16>::step(wl[ni], xh[mi & 1], acc[ni][mi]);  // small terms first
                        Mma16<bf16>::step(wh[ni], xl[mi & 1], acc[ni][mi]);
                        Mma16<bf16>::step(wh[ni], xh[mi & 1], acc[ni][mi]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    uint4 xh, xl;
                    split_bf16x3(*(const uint4*)(sl + swz(xrow0 + mi * 16 + tap, fg)), *(const uint4*)(sl + swz(xrow0 + mi * 16 + tap, 4 + fg)), xh, xl);
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        Mma16<bf16>::step(wl[ni], xh, acc[ni][mi]);  // small terms first
                        Mma16<bf16>::step(wh[ni], xl, acc[ni][mi]);
                        Mma16<bf16>::step(wh[ni], xh, acc[ni][mi]);
                    }
                }
            }
        } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 fw[4], fx[MI];
#pragma unroll
            for (int i = 0; i < 4; ++i) fw[i] = *(const uint4*)(wt + woff[i][ks]);
#pragma unroll
            for (int i = 0; i < MI; ++i) fx[i] = *(const uint4*)(sl + swz(xrow0 + i * 16 + tap, ks * 4 + fg));
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) Mma16<T>::step(fw[ni], fx[mi], acc[ni][mi]);
        }
        }
    };

    // SPLIT, conv launches: head / tail split of a landed fp32 activation slab, in place, ONCE per element: the pair of 16-byte slots
    // (s, 4 + s) of a row - the eight k-values lane group s feeds one bf16 MFMA - becomes (heads, tails).  Until r04 every wave split
    // every fragment it read: a weight value twice (2 row waves), an activation four times (4 column waves) and again at every conv
    // tap - (4 + MI) x ~24 VALU instructions per wave and step next to 12 MI MFMAs; the decoder conv1 ran 3.7x its bf16 launch.
    // Same arithmetic per element (split_bf16x3): bit-identical results.  (Splitting the weight tile in LDS as well - one more
    // barrier per step - measured slower on every pointwise launch: the weights are split once at load time instead.)
    auto split_rows = [&](unsigned char* buf, int nrows) {
        for (int i = tid; i < nrows * 4; i += 512) {
            const int row = i >> 2, sl4 = i & 3;
            const int x = row & 7;
            unsigned char* a0 = buf + row * ROWB + ((sl4 ^ x) << 4);
            unsigned char* a1 = buf + row * ROWB + (((4 + sl4) ^ x) << 4);
            uint4 h, l;
            split_bf16x3(*(const uint4*)a0, *(const uint4*)a1, h, l);
            *(uint4*)a0 = h;
            *(uint4*)a1 = l;
        }
    };
    // Step (cc, tap) uses slab[cc & 1] and wt[(cc*ntap + tap) & 1]; ntap is odd (the launcher checks),
    // so the weight parity is (cc + tap) & 1.  The steps are laid out as straight-line code with
    // STATIC buffer names (no pointer selects: hipcc then knows which LDS object each ds_read
    // touches and does not wait for the DMAs it has just issued into the other buffers).
#define FS2_SLAB_STEP(slab_cur, slab_nxt, w_cur, w_nxt, ccv, tapv)                          \
    {                                                                                       \
        dma_drain();     /* this wave's DMAs have landed ...                          */     \
        __syncthreads(); /* ... and so have everyone else's; the other buffers are free */  \
        int ntp = (tapv) + 1, ncb = (ccv);                                                  \
        if (ntp == ntap) { ntp = 0; ++ncb; }                                                \
        if (ncb < ncc) issue_w(w_nxt, ncb, ntp);                                            \
        if ((tapv) == 0 && (ccv) + 1 < ncc) issue_slab(slab_nxt, (ccv) + 1);                \
        if constexpr (XPRE) {                                                               \
            if ((tapv) == 0) {                                                              \
                split_rows(slab_cur, BMs + ntap - 1);                                       \
                __syncthreads();                                                            \
            }                                                                               \
        }                                                                                   \
        compute(slab_cur, w_cur, (tapv));                                                   \
    }
    // the first operand DMAs go out BEFORE the residual preload below: that preload waits for its own global loads (11 k of a
    // 35 k-tick out-projection + LayerNorm launch sat in front of the first DMA, tools/probes/slab_phase_stamps.py) and the two
    // round trips now overlap
    SLAB_STAMP(1);
    if constexpr (LEAD == 0) {
        issue_slab(slab0, 0);
        issue_w(wt0, 0, 0);
    } else if (dma_wave) {  // with the second step's weight tile: two tiles are in flight from here on.  ONE branch around all three
        issue_slab_l(slab0, 0, true);  // requests: behind a join whose other side has requests pending hipcc takes them for the newest
        issue_w_l(wt0, 0, 0, true);
        issue_w_l(wt1, ntap == 1 ? 1 : 0, ntap == 1 ? 0 : 1, ncc * ntap > 1);
    }
    float prm[LN ? 4 : 1];
    if (tid < S_BN) {
        const int n = n0 + tid;
        const bool nv = n < p.N;
        prm[0] = (p.bias && nv) ? p.bias[n] : 0.f;
        if constexpr (LN) {  // (one column tile: n0 == 0)
            prm[1] = nv ? p.ln_g[n] : 0.f;
            prm[2] = nv ? p.ln_b[n] : 0.f;
            prm[3] = (nv && p.dot_w) ? p.dot_w[n] : 0.f;
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < MI; ++b) acc[a][b] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if ((LN || DEFER) && res_in_acc) {
        const T* R = (const T*)(LN ? p.res : p.epi_res) + (size_t)ub * S * p.ldc;
        const bool rnorm = DEFER && p.epi_res_stats != nullptr;
        const size_t rowbase0 = (size_t)ub * S;
        // Every load of the preload is issued before the first one is waited for.  (Until r04 each 16-byte load sat under its own
        // N-tail branch, and hipcc puts a vmcnt(0) behind a load it cannot move out of an exec-masked block: 2 * MI serial round
        // trips - twelve at 192-row tiles, the "residual preload 11.2 k ticks" of tools/probes/slab_phase_stamps.py.)  The tile
        // that lies wholly inside N - the common case - takes a branch-free path by workgroup-uniform dispatch.
        auto preload = [&](auto full_c) {
            constexpr bool FULL = decltype(full_c)::value;
            // (groups of GP row blocks, one after the other, measured r04: GP = 2 at 192-row tiles costs the C3 step 1 ms - three
            // dependent round trips per workgroup in front of its first MFMA - and saves no register: the pressure was elsewhere)
            constexpr int GP = MI;
#pragma unroll
            for (int g0 = 0; g0 < MI; g0 += GP) {
            float rmean[GP], rrstd[GP];
            int tr[GP];
#pragma unroll
            for (int gi = 0; gi < GP; ++gi) {
                const int t = t0 + wm * (MI * 16) + (g0 + gi) * 16 + fr;
                tr[gi] = t >= S ? S - 1 : t;  // rows past the utterance end are never stored
                rmean[gi] = 0.f;
                rrstd[gi] = 1.f;
            }
            if (rnorm) {
                float2 pq[GP][4];
#pragma unroll
                for (int gi = 0; gi < GP; ++gi) {
                    const float2* ps = (const float2*)p.epi_res_stats + (rowbase0 + tr[gi]) * p.epi_res_parts;
#pragma unroll
                    for (int q = 0; q < 4; ++q) pq[gi][q] = ps[q < p.epi_res_parts ? q : 0];  // unconditional: a clamped index, masked below
                }
                const float invn = 1.0f / (float)p.N;
#pragma unroll
                for (int gi = 0; gi < GP; ++gi) {
#pragma unroll
                    for (int q = 1; q < 4; ++q) if (q >= p.epi_res_parts) pq[gi][q] = make_float2(0.f, 0.f);
                    const float s1 = (pq[gi][0].x + pq[gi][1].x) + (pq[gi][2].x + pq[gi][3].x);
                    const float s2 = (pq[gi][0].y + pq[gi][1].y) + (pq[gi][2].y + pq[gi][3].y);
                    rmean[gi] = s1 * invn;
                    rrstd[gi] = 1.0f / sqrtf(fmaxf(__builtin_fmaf(-rmean[gi], rmean[gi], s2 * invn), 0.f) + p.ln_eps);
                }
            }
            if constexpr (FULL) {
                if constexpr (sizeof(T) == 4) {
#pragma unroll
                    for (int gi = 0; gi < GP; ++gi)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const T* src = R + (size_t)tr[gi] * p.ldc + n0 + wn * 64 + j * 32 + fg * 8;
                            const float4 q0 = *(const float4*)src, q1 = *(const float4*)(src + 4);
                            acc[2 * j][g0 + gi] = (f32x4_t){q0.x, q0.y, q0.z, q0.w};
                            acc[2 * j + 1][g0 + gi] = (f32x4_t){q1.x, q1.y, q1.z, q1.w};
                        }
                } else {
                    uint4 rq[GP][2];
#pragma unroll
                    for (int gi = 0; gi < GP; ++gi)
#pragma unroll
                        for (int j = 0; j < 2; ++j) rq[gi][j] = *(const uint4*)(R + (size_t)tr[gi] * p.ldc + n0 + wn * 64 + j * 32 + fg * 8);
#pragma unroll
                    for (int gi = 0; gi < GP; ++gi)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const unsigned w4[4] = {rq[gi][j].x, rq[gi][j].y, rq[gi][j].z, rq[gi][j].w};
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                acc[2 * j + (e >> 1)][g0 + gi][(2 * e) & 3] = unpack_lo<T>(w4[e]);
                                acc[2 * j + (e >> 1)][g0 + gi][(2 * e + 1) & 3] = unpack_hi<T>(w4[e]);
                            }
                        }
                }
                if (rnorm) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int n = n0 + wn * 64 + j * 32 + fg * 8;
#pragma unroll
                        for (int r = 0; r < 8; ++r) {
                            const float gvr = p.epi_res_g[n + r], bvr = p.epi_res_b[n + r];
#pragma unroll
                            for (int gi = 0; gi < GP; ++gi)
                                acc[2 * j + (r >> 2)][g0 + gi][r & 3] = __builtin_fmaf((acc[2 * j + (r >> 2)][g0 + gi][r & 3] - rmean[gi]) * rrstd[gi], gvr, bvr);
                        }
                    }
                }
            } else {
#pragma unroll
                for (int gi = 0; gi < GP; ++gi) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int n = n0 + wn * 64 + j * 32 + fg * 8;
                        const T* src = R + (size_t)tr[gi] * p.ldc + n;
                        float rv[8];
#pragma unroll
                        for (int r = 0; r < 8; ++r) rv[r] = (n + r < p.N) ? Num<T>::to_f32(src[r]) : 0.f;
                        if (rnorm) {
#pragma unroll
                            for (int r = 0; r < 8; ++r)
                                rv[r] = n + r < p.N ? __builtin_fmaf((rv[r] - rmean[gi]) * rrstd[gi], p.epi_res_g[n + r], p.epi_res_b[n + r]) : 0.f;
                        }
#pragma unroll
                        for (int r = 0; r < 8; ++r) acc[2 * j + (r >> 2)][g0 + gi][r & 3] = rv[r];
                    }
                }
            }
            if (MI > GP) __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (n0 + S_BN <= p.N) preload(BoolC<true>{});
        else preload(BoolC<false>{});
    }
    if (tid < S_BN) {  // (published by the first step's barrier; the epilogues read them after many more)
        sprm[tid] = prm[0];
        if constexpr (LN) {
            sprm[S_BN + tid] = prm[1];
            sprm[2 * S_BN + tid] = prm[2];
            sprm[3 * S_BN + tid] = prm[3];
        }
    }
    SLAB_STAMP(6);
    if constexpr (LEAD == 0) {
    for (int cc = 0; cc < ncc; cc += 2) {
        for (int tap = 0; tap < ntap; tap += 2) {
            FS2_SLAB_STEP(slab0, slab1, wt0, wt1, cc, tap)
            if (tap + 1 < ntap) FS2_SLAB_STEP(slab0, slab1, wt1, wt0, cc, tap + 1)
        }
        if (cc + 1 < ncc) {
            for (int tap = 0; tap < ntap; tap += 2) {
                FS2_SLAB_STEP(slab1, slab0, wt1, wt0, cc + 1, tap)
                if (tap + 1 < ntap) FS2_SLAB_STEP(slab1, slab0, wt0, wt1, cc + 1, tap + 1)
            }
        }
    }
    } else {
        // ---- lead-2 K loop: the weight tile of step s + 2 is requested at the top of step s, into the third stage ----
        // In the loop above a tile is asked for exactly one step before it is read, so a step is never shorter than one round trip
        // to L2, whatever its MFMA work; at 128- and 192-row tiles (1024 / 1536 MFMA cycles per step and SIMD) the trip is the
        // longer of the two.  Here step s = (cc, tap) reads weight stage s % 3 and slab stage cc & 1, and at its top
        //   1. waits with a COUNTED vmcnt: vector-memory operations retire in issue order, so leaving exactly the instructions
        //      issued behind tile s in flight (tile s + 1, and the next channel block's slab where that went out behind it)
        //      means tile s and everything older has landed;
        //   2. barrier: everyone's share has, and every wave has left step s - 1 - stage (s + 2) % 3 and the other slab are free;
        //   3. requests tile s + 2 (pointwise: the next step's slab first, it is read one step earlier).
        // (Nothing pins the requests to the top of the step: in the compiled loop hipcc spreads them through the step's MFMAs, some as
        //  late as its end, so tile s + 2 leaves between one and two steps before it is read, not a full two.  Left so on purpose: a
        //  DMA issue costs its wave 100-150 cycles next to MFMAs, and fourteen of them in a block in front of the first fragment read
        //  is what the interleaving avoids; a variant pinned by a sched_barrier was not measured.)
        // Conv launches (LEAD = 2, taps a multiple of 3: the stage of a step is tap % 3, a static name): the next channel block's
        // slab goes out at tap 0 BEHIND that step's weight tile, so the waits of taps 1 and 2 leave it in flight (DWI + DSI).
        // Every step issues the same instructions (dead requests go out of range), so each count is a compile-time number; the
        // loop exists twice, for the DMA waves and for the others, instead of holding its requests under a branch (at a join
        // hipcc's LDS-DMA scoreboard turns "maybe issued" into a vmcnt(0) in front of the fragment reads).
        // Same MFMA sequence per output element as the loop above: bit-identical results.
        const int nsteps = ncc * ntap;
        auto kloop = [&](auto dmaw_c) {
            constexpr bool DMAW = decltype(dmaw_c)::value;
            // The counts are right only while the DMA instructions of a step reach the queue in SOURCE order (slab group before weight
            // group in the pointwise form, weight group before slab group in the conv form).  hipcc keeps that order in this build (every
            // DMA rewrites M0, which serialises them; checked in the ISA of each step instance), but nothing in the language promises it
            // for stores into LDS objects it can prove distinct: after a compiler update, read the ISA again - the bit-equality tests
            // of tests/test_gpu_slab_lead.py are the only net that would catch a reordering.
#define FS2_LEAD_WAIT(cnt)                                                                                              \
            /* vmcnt(cnt) (the other waves: none) + lgkmcnt(0), then the BARE barrier: __syncthreads()'s fence counts a */  \
            /* pending LDS-DMA as a pending LDS write and drains it with a vmcnt(0) of its own                          */  \
            __builtin_amdgcn_s_waitcnt(DMAW ? (0x0070 | (cnt)) : 0xC07F);                                               \
            __builtin_amdgcn_s_barrier();
            if constexpr (LEAD == 1) {
#define FS2_LEAD_STEP(slab_cur, slab_nxt, w_cur, w_nn, sv)                                                              \
                {                                                                                                       \
                    FS2_LEAD_WAIT(DWI)                                                                                  \
                    if constexpr (DMAW) {                                                                               \
                        issue_slab_l(slab_nxt, (sv) + 1, (sv) + 1 < nsteps);                                            \
                        issue_w_l(w_nn, (sv) + 2, 0, (sv) + 2 < nsteps);                                                \
                    }                                                                                                   \
                    compute(slab_cur, w_cur, 0);                                                                        \
                }
                // (the first step stands in front of the loop: with it at the loop header hipcc's scoreboard, merging the prologue's
                //  requests with the loop's own, put a vmcnt(0) behind the header's barrier - every sixth step fell back to one step
                //  of lead; so placed, the routed 32-row forms have none.  The taller forms still keep one, ISA-checked: they are
                //  reachable with knob 242 only.)
                FS2_LEAD_STEP(slab0, slab1, wt0, wt2, 0)
                for (int s = 1; s < nsteps; s += 6) {
                    FS2_LEAD_STEP(slab1, slab0, wt1, wt0, s)
                    if (s + 1 >= nsteps) break;
                    FS2_LEAD_STEP(slab0, slab1, wt2, wt1, s + 1)
                    if (s + 2 >= nsteps) break;
                    FS2_LEAD_STEP(slab1, slab0, wt0, wt2, s + 2)
                    if (s + 3 >= nsteps) break;
                    FS2_LEAD_STEP(slab0, slab1, wt1, wt0, s + 3)
                    if (s + 4 >= nsteps) break;
                    FS2_LEAD_STEP(slab1, slab0, wt2, wt1, s + 4)
                    if (s + 5 >= nsteps) break;
                    FS2_LEAD_STEP(slab0, slab1, wt0, wt2, s + 5)
                }
#undef FS2_LEAD_STEP
            } else {
                // tile s + 2 of step (ccv, tapv): two taps on, wrapping into the next channel block
#define FS2_LEAD_STEP(slab_cur, slab_nxt, w_cur, w_nn, ccv, tapv, cnt, slab_req)                                        \
                {                                                                                                       \
                    FS2_LEAD_WAIT(cnt)                                                                                  \
                    if constexpr (DMAW) {                                                                               \
                        int t2 = (tapv) + 2, c2 = (ccv);                                                                \
                        if (t2 >= ntap) { t2 -= ntap; ++c2; }                                                           \
                        issue_w_l(w_nn, c2, t2, c2 < ncc);                                                              \
                        if constexpr (slab_req) issue_slab_l(slab_nxt, (ccv) + 1, (ccv) + 1 < ncc);                     \
                    }                                                                                                   \
                    compute(slab_cur, w_cur, (tapv));                                                                   \
                }
#define FS2_LEAD_BLOCK(slab_cur, slab_nxt, ccv)                                                                         \
                {                                                                                                       \
                    FS2_LEAD_STEP(slab_cur, slab_nxt, wt0, wt2, ccv, 0, DWI, true)                                      \
                    FS2_LEAD_STEP(slab_cur, slab_nxt, wt1, wt0, ccv, 1, DWI + DSI, false)                               \
                    FS2_LEAD_STEP(slab_cur, slab_nxt, wt2, wt1, ccv, 2, DWI + DSI, false)                               \
                    for (int tap = 3; tap < ntap; tap += 3) {                                                           \
                        FS2_LEAD_STEP(slab_cur, slab_nxt, wt0, wt2, ccv, tap, DWI, false)                               \
                        FS2_LEAD_STEP(slab_cur, slab_nxt, wt1, wt0, ccv, tap + 1, DWI, false)                           \
                        FS2_LEAD_STEP(slab_cur, slab_nxt, wt2, wt1, ccv, tap + 2, DWI, false)                           \
                    }                                                                                                   \
                }
                static_assert(DWI + DSI <= 15, "vmcnt's low four bits");
                for (int cc = 0;; cc += 2) {
                    FS2_LEAD_BLOCK(slab0, slab1, cc)
                    if (cc + 1 >= ncc) break;
                    FS2_LEAD_BLOCK(slab1, slab0, cc + 1)
                    if (cc + 2 >= ncc) break;
                }
#undef FS2_LEAD_BLOCK
#undef FS2_LEAD_STEP
            }
#undef FS2_LEAD_WAIT
        };
        if (dma_wave) kloop(BoolC<true>{});
        else kloop(BoolC<false>{});
        dma_drain();  // the dead requests of the last two steps: landed before the epilogues reuse the operand buffers behind their barrier
    }
    SLAB_STAMP(2);
#undef FS2_SLAB_STEP

    if constexpr (LN) {
        // ---- fused row epilogue: the workgroup owns whole rows (tiles_n == 1) ----
        // LayerNorm(act(acc + bias) [+ res]) with two-pass statistics: lane partials -> lane-group
        // shuffles -> one LDS exchange between the four column waves; optional predictor head.
        const size_t rowbase = (size_t)ub * S;
        // On a SIMD the epilogue's VALU instructions and the MFMA passes of the other resident wave mostly ADD UP
        // (profiles/HISTORY.md §4, §7; for the K = 256 launches this epilogue is as many issue cycles as the K loop), so the
        // per-element selects that only matter for N < 256, for ReLU or for the predictor head are compiled out
        // of the common case by workgroup-uniform dispatch - same arithmetic, same order, same results.
        const bool full = p.N == S_BN;
        {   // ReLU as max(v, lo) with lo = 0 / -inf: one instruction either way, no per-element select
            const float lo = p.relu ? 0.f : -__builtin_inff();
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int n = wn * 64 + wcol(ni, fg);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float bvv = sprm[n + r];
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi) acc[ni][mi][r] = fmaxf(acc[ni][mi][r] + bvv, lo);
                }
            }
            if (p.drop_p > 0.f) {
                // nn.Dropout between the sub-layer and its residual add (model.py:117-121: x = norm(x + dropout(sublayer(x)))): the
                // stand-alone kernel's mask (dropout_bits over the element index row * N + col of the (M, N) product), applied to the
                // fp32 value before the residual - the backward regenerates it from the same (seed, key)
                const uint32_t thr = (uint32_t)(p.drop_p * 16777216.0f);
                const float dsc = 1.f / (1.f - p.drop_p);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int t = t0 + wm * (MI * 16) + mi * 16 + fr;
                    const uint64_t e0 = (uint64_t)(rowbase + (t < S ? t : S - 1)) * (uint64_t)p.N;
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        const int n = wn * 64 + wcol(ni, fg);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            acc[ni][mi][r] = dropout_bits(p.drop_seed, p.drop_key, e0 + (uint64_t)(n + r)) >= thr ? acc[ni][mi][r] * dsc : 0.f;
                    }
                }
            }
            if (!full) {  // columns past N hold act(0 + 0): make them exact zeros for the row sums
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const int n = wn * 64 + wcol(ni, fg);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n + r >= p.N) {
#pragma unroll
                            for (int mi = 0; mi < MI; ++mi) acc[ni][mi][r] = 0.f;
                        }
                }
            }
        }
        if (p.res && !res_in_acc) {
            const T* R = (const T*)p.res;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                int t = t0 + wm * (MI * 16) + mi * 16 + fr;
                if (t >= S) t = S - 1;  // rows past the utterance end are never stored
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const int n = wn * 64 + wcol(ni, fg);
                    if (n + 3 < p.N) {
                        float rv[4];
                        if constexpr (sizeof(T) == 4) {
                            const float4 q = *(const float4*)(R + (rowbase + t) * p.ldc + n);
                            rv[0] = q.x; rv[1] = q.y; rv[2] = q.z; rv[3] = q.w;
                        } else {
                            const uint2 q = *(const uint2*)(R + (rowbase + t) * p.ldc + n);
                            rv[0] = unpack_lo<T>(q.x); rv[1] = unpack_hi<T>(q.x);
                            rv[2] = unpack_lo<T>(q.y); rv[3] = unpack_hi<T>(q.y);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[ni][mi][r] += rv[r];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (n + r < p.N) acc[ni][mi][r] += Num<T>::to_f32(R[(rowbase + t) * p.ldc + n + r]);
                    }
                }
            }
        }
        if (p.z_out) {  // training tape: the pre-norm rows, in the output dtype, 8 consecutive channels per store
            OutT* __restrict__ Zn = (OutT*)p.z_out + rowbase * p.ldc;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int t = t0 + wm * (MI * 16) + mi * 16 + fr;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int n = wn * 64 + j * 32 + fg * 8;
                    if (t < S && n < p.N) {
                        OutT* dst = Zn + (size_t)t * p.ldc + n;
                        const f32x4_t a0 = acc[2 * j][mi], a1 = acc[2 * j + 1][mi];
                        if (n + 7 < p.N) {
                            if constexpr (sizeof(OutT) == 4) {
                                *(float4*)dst = make_float4(a0[0], a0[1], a0[2], a0[3]);
                                *(float4*)(dst + 4) = make_float4(a1[0], a1[1], a1[2], a1[3]);
                            } else {
                                *(uint4*)dst = make_uint4(pack2<OutT>(a0[0], a0[1]), pack2<OutT>(a0[2], a0[3]),
                                                          pack2<OutT>(a1[0], a1[1]), pack2<OutT>(a1[2], a1[3]));
                            }
                        } else {
#pragma unroll
                            for (int r = 0; r < 8; ++r)
                                if (n + r < p.N) dst[r] = Num<OutT>::from_f32(r < 4 ? a0[r] : a1[r - 4]);
                        }
                    }
                }
            }
        }
        __syncthreads();  // every wave is done with the operand buffers: reuse them for the exchange
        SLAB_STAMP(3);
        float* red = (float*)slab0;  // [4 column waves][BMs rows]
        const float* lnp = sprm + S_BN;  // [gamma 256 | beta 256 | head weight 256], parked at the top of the kernel
        const float invn = 1.0f / (float)p.N;
        float mean[MI], rstd[MI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            float sm = 0.f;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) sm += (acc[ni][mi][0] + acc[ni][mi][1]) + (acc[ni][mi][2] + acc[ni][mi][3]);
            sm = group4_sum(sm);
            if (fg == 0) red[wn * BMs + wm * (MI * 16) + mi * 16 + fr] = sm;
        }
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int row = wm * (MI * 16) + mi * 16 + fr;
            mean[mi] = ((red[row] + red[BMs + row]) + (red[2 * BMs + row] + red[3 * BMs + row])) * invn;
        }
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)  // acc <- acc - mean once: the variance and the normalisation both use it
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[ni][mi][r] -= mean[mi];
        auto sq_dev = [&](auto full_c) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                float q = 0.f;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const int n = wn * 64 + wcol(ni, fg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float d = (decltype(full_c)::value || n + r < p.N) ? acc[ni][mi][r] : 0.f;
                        q = __builtin_fmaf(d, d, q);  // explicit: an SLP-packed mul + add would round differently per variant
                    }
                }
                q = group4_sum(q);
                if (fg == 0) red[wn * BMs + wm * (MI * 16) + mi * 16 + fr] = q;
            }
        };
        if (full) sq_dev(BoolC<true>{});
        else sq_dev(BoolC<false>{});
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int row = wm * (MI * 16) + mi * 16 + fr;
            const float var = ((red[row] + red[BMs + row]) + (red[2 * BMs + row] + red[3 * BMs + row])) * invn;
            rstd[mi] = 1.0f / sqrtf(var + p.ln_eps);
        }
        OutT* __restrict__ Cn = p.C ? (OutT*)p.C + rowbase * p.ldc : nullptr;
        SLAB_STAMP(4);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int t = t0 + wm * (MI * 16) + mi * 16 + fr;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = wn * 64 + j * 32 + fg * 8;  // 8 consecutive channels of fragments 2j, 2j+1
                float y[8];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float4 g4 = *(const float4*)(lnp + n + 4 * h), b4 = *(const float4*)(lnp + S_BN + n + 4 * h);
                    const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[4 * h + r] = __builtin_fmaf(acc[2 * j + h][mi][r] * rstd[mi], gg[r], bb[r]);
                }
                if (Cn && t < S && n < p.N) {
                    OutT* dst = Cn + (size_t)t * p.ldc + n;
                    if (n + 7 < p.N) {
                        if constexpr (sizeof(OutT) == 4) {
                            *(float4*)dst = make_float4(y[0], y[1], y[2], y[3]);
                            *(float4*)(dst + 4) = make_float4(y[4], y[5], y[6], y[7]);
                        } else {
                            *(uint4*)dst = make_uint4(pack2<OutT>(y[0], y[1]), pack2<OutT>(y[2], y[3]),
                                                      pack2<OutT>(y[4], y[5]), pack2<OutT>(y[6], y[7]));
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 8; ++r) if (n + r < p.N) dst[r] = Num<OutT>::from_f32(y[r]);
                    }
                }
            }
        }
        SLAB_STAMP(5);
        if (p.dot_w) {  // predictor head (rare): the normalised values once more, times the head weights
            float dsum[MI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                dsum[mi] = 0.f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int n = wn * 64 + j * 32 + fg * 8;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float4 g4 = *(const float4*)(lnp + n + 4 * h), b4 = *(const float4*)(lnp + S_BN + n + 4 * h);
                        const float4 w4 = *(const float4*)(lnp + 2 * S_BN + n + 4 * h);
                        const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
                        const float ww[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            dsum[mi] = __builtin_fmaf(__builtin_fmaf(acc[2 * j + h][mi][r] * rstd[mi], gg[r], bb[r]), ww[r], dsum[mi]);
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                float d = dsum[mi];
                d = group4_sum(d);
                if (fg == 0) red[wn * BMs + wm * (MI * 16) + mi * 16 + fr] = d;
            }
            __syncthreads();
            if (wn == 0 && fg == 0) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int row = wm * (MI * 16) + mi * 16 + fr, t = t0 + row;
                    if (t < S) {
                        const float d = ((red[row] + red[BMs + row]) + (red[2 * BMs + row] + red[3 * BMs + row])) + p.dot_b;
                        p.pred[rowbase + t] = (p.mask && p.mask[rowbase + t]) ? 0.f : d;
                    }
                }
            }
        }
        return;
    }
    OutT* __restrict__ C = (OutT*)p.C + ((size_t)ks * p.M + (size_t)ub * S) * p.ldc;
    // lane (fr, fg) holds, for output row t, the 8 consecutive channels n .. n+7 of each fragment
    // pair (2j, 2j+1): one 16-byte (bf16) / two 16-byte (fp32) stores, 64 contiguous bytes per row
    // across the four lane groups; the two halves (j = 0, 1) of a row's 128-byte line go out back to back
    float bv[2][8];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + fg * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) bv[j][r] = sprm[n - n0 + r];
    }
    // ReLU and the N-tail checks are compiled out of the common case by workgroup-uniform dispatch (see the
    // LayerNorm epilogue above): at K = 256 this store loop is as many issue cycles as the K loop
    // gate_c: out = gate[row][col] > 0 ? v : 0 with `gate` a tensor of C's layout and dtype - the ReLU backward of a data-gradient
    // product (training step: dh = (dc2 . W2) o [h > 0]) folded into the store instead of a 3-tensor elementwise pass
    auto store = [&](auto relu_c, auto full_c, auto gate_c, auto drop_c, auto rs_c) {
    // rs_c: the row-scaled product (GemmArgs::rs_stats): v = rstd * acc - (rstd * mean) * wg + bias'
    float rsr[decltype(rs_c)::value ? MI : 1], rsm[decltype(rs_c)::value ? MI : 1], wgv[decltype(rs_c)::value ? 2 : 1][8];
    if constexpr (decltype(rs_c)::value) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int t = t0 + wm * (MI * 16) + mi * 16 + fr;
            const float2 q = ((const float2*)p.rs_stats)[(size_t)ub * S + (t < S ? t : S - 1)];
            rsr[mi] = q.x;
            rsm[mi] = q.y;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + fg * 8;
#pragma unroll
            for (int r = 0; r < 8; ++r) wgv[j][r] = n + r < p.N ? p.rs_wg[n + r] : 0.f;
        }
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int t = t0 + wm * (MI * 16) + mi * 16 + fr;
        if (t >= S) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + fg * 8;
            if (!decltype(full_c)::value && n >= p.N) continue;
            float v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if constexpr (decltype(rs_c)::value) v[r] = __builtin_fmaf(acc[2 * j + (r >> 2)][mi][r & 3], rsr[mi], __builtin_fmaf(-rsm[mi], wgv[j][r], bv[j][r]));
                else v[r] = acc[2 * j + (r >> 2)][mi][r & 3] + bv[j][r];
                if constexpr (decltype(relu_c)::value) v[r] = fmaxf(v[r], 0.f);
            }
            if constexpr (decltype(drop_c)::value) {
                // nn.Dropout behind the activation (the FFN's hidden tensor in training mode, model.py:94-106): fs2_op_dropout's mask over the
                // (M, N) product, in the store instead of a read-modify-write pass over the (M, filter) tensor
                const uint32_t thr = (uint32_t)(p.drop_p * 16777216.0f);
                const float dsc = 1.f / (1.f - p.drop_p);
                const uint64_t e0 = ((uint64_t)ub * S + (uint64_t)t) * (uint64_t)p.N + (uint64_t)n;
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = dropout_bits(p.drop_seed, p.drop_key, e0 + r) >= thr ? v[r] * dsc : 0.f;
            }
            if constexpr (decltype(gate_c)::value) {
                const OutT* gt = (const OutT*)((const char*)p.gate + ((size_t)ub * S * p.ldc + (size_t)t * p.ldc + n) * sizeof(OutT));
                if (decltype(full_c)::value || n + 7 < p.N) {
                    float gv[8];
                    if constexpr (sizeof(OutT) == 4) {
                        const float4 q0 = *(const float4*)gt, q1 = *(const float4*)(gt + 4);
                        gv[0] = q0.x; gv[1] = q0.y; gv[2] = q0.z; gv[3] = q0.w; gv[4] = q1.x; gv[5] = q1.y; gv[6] = q1.z; gv[7] = q1.w;
                    } else {
                        const uint4 q = *(const uint4*)gt;
                        const unsigned w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            gv[2 * e] = unpack_lo<OutT>(w4[e]);
                            gv[2 * e + 1] = unpack_hi<OutT>(w4[e]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[r] = gv[r] > 0.f ? v[r] * p.gate_scale : 0.f;
                } else {
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[r] = (n + r < p.N && Num<OutT>::to_f32(gt[r]) > 0.f) ? v[r] * p.gate_scale : 0.f;
                }
            }
            if constexpr (sizeof(OutT) == 4) {
                if (p.C_lo) {  // the fp32 result as two bf16 tensors, head + tail (the split-arithmetic attention's operands): same bytes
                    const size_t off = ((size_t)ub * S + t) * p.ldc + n;
                    uint4 hq, lq;
                    split_bf16x3(make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])),
                                 make_uint4(__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7])), hq, lq);
                    bf16* dh = (bf16*)p.C + off;
                    bf16* dl = (bf16*)p.C_lo + off;
                    if (decltype(full_c)::value || n + 7 < p.N) {
                        *(uint4*)dh = hq;
                        *(uint4*)dl = lq;
                    } else {
                        const unsigned hw[4] = {hq.x, hq.y, hq.z, hq.w}, lw[4] = {lq.x, lq.y, lq.z, lq.w};
#pragma unroll
                        for (int r = 0; r < 8; ++r)
                            if (n + r < p.N) {
                                ((unsigned short*)dh)[r] = (unsigned short)(hw[r >> 1] >> (16 * (r & 1)));
                                ((unsigned short*)dl)[r] = (unsigned short)(lw[r >> 1] >> (16 * (r & 1)));
                            }
                    }
                    continue;
                }
            }
            OutT* dst = (OutT*)((char*)C + (unsigned)(t * p.ldc + n) * (unsigned)sizeof(OutT));  // one utterance < 4 GiB
            if (decltype(full_c)::value || n + 7 < p.N) {
                if constexpr (sizeof(OutT) == 4) {
                    *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                    *(float4*)(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                } else {
                    *(uint4*)dst = make_uint4(pack2<OutT>(v[0], v[1]), pack2<OutT>(v[2], v[3]),
                                              pack2<OutT>(v[4], v[5]), pack2<OutT>(v[6], v[7]));
                }
            } else {
#pragma unroll
                for (int r = 0; r < 8; ++r) if (n + r < p.N) dst[r] = Num<OutT>::from_f32(v[r]);
            }
        }
    }
    };
    if constexpr (DEFER) {
        // Deferred-LayerNorm epilogue (rows wider than one tile): v = act(acc + bias) + res, stored as it is, plus this
        // column tile's sum(v), sum(v^2) per row -> stats_out[row][column tile]; the consumers (depth-wise conv,
        // normalise-only LayerNorm, the next epilogue's residual) finish mean / rstd from the tiles' parts.
        // The residual may itself be such a pre-norm tensor: then it is normalised on load from ITS parts.
        const size_t rowbase = (size_t)ub * S;
        const float lo = p.relu ? 0.f : -__builtin_inff();
        float a1[MI], a2[MI];
        auto body = [&](auto full_c) {
            constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int t = t0 + wm * (MI * 16) + mi * 16 + fr;
            a1[mi] = a2[mi] = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + wn * 64 + j * 32 + fg * 8;
                float v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = fmaxf(acc[2 * j + (r >> 2)][mi][r & 3] + bv[j][r], lo);
                // (a residual reaches this epilogue inside the accumulators only: res_in_acc; one behind a ReLU the launcher refuses -
                //  the in-epilogue path cost 35 registers at 192-row tiles and was dead code in every launch of the forward)
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if (!FULL && n + r >= p.N) v[r] = 0.f;
                    a1[mi] += v[r];
                    a2[mi] = __builtin_fmaf(v[r], v[r], a2[mi]);
                }
                if (t < S && (FULL || n < p.N)) {
                    OutT* dst = (OutT*)((char*)C + (unsigned)(t * p.ldc + n) * (unsigned)sizeof(OutT));
                    if (FULL || n + 7 < p.N) {
                        if constexpr (sizeof(OutT) == 4) {
                            *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                            *(float4*)(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                        } else {
                            *(uint4*)dst = make_uint4(pack2<OutT>(v[0], v[1]), pack2<OutT>(v[2], v[3]),
                                                      pack2<OutT>(v[4], v[5]), pack2<OutT>(v[6], v[7]));
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 8; ++r) if (n + r < p.N) dst[r] = Num<OutT>::from_f32(v[r]);
                    }
                }
            }
        }
        };
        if (n0 + S_BN <= p.N) body(BoolC<true>{});
        else body(BoolC<false>{});
        if (p.stats_out) {  // one (sum, sum of squares) per row per column TILE: the four column waves meet in LDS
            __syncthreads();  // every wave is done with the operand buffers
            float2* red = (float2*)slab0;  // [4 column waves][BMs rows]
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const float s1 = group4_sum(a1[mi]), s2 = group4_sum(a2[mi]);
                if (fg == 0) red[wn * BMs + wm * (MI * 16) + mi * 16 + fr] = make_float2(s1, s2);
            }
            __syncthreads();
            for (int row = tid; row < BMs; row += 512) {
                const int t = t0 + row;
                if (t < S) {
                    const float2 q0 = red[row], q1 = red[BMs + row], q2 = red[2 * BMs + row], q3 = red[3 * BMs + row];
                    ((float2*)p.stats_out)[(rowbase + t) * (size_t)tiles_n + bn] =
                        make_float2((q0.x + q1.x) + (q2.x + q3.x), (q0.y + q1.y) + (q2.y + q3.y));
                }
            }
        }
        return;
    }
    const bool fulln = n0 + S_BN <= p.N;  // this column tile lies wholly inside N
    if (p.rs_stats) {  // (the launcher admits the row-scaled product without ReLU / gate / dropout / head + tail store, bf16 only)
        if constexpr (sizeof(T) == 2 && sizeof(OutT) == 2 && !SPLIT) {
            if (fulln) store(BoolC<false>{}, BoolC<true>{}, BoolC<false>{}, BoolC<false>{}, BoolC<true>{});
            else store(BoolC<false>{}, BoolC<false>{}, BoolC<false>{}, BoolC<false>{}, BoolC<true>{});
        }
    } else if (p.gate) {  // (the launcher admits a gate without ReLU only)
        if (fulln) store(BoolC<false>{}, BoolC<true>{}, BoolC<true>{}, BoolC<false>{}, BoolC<false>{});
        else store(BoolC<false>{}, BoolC<false>{}, BoolC<true>{}, BoolC<false>{}, BoolC<false>{});
    } else if (p.drop_p > 0.f) {  // (the launcher admits the store's dropout with ReLU, bf16 / fp32 in = out, no gate)
        if (fulln) store(BoolC<true>{}, BoolC<true>{}, BoolC<false>{}, BoolC<true>{}, BoolC<false>{});
        else store(BoolC<true>{}, BoolC<false>{}, BoolC<false>{}, BoolC<true>{}, BoolC<false>{});
    } else if (fulln) {
        if (p.relu) store(BoolC<true>{}, BoolC<true>{}, BoolC<false>{}, BoolC<false>{}, BoolC<false>{});
        else store(BoolC<false>{}, BoolC<true>{}, BoolC<false>{}, BoolC<false>{}, BoolC<false>{});
    } else {
        if (p.relu) store(BoolC<true>{}, BoolC<false>{}, BoolC<false>{}, BoolC<false>{}, BoolC<false>{});
        else store(BoolC<false>{}, BoolC<false>{}, BoolC<false>{}, BoolC<false>{}, BoolC<false>{});
    }
#else
    (void)p;
#endif
}

template <typename T, typename OutT, int MI, bool LN, bool SPLIT = false, bool DEFER = false, bool XPRE = false, int LEAD = 0>
static int launch_slab_t(const GemmArgs& a0, hipStream_t stream) {
    GemmArgs a = a0;
    a.xcd_remap = tuning_of(a0.tune).slab_xcd_remap;
    const int BMs = SlabCfg<MI>::BM;
    if (a.xcd_remap == 2) {  // column pairs per XCD: 4 / 8 / 16 column tiles, a weight panel that does not fit an XCD's L2, whole rounds of row tiles
        const int tn = (a.N + S_BN - 1) / S_BN, rows = (a.M / a.S) * ((a.S + BMs - 1) / BMs);
        const bool ok = (tn == 4 || tn == 8 || tn == 16) && a.ksplit <= 1 && rows % (16 / tn) == 0 &&
                        (size_t)a.N * a.K * sizeof(T) > (size_t)3 << 20;
        if (!ok) a.xcd_remap = 1;
    }
    if (a.taps == 1) a.S = a.M;  // plain GEMM: one "utterance" of M rows
    const int tiles = (a.M / a.S) * ((a.S + BMs - 1) / BMs) * ((a.N + S_BN - 1) / S_BN) * (a.ksplit > 1 ? a.ksplit : 1);
    hipLaunchKernelGGL((gemm_conv_slab_kernel<T, OutT, MI, LN, SPLIT, DEFER, XPRE, LEAD>), dim3(tiles), dim3(512), 0, stream, a);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

// Split launches whose caller holds plain fp32 weights (the operator-level entry points with Tuning::split_f32, knob 501: tests
// only - an engine packs its weights once at fs2_finalize, GemmArgs::w_presplit): packed on the fly into a block that lives for
// this launch, allocated and freed in STREAM ORDER (no process-wide buffer: until r05 one static grow-only block was shared by
// every caller and stream).  Not under stream capture.
static int presplit_on_the_fly(GemmArgs& a, hipStream_t stream, void** tmp) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return FS2_ERR_STATE;
    const size_t bytes = (size_t)a.N * a.K * 4;
    if (hipMallocAsync(tmp, bytes, stream) != hipSuccess) return FS2_ERR_NOMEM;
    const int r = launch_presplit_pack((const float*)a.W, *tmp, (size_t)a.N * a.K, stream);
    a.W = *tmp;
    a.w_presplit = 1;
    return r;
}

template <typename T, typename OutT, bool ZR = false>
static int launch_t(const GemmArgs& a, hipStream_t stream) {
    static bool attr_set = false;
    const size_t smem = 4 * TILE_BYTES;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)gemm_conv_kernel<T, OutT, ZR>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return FS2_ERR_HIP;
        attr_set = true;
    }
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    hipLaunchKernelGGL((gemm_conv_kernel<T, OutT, ZR>), dim3(tiles), dim3(256), smem, stream, a);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

// ---- the (in, out) storage dtype pairs, once ------------------------------------------------------------------------------------
// A kernel family's epilogue accepts a SET of pairs; the router tests membership, the launcher turns the pair into <T, OutT> and
// instantiates the members of the set only.
enum : unsigned {
    DT_F32 = 1, DT_BF16 = 2, DT_F16 = 4, DT_BF16_F32 = 8, DT_F16_F32 = 16,
    DT_SAME = DT_F32 | DT_BF16 | DT_F16,            // the slab kernel's LayerNorm and deferred epilogues
    DT_ALL = DT_SAME | DT_BF16_F32 | DT_F16_F32,    // its plain epilogue; the 128x128 kernel
    DT_TO_F32 = DT_F32 | DT_BF16_F32 | DT_F16_F32,  // the 128x128 kernel's zero_rows form (the mel head)
};
static unsigned dtype_pair(int in, int out) {
    if (in == FS2_F32) return out == FS2_F32 ? DT_F32 : 0;
    if (in == FS2_BF16) return out == FS2_BF16 ? DT_BF16 : out == FS2_F32 ? DT_BF16_F32 : 0;
    if (in == FS2_F16) return out == FS2_F16 ? DT_F16 : out == FS2_F32 ? DT_F16_F32 : 0;
    return 0;
}
template <unsigned SET, typename F>
static int with_dtypes(int in, int out, F&& f) {  // f(Ty<T>, Ty<OutT>)
    const unsigned p = dtype_pair(in, out);
    if constexpr ((SET & DT_F32) != 0) if (p == DT_F32) return f(Ty<float>{}, Ty<float>{});
    if constexpr ((SET & DT_BF16) != 0) if (p == DT_BF16) return f(Ty<bf16>{}, Ty<bf16>{});
    if constexpr ((SET & DT_BF16_F32) != 0) if (p == DT_BF16_F32) return f(Ty<bf16>{}, Ty<float>{});
    if constexpr ((SET & DT_F16) != 0) if (p == DT_F16) return f(Ty<f16>{}, Ty<f16>{});
    if constexpr ((SET & DT_F16_F32) != 0) if (p == DT_F16_F32) return f(Ty<f16>{}, Ty<float>{});
    return FS2_ERR_SHAPE;
}
static constexpr unsigned slab_dtypes(bool ln, bool defer) { return ln || defer ? DT_SAME : DT_ALL; }
static constexpr unsigned flat_dtypes(bool zr) { return zr ? DT_TO_F32 : DT_ALL; }

// ---- the route -------------------------------------------------------------------------------------------------------------------
// Feature rules, as data: an optional member of GemmArgs that only some kernels implement has ONE row saying which families have
// it, which other members it cannot be combined with, and what the shape / dtypes / knobs must satisfy.  A request that breaks a
// row of a member it carries is FS2_ERR_SHAPE.  (Members without a row - bias, res, dot_w, relu, split - are every family's, or the
// LayerNorm epilogue's, which route_gemm handles as a whole.)
enum : unsigned {  // router-internal feature bits behind GemmFeature's
    GF_KSPLIT = 1u << 17,
    GF_RS_NARROW = 1u << 18,  // rs_stats with N < 192: the 128x128 kernel's form of it (GF_RS: the slab / persistent kernels')
};
enum : unsigned {  // conditions a row can need
    ND_AUTO = 1u << 0, ND_NOT_FLAT = 1u << 1, ND_SLAB_KNOB = 1u << 2,  // gemm_variant: 0 (no family forced) / not 1 / 0 or a forced slab tile height (3-7)
    ND_WIDE = 1u << 3,                                                  // N >= 192
    ND_TILES = 1u << 4,                                                 // whole utterances and an odd tap count: what the slab kernel tiles
    ND_SAME_DT = 1u << 5, ND_IN_F32 = 1u << 6, ND_OUT_F32 = 1u << 7, ND_IN_16 = 1u << 8,
    ND_RELU = 1u << 9, ND_RS_WG = 1u << 10, ND_TAPS1 = 1u << 11,
    ND_SPLIT_ON = 1u << 12,                                             // GemmArgs::split or Tuning::split_f32
    ND_KDIV = 1u << 13,                                                 // ksplit divides the channel blocks
};
struct FeatureRule { unsigned feature, not_with, needs, families; };
static constexpr unsigned FAM_FLAT = 1u << GEMM_FLAT128, FAM_SLAB = 1u << GEMM_SLAB, FAM_PERSIST = 1u << GEMM_PERSIST;
static constexpr unsigned GF_OTHER_EPI = GF_LN | GF_STATS | GF_EPIRES;  // members of the plain epilogue exclude the other two epilogues
static const FeatureRule kFeatureRules[] = {
    // the plain store's dropout: behind a ReLU (the FFN's hidden tensor)
    {GF_DROP, GF_GATE | GF_STATS | GF_EPIRES | GF_KSPLIT | GF_ZR, ND_RELU | ND_AUTO | ND_WIDE | ND_TILES | ND_SAME_DT, FAM_SLAB},
    // a narrow head behind a folded LayerNorm (the mel Linear), 16-bit operands / the row-scaled product of the plain 16-bit epilogue
    {GF_RS_NARROW, GF_OTHER_EPI | GF_RELU | GF_GATE | GF_CLO | GF_KSPLIT | GF_DROP, ND_RS_WG | ND_TAPS1 | ND_IN_16, FAM_FLAT},
    {GF_RS, GF_OTHER_EPI | GF_RELU | GF_GATE | GF_CLO | GF_KSPLIT | GF_DROP, ND_RS_WG | ND_NOT_FLAT | ND_TILES | ND_IN_16 | ND_SAME_DT, FAM_SLAB | FAM_PERSIST},
    {GF_ZR, GF_LN, 0, FAM_FLAT},  // the mel head with zeroed pad rows
    {GF_GATE, GF_OTHER_EPI | GF_RELU, ND_AUTO | ND_WIDE | ND_TILES | ND_SAME_DT, FAM_SLAB},
    // weights packed as heads + tails are the split arithmetic's own format
    {GF_WPRE, GF_KSPLIT, ND_SPLIT_ON | ND_AUTO | ND_WIDE | ND_TILES | ND_IN_F32, FAM_SLAB},
    {GF_CLO, GF_OTHER_EPI | GF_GATE | GF_KSPLIT | GF_DROP, ND_AUTO | ND_WIDE | ND_TILES | ND_IN_F32 | ND_OUT_F32, FAM_SLAB},  // head + tail store: plain fp32 epilogue
    {GF_KSPLIT, GF_OTHER_EPI | GF_BIAS | GF_RELU | GF_GATE, ND_SLAB_KNOB | ND_WIDE | ND_TILES | ND_OUT_F32 | ND_KDIV, FAM_SLAB},  // plain fp32 store only
    // the deferred-LayerNorm epilogue; its residual rides in the accumulators' initial value: no activation in between
    {GF_STATS, 0, 0, FAM_SLAB | FAM_PERSIST},
    {GF_EPIRES, GF_RELU, 0, FAM_SLAB | FAM_PERSIST},
};

struct Request { unsigned feats, have; };  // what the rules look at: the members a request carries, the conditions that hold
static Request classify(const GemmArgs& a, int in_dtype, int out_dtype) {
    const Tuning& tn = tuning_of(a.tune);
    const int v = tn.gemm_variant, ke = 128 / (int)elem_bytes(in_dtype);
    const bool ln = a.ln_g != nullptr;  // the LayerNorm epilogue takes precedence over the deferred one, and has a dropout of its own
    const unsigned feats = (a.bias ? GF_BIAS : 0) | (a.relu ? GF_RELU : 0) | (ln ? GF_LN : 0) | (!ln && a.stats_out ? GF_STATS : 0) |
                           (!ln && a.epi_res ? GF_EPIRES : 0) | (!ln && a.drop_p > 0.f ? GF_DROP : 0) | (a.gate ? GF_GATE : 0) |
                           (a.rs_stats ? (a.N < 192 ? GF_RS_NARROW : GF_RS) : 0) | (a.zero_rows ? GF_ZR : 0) | (a.C_lo ? GF_CLO : 0) |
                           (a.w_presplit ? GF_WPRE : 0) | (a.ksplit > 1 ? GF_KSPLIT : 0);
    const unsigned have = (v == 0 ? ND_AUTO : 0) | (v != 1 ? ND_NOT_FLAT : 0) | (v == 0 || (v >= 3 && v <= 7) ? ND_SLAB_KNOB : 0) |
                          (a.N >= 192 ? ND_WIDE : 0) | (a.S > 0 && a.M % a.S == 0 && (a.taps & 1) ? ND_TILES : 0) |
                          (in_dtype == out_dtype ? ND_SAME_DT : 0) | (in_dtype == FS2_F32 ? ND_IN_F32 : 0) | (out_dtype == FS2_F32 ? ND_OUT_F32 : 0) |
                          (is_16bit(in_dtype) ? ND_IN_16 : 0) | (a.relu ? ND_RELU : 0) | (a.rs_wg ? ND_RS_WG : 0) | (a.taps == 1 ? ND_TAPS1 : 0) |
                          (a.split || tn.split_f32 ? ND_SPLIT_ON : 0) | (a.ksplit > 1 && (a.Cin / ke) % a.ksplit == 0 ? ND_KDIV : 0);
    return {feats, have};
}
// the rows of the members in `subject`: their combinations and conditions, and (family != GEMM_NONE) that the family has them
static bool rules_hold(const Request& q, unsigned subject, int family) {
    for (const FeatureRule& r : kFeatureRules) {
        if (!(subject & r.feature)) continue;
        if ((q.feats & r.not_with) || (r.needs & ~q.have)) return false;
        if (family != GEMM_NONE && !(r.families & (1u << family))) return false;
    }
    return true;
}

// The slab kernel's lead-2 K loop (three weight stages, tile s + 2 requested at step s; bit-identical to the two-stage loop): 0 = not
// taken, 1 = its pointwise form, 2 = its conv form.  It EXISTS for 16-bit operands stored as they came in, no split-K: pointwise
// launches at tiles of up to 128 rows with any epilogue and at 192 rows with the plain epilogue (with the LayerNorm or the deferred
// epilogue the 192-row form needs 256 registers and spills: not built, never routed), conv launches with taps a multiple of 3
// (k = 3, 9) at up to 128 rows.  It is TAKEN (Tuning::slab_lead = 1) for the launch classes that measured faster with it - a choice by
// (taps, K, tile height, epilogue), never by the batch.
static int slab_lead_form(int knob, const GemmArgs& a, int in_dtype, int out_dtype, int mi, bool ln, bool defer) {
    if (!knob || !is_16bit(in_dtype) || out_dtype != in_dtype || a.ksplit > 1) return 0;
    const bool plain = !ln && !defer;
    const int form = a.taps == 1 ? (mi <= 4 || (mi == 6 && plain) ? 1 : 0) : (a.taps % 3 == 0 && mi <= 4 ? 2 : 0);
    if (knob >= 2 || !form) return form;
    // Measured per launch class (tools/bench_slab_lead.py, profiles/slab_lead_ab.md) with operands cold, which is the state the
    // ENCODER's launches are in inside a forward (profiles/HISTORY.md section 4, "Round 4"): faster by more than the spread of the
    // two-stage rounds are  k = 9 plain at 128 rows (encoder conv1, 45.4 -> 38.6 us),  K = 1024 + LayerNorm at 32 rows (encoder conv2,
    // 25.0 -> 21.6)  and  k = 3 + LayerNorm at 32 rows (19.6 -> 15.6).  Exactly these three (taps, K or tile, epilogue) classes are
    // routed, whatever their N and Cin, which were not varied.  Everything else keeps the two-stage loop: the four-step K = 256
    // launches (0.3-0.5 us lower, at their spread), other tap counts, K and tile heights (not measured), and the decoder's launches,
    // whose input the previous launch has just written - with warm operands the loop is neutral there.
    if (form == 2) return (mi == 4 && plain && a.taps == 9) || (mi == 1 && ln && a.taps == 3) ? 2 : 0;
    return mi == 1 && ln && a.K == 1024 ? 1 : 0;
}

// One launch for the request as it stands.  With ln_g set the question is whether the slab kernel takes it with the LayerNorm in
// its epilogue (whole rows per workgroup); GEMM_NONE with FS2_OK and M > 0 then means it does not.
static GemmRoute route_one(const GemmArgs& a, int in_dtype, int out_dtype) {
    GemmRoute r;
    if (a.M <= 0 || a.N <= 0) return r;
    const int ke = 128 / (int)elem_bytes(in_dtype), e16 = 16 / (int)elem_bytes(in_dtype);
    if (a.K % ke || a.Cin % ke || a.ldx % e16 || a.K != a.taps * a.Cin || a.ldc % 4) return GemmRoute{FS2_ERR_SHAPE};
    const Tuning& tn = tuning_of(a.tune);
    const Request q = classify(a, in_dtype, out_dtype);
    const bool ln = q.feats & GF_LN, defer = q.feats & (GF_STATS | GF_EPIRES), tiles_ok = q.have & ND_TILES;
    const int variant = tn.gemm_variant;  // 0 = auto, 1 = 128x128 register-staged, 3/4/5 = slab kernel with 128/192/256-row tiles, 6/7 = 32/64-row
    const int ksp = a.ksplit > 1 ? a.ksplit : 1;
    // A member that only the 128x128 kernel has decides the family by itself, and the slab kernel's members are then not looked at
    // (a gate or C_lo beside zero_rows is ignored, not refused): kept as it always was, the statuses are pinned by the route test.
    // (Every conflicting pair of members stands in one row of the table only: a new member names its conflicts in its own row.)
    const bool flat_only = q.feats & (GF_RS_NARROW | GF_ZR);
    const unsigned subject = flat_only ? q.feats & (GF_DROP | GF_RS_NARROW | GF_ZR) : q.feats;
    if (!rules_hold(q, subject, GEMM_NONE)) return GemmRoute{FS2_ERR_SHAPE};

    int family = GEMM_FLAT128, mi = 0;
    if (flat_only) {
    } else if (tiles_ok && (variant == 6 || variant == 7)) {
        family = GEMM_SLAB; mi = variant == 6 ? 1 : 2;
    } else if (tiles_ok && variant >= 3 && variant <= 5 && !(ln && variant == 5)) {
        family = GEMM_SLAB; mi = variant == 3 ? 4 : (variant == 4 || defer) ? 6 : 8;
    } else if (variant == 0 && tiles_ok && a.N >= 192) {
        // One 512-thread workgroup per CU: pick the row-tile height that minimises
        // (rounds over the 256 CUs) x (tile rows + ~40 rows' worth of prologue/epilogue), measured
        // on MI355X (tools/bench_ops.py); fall back to the flat 128x128 kernel when utterances are
        // so short that per-utterance tiles would be mostly padding.
        const int S = a.taps == 1 ? a.M : a.S, nutt = a.M / S, tiles_n = (a.N + S_BN - 1) / S_BN;
        int best = 0;
        long best_cost = 0, best_rows = 0;
        static const int kHeights[5] = {1, 2, 4, 6, 8};  // x32 rows; 32/64-row tiles keep small-M launches
        for (int hi = 0; hi < 5; ++hi) {                  // (the encoder's) spread over all CUs
            const int h = kHeights[hi];
            if ((ln || defer) && h > 6) continue;  // 256-row tiles spill with the fused LayerNorm epilogue and with the deferred one (r04: 24 spills even without its in-epilogue residual path; selected nowhere)
            const long bm = h * 32, tm = (S + bm - 1) / bm;
            const long tiles = (long)nutt * tm * tiles_n * ksp;
            long cost = ((tiles + 255) / 256) * (bm + 40);
            // long reductions (K >= 4096: the data-gradient convs of the training step, K = taps * filter): every workgroup
            // streams the whole K x 256 weight panel out of L2, and tiles x panel bytes over the ~10 TB/s the L2s deliver
            // together becomes the bound before the CUs fill - in the same units (one row of MFMA work per K) that is ~1 per
            // tile.  C5 encoder conv1 dgrad (M = 2048, N = 1024, K = 36864): 256 x 32-row tiles 500 us -> 128 x 64-row tiles.
            if (a.K / ksp >= 4096) cost = cost > tiles ? cost : tiles;
            if (!best || cost < best_cost) { best = h; best_cost = cost; best_rows = (long)nutt * tm * bm; }
        }
        if (best_rows <= 2L * a.M || (q.feats & (GF_CLO | GF_WPRE | GF_RS))) {  // (the head + tail store / pre-split weights / row-scaled product exist in this kernel only)
            // more tiles than CUs: one workgroup per CU walks them, the next tile's first operands under this tile's epilogue
            // (gemm_persist.hip; same tile height, same arithmetic per element - bit-identical)
            family = !ln && tn.gemm_persist && gemm_persist_supported(a, in_dtype, out_dtype, best) && gemm_persist_pays(a, best) ? GEMM_PERSIST : GEMM_SLAB;
            mi = best;
        }
    }
    if (ln && family != GEMM_SLAB) return r;  // only the slab kernel has the LayerNorm epilogue
    if (!rules_hold(q, subject, family)) return GemmRoute{FS2_ERR_SHAPE};
    r.family = family; r.mi = mi;
    if (family == GEMM_FLAT128) {
        r.zr = q.feats & GF_ZR;
        if (!(dtype_pair(in_dtype, out_dtype) & flat_dtypes(r.zr))) return GemmRoute{FS2_ERR_SHAPE};
    } else if (family == GEMM_SLAB) {
        r.ln = ln; r.defer = defer;
        if (!(dtype_pair(in_dtype, out_dtype) & slab_dtypes(ln, defer))) return GemmRoute{FS2_ERR_SHAPE};
        r.split = in_dtype == FS2_F32 && out_dtype == FS2_F32 && (q.have & ND_SPLIT_ON);
        r.xpre = r.split && a.taps > 1;  // conv launches of the split arithmetic: the slab is split in place when it lands
        r.presplit = r.split && !a.w_presplit;
        r.lead = slab_lead_form(tn.slab_lead, a, in_dtype, out_dtype, mi, ln, defer);
    }
    return r;
}

static GemmRoute route_request(const GemmArgs& a, int in_dtype, int out_dtype) {
    const auto no = [](int status) { return GemmRoute{status}; };
    const auto on = [](int family, int mi) { GemmRoute r; r.family = family; r.mi = mi; return r; };
    if (!is_storage_dtype(in_dtype) || !is_storage_dtype(out_dtype)) return no(FS2_ERR_ARG);
    // f16 operands: the forward's epilogues only (no dropout, gate, pre-norm tape, split-K, head sums: the training step's and the predictors')
    if ((in_dtype == FS2_F16 || out_dtype == FS2_F16) && (a.drop_p > 0.f || a.gate || a.z_out || a.ksplit > 1 || a.head_out || a.C_lo)) return no(FS2_ERR_ARG);
    const Tuning& tn = tuning_of(a.tune);
    if (a.head_out) {  // head sums instead of the rows: the persistent kernel's deferred epilogue only (callers ask gemm_head_supported first)
        if (a.ln_g || !gemm_head_supported(a, in_dtype, out_dtype)) return no(FS2_ERR_SHAPE);
        return on(GEMM_PERSIST, 6);
    }
    if (!a.ln_g) {
        if (a.drop_p > 0.f) {
            if (!rules_hold(classify(a, in_dtype, out_dtype), GF_DROP, GEMM_NONE)) return no(FS2_ERR_SHAPE);
        } else if (tn.gemm_wres && tn.gemm_variant == 0 && a.ksplit <= 1 && gemm_wres_supported(a, in_dtype, out_dtype, tn.gemm_wres == 2)) {
            // K = 256 bf16: the column tile's weights live in registers, row tiles stream (gemm_wres.hip; bit-identical results)
            return on(GEMM_WRES, 0);
        }
        return route_one(a, in_dtype, out_dtype);
    }
    // fused row epilogue requested: the slab kernel (whole rows per workgroup, N <= 256), else GEMM -> ln_tmp followed by the
    // stand-alone LayerNorm kernel (same arithmetic, one more HBM round trip)
    if (a.z_out && a.N > S_BN) return no(FS2_ERR_SHAPE);  // the pre-norm store exists in the one-column-tile epilogue only
    if (a.drop_p > 0.f && (a.N > S_BN || !a.z_out)) return no(FS2_ERR_SHAPE);  // the epilogue's dropout: one-column-tile fused form only (training tape)
    if (a.N <= S_BN && in_dtype == out_dtype) {
        const GemmRoute r = route_one(a, in_dtype, out_dtype);
        if (r.status != FS2_OK || r.family != GEMM_NONE) return r;
    }
    if (a.z_out) return no(FS2_ERR_SHAPE);  // not fusable for this shape: the caller takes its two-launch path (nothing is launched)
    if (!a.ln_tmp || in_dtype != out_dtype) return no(FS2_ERR_ARG);
    GemmArgs g = a;
    g.ln_g = nullptr;
    g.C = a.ln_tmp;
    GemmRoute r = route_one(g, in_dtype, out_dtype);
    if (r.status != FS2_OK || r.family == GEMM_NONE) return r;
    if (!layernorm_rows_ok(a.N)) return no(FS2_ERR_SHAPE);  // refused before the GEMM goes out, not behind it
    r.two_launch = true;
    return r;
}
GemmRoute route_gemm(const GemmArgs& a, int in_dtype, int out_dtype) {
    GemmRoute r = route_request(a, in_dtype, out_dtype);
    r.in_dtype = in_dtype; r.out_dtype = out_dtype;
    return r;
}

// ---- the launcher: executes a route, decides nothing ------------------------------------------------------------------------------
template <int MI, bool LN, bool DEFER>
static int launch_slab_e(const GemmRoute& r, const GemmArgs& a, hipStream_t stream) {
    return with_dtypes<slab_dtypes(LN, DEFER)>(r.in_dtype, r.out_dtype, [&](auto t, auto o) {
        using T = typename decltype(t)::type;
        using OutT = typename decltype(o)::type;
        if constexpr (sizeof(T) == 4) {
            if (r.xpre) return launch_slab_t<T, OutT, MI, LN, true, DEFER, true>(a, stream);
            if (r.split) return launch_slab_t<T, OutT, MI, LN, true, DEFER>(a, stream);
        } else if constexpr (sizeof(OutT) == 2 && MI <= 6) {  // the lead-2 K loop: 16-bit in and out (slab_lead_form says which forms exist)
            if constexpr (MI <= 4 || (!LN && !DEFER)) {
                if (r.lead == 1) return launch_slab_t<T, OutT, MI, LN, false, DEFER, false, 1>(a, stream);
            }
            if constexpr (MI <= 4) {
                if (r.lead == 2) return launch_slab_t<T, OutT, MI, LN, false, DEFER, false, 2>(a, stream);
            }
        }
        return launch_slab_t<T, OutT, MI, LN, false, DEFER>(a, stream);
    });
}
template <int MI>
static int launch_slab_mi(const GemmRoute& r, const GemmArgs& a, hipStream_t stream) {
    if constexpr (MI <= 6) {  // the 256-row form of the LayerNorm and deferred epilogues spills: not built, never routed
        if (r.ln) return launch_slab_e<MI, true, false>(r, a, stream);
        if (r.defer) return launch_slab_e<MI, false, true>(r, a, stream);
    }
    return launch_slab_e<MI, false, false>(r, a, stream);
}
template <bool ZR>
static int launch_flat(const GemmRoute& r, const GemmArgs& a, hipStream_t stream) {
    return with_dtypes<flat_dtypes(ZR)>(r.in_dtype, r.out_dtype, [&](auto t, auto o) {
        return launch_t<typename decltype(t)::type, typename decltype(o)::type, ZR>(a, stream);
    });
}

int launch_route(const GemmRoute& r, const GemmArgs& a_in, hipStream_t stream) {
    if (r.status != FS2_OK || r.family == GEMM_NONE) return r.status;
    GemmArgs a = a_in;
    if (r.two_launch) { a.ln_g = nullptr; a.C = a_in.ln_tmp; }
    void* tmp = nullptr;
    if (r.presplit) {
        const int st = presplit_on_the_fly(a, stream, &tmp);
        if (st != FS2_OK) { if (tmp) (void)hipFreeAsync(tmp, stream); return st; }
    }
    int st;
    if (r.family == GEMM_FLAT128) st = r.zr ? launch_flat<true>(r, a, stream) : launch_flat<false>(r, a, stream);
    else if (r.family == GEMM_PERSIST) st = launch_gemm_persist(a, r.in_dtype, r.mi, stream);
    else if (r.family == GEMM_WRES) st = launch_gemm_wres(a, r.in_dtype, stream);
    else if (r.mi == 1) st = launch_slab_mi<1>(r, a, stream);
    else if (r.mi == 2) st = launch_slab_mi<2>(r, a, stream);
    else if (r.mi == 4) st = launch_slab_mi<4>(r, a, stream);
    else if (r.mi == 6) st = launch_slab_mi<6>(r, a, stream);
    else st = launch_slab_mi<8>(r, a, stream);
    if (tmp) (void)hipFreeAsync(tmp, stream);  // behind the launch that reads it, in stream order
    if (st != FS2_OK || !r.two_launch) return st;
    LayerNormArgs l;
    l.x = a_in.ln_tmp; l.res = a_in.res; l.gamma = a_in.ln_g; l.beta = a_in.ln_b; l.y = a_in.C;
    l.dot_w = a_in.dot_w; l.dot_b = a_in.dot_b; l.mask = a_in.mask; l.pred = a_in.pred;
    l.M = a_in.M; l.H = a_in.N; l.eps = a_in.ln_eps;
    return launch_layernorm(l, r.out_dtype, stream);
}

bool gemm_presplit_eligible(int N, int K) { return N >= 192 && K % 32 == 0; }

// fp32 (N, K) weights -> the split arithmetic's operand format, same size, in place or into `out`: per 32-channel chunk (128 bytes)
// 16-byte slot s < 4 = the bf16 heads of channels [4s, 4s + 4) and [16 + 4s, 16 + 4s + 4), slot 4 + s = their tails
__global__ __launch_bounds__(256) void presplit_pack_kernel(const float* w, unsigned char* out, size_t npairs) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const size_t chunk = i >> 2;
    const int sl = (int)(i & 3);
    const uint4 c0 = *(const uint4*)(w + chunk * 32 + 4 * sl), c1 = *(const uint4*)(w + chunk * 32 + 16 + 4 * sl);
    uint4 h, l;
    split_bf16x3(c0, c1, h, l);
    *(uint4*)(out + chunk * 128 + sl * 16) = h;        // (in place: a thread writes the two slots it has read)
    *(uint4*)(out + chunk * 128 + (4 + sl) * 16) = l;
}
int launch_presplit_pack(const float* w, void* out, size_t n_values, hipStream_t stream) {
    if (n_values % 32) return FS2_ERR_SHAPE;
    if (!n_values) return FS2_OK;
    const size_t np = n_values / 8;
    hipLaunchKernelGGL(presplit_pack_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, w, (unsigned char*)out, np);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

// ---- split-K: planes -> output ----------------------------------------------------------------------------------------------
// out[i] = [out[i] +] ((p0 + p1) + p2) + ... in plane order (deterministic), 4 elements per thread, 16-byte plane loads
template <typename OutT>
__global__ __launch_bounds__(256) void split_k_reduce_kernel(const float* __restrict__ part, OutT* __restrict__ out, size_t n, int ksplit,
                                                             int accumulate) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    float4 a = *(const float4*)(part + i);
    for (int s = 1; s < ksplit; ++s) {
        const float4 b = *(const float4*)(part + (size_t)s * n + i);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if constexpr (sizeof(OutT) == 4) {
        float4* o = (float4*)(out + i);
        if (accumulate) { const float4 c = *o; a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w; }
        *o = a;
    } else {
        uint2* o = (uint2*)(out + i);
        if (accumulate) {
            const uint2 c = *o;
            a.x += unpack_lo<OutT>(c.x); a.y += unpack_hi<OutT>(c.x);
            a.z += unpack_lo<OutT>(c.y); a.w += unpack_hi<OutT>(c.y);
        }
        *o = make_uint2(pack2<OutT>(a.x, a.y), pack2<OutT>(a.z, a.w));
    }
}

int launch_split_k_reduce(const float* part, void* out, size_t n, int ksplit, int accumulate, int out_dtype, hipStream_t stream) {
    if (!part || !out || ksplit < 1 || n % 4 || (out_dtype != FS2_F32 && out_dtype != FS2_BF16)) return FS2_ERR_ARG;
    if (!n) return FS2_OK;
    const dim3 g((unsigned)((n / 4 + 255) / 256));
    if (out_dtype == FS2_F32) hipLaunchKernelGGL(split_k_reduce_kernel<float>, g, dim3(256), 0, stream, part, (float*)out, n, ksplit, accumulate);
    else hipLaunchKernelGGL(split_k_reduce_kernel<bf16>, g, dim3(256), 0, stream, part, (bf16*)out, n, ksplit, accumulate);
    return hipGetLastError() == hipSuccess ? FS2_OK : FS2_ERR_HIP;
}

// A long reduction over few row tiles (the encoder-side data-gradient convs of the training step: M = 8192, N = 256, K = 9 x 1024)
// leaves every workgroup streaming the whole K x 256 weight panel at the CU's ~64 GB/s ingest rate with half the CUs idle
// (130 us at C2).  Split over K so that 128-row tiles fill the chip once: 1/ksplit of the panel per workgroup.
int gemm_splitk_choice(int M, int N, int Cin, int taps, int S, int in_dtype) {
    if (!is_f32_or_bf16(in_dtype)) return 1;  // split-K is the training step's
    const int ke = 128 / (int)elem_bytes(in_dtype);
    if (taps < 1 || !(taps & 1) || N < 192 || Cin % ke || (long)taps * Cin < 2048) return 1;
    if (taps == 1) S = M;
    if (S <= 0 || M % S) return 1;
    const long tiles = (long)(M / S) * ((S + 127) / 128) * ((N + S_BN - 1) / S_BN);
    int best = 1;
    for (int k = 2; k <= 8; k *= 2)
        if ((Cin / ke) % k == 0 && tiles * k <= 256 && (long)taps * Cin / k >= 1024) best = k;
    return best;
}

}  // namespace fs2

#ifdef FS2_SLAB_PROBE
extern "C" int fs2_dbg_slab_phase_stamps(unsigned long long* out /*4 x 8, host*/) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fs2::g_slab_stamps), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -2;
}
#endif
