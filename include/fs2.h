/* C ABI of the MI355X-native FastSpeech2 / LightSpeech mel forward (libfs2_hip.so).
 *
 * The reference (MiniXC/LightningFastSpeech2) has no FFI layer: its "operator API" for this path is
 * the Python method  FastSpeech2.forward(targets: dict, inference) -> dict
 * (litfass/fastspeech2/fastspeech2.py:636-784) over a state_dict whose key names are fixed by the
 * module tree built at fastspeech2.py:242-438.  This header is what a binding for
 * that method binds (ctypes stub in INTEGRATION.md; the in-tree host mirror is
 * lightningfastspeech2_amd/model.py):
 *
 *   fs2_create / fs2_load_weight / fs2_finalize   <- FastSpeech2.__init__ + load_state_dict
 *                                                    (fastspeech2.py:46-491, :530-620): weights are
 *                                                    passed under the reference's own key names
 *   fs2_encode + fs2_decode                       <- FastSpeech2.forward(batch, inference=True)
 *                                                    (fastspeech2.py:636-731), split at the one point
 *                                                    where the output length T becomes known
 *                                                    (LengthRegulator, model.py:354-355)
 *
 * Plain pointers and sizes only; device pointers are HIP device addresses on the engine's device
 * (e.g. torch tensors' data_ptr()).  All work is enqueued on the caller's stream; no hidden streams,
 * no global state, one engine per device.  Every function returns a status code (0 = OK);
 * fs2_last_error() has the text.  No exceptions cross this boundary.
 */
#ifndef FS2_H_
#define FS2_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_ABI_VERSION 4
#define FS2_MAX_LAYERS 32
#define FS2_MAX_VARIANCES 4
#define FS2_MAX_PRIORS 8   /* hparams.priors: the shipped recipe lists five (scripts/train.sh:49: energy duration snr pitch srmr) */
#define FS2_NAME_LEN 32

enum fs2_status {
    FS2_OK = 0,
    FS2_ERR_HIP = 1,     /* a HIP runtime call or kernel launch failed */
    FS2_ERR_SHAPE = 2,   /* shape/config outside what the kernels support */
    FS2_ERR_ARG = 3,     /* null / inconsistent argument */
    FS2_ERR_WEIGHT = 4,  /* unknown weight name, wrong shape, or weights missing at finalize */
    FS2_ERR_STATE = 5,   /* call order violated (e.g. decode before encode) */
    FS2_ERR_NOMEM = 6
};

enum fs2_dtype {
    FS2_F32 = 0,
    FS2_BF16 = 1,
    FS2_MIXED = 2,    /* engine modes only (fs2_config.dtype): fp32 "front" + bf16 "back", see fs2_config.dtype */
    FS2_MIXED_X3 = 3, /* the same with the front's GEMMs / convs as bf16 x 3 split products of fp32 operands */
    FS2_F32_X3 = 4,   /* engine mode: F32 storage and row arithmetic everywhere, EVERY GEMM / conv as bf16 x 3 split products */
    FS2_F16 = 5,      /* storage / operator dtype: IEEE binary16 operands, fp32 accumulate.  Stores SATURATE: a value beyond +-65504 (an
                         infinity included) is stored as +-65504, NaN stays NaN, everything else rounds to nearest-even (subnormals
                         included) - on the device and in fs2_finalize's weight conversion alike.  Taken by fs2_op_gemm / _gemm_add /
                         _gemm_ln / _gemm_stats / _gemm_rowscale_dt, fs2_op_attention (+ _scratch_bytes), fs2_op_attn_out_ln, fs2_op_layernorm, fs2_op_dwconv,
                         fs2_op_convert and the vocoder (fs2_voc_config.dtype); every other operator (the training step's, bgemm, the
                         attention backward, the predictor, the row kernels of the front) answers FS2_ERR_ARG / FS2_ERR_SHAPE, a
                         *_supported query 0 */
    FS2_MIXED_F16_X3 = 6 /* engine mode: MIXED_X3's front, launch for launch; the back (decoder stack, the mel Linear's operands) in F16 */
};

/* Mirrors the hparams that shape FastSpeech2.forward (fastspeech2.py:46-130). */
typedef struct fs2_config {
    int32_t abi_version;   /* FS2_ABI_VERSION */
    int32_t dtype;         /* fs2_dtype: arithmetic mode. F32 = parity mode (fp32 MFMA, <=1e-3 vs the
                              reference); BF16 = throughput mode (bf16 storage + MFMA, fp32 accumulate,
                              fp32 softmax/LayerNorm statistics/predictor heads/bucketize);
                              MIXED = decision-safe throughput mode: everything a discrete decision depends on
                              (embedding, encoder, duration predictor and rounding, length regulator, variance
                              predictors and bucketize - model.py:259,299-309,315-333,434-438) runs as in F32, the
                              decoder and the mel head (where an error stays an error of O(bf16 rounding) in the
                              mel) as in BF16: durations / buckets follow the fp32 path's, at bf16 decoder speed;
                              MIXED_X3 = MIXED with the front's matrix products evaluated as hi*hi + hi*lo + lo*hi of
                              bf16 head/tail pairs split from the fp32 operands in registers (fp32 storage,
                              accumulation, attention, LayerNorm, heads; ~1e-5 relative per product instead of fp32's
                              6e-8 or bf16's 4e-3): 3 bf16 MFMAs per 32 k-values instead of 8 fp32 MFMAs;
                              F32_X3 = F32 with every GEMM / conv (both sides) evaluated that way: the parity mode's layout,
                              attention, LayerNorm, heads and decisions logic at about half its time (C2: 8.1 vs 15.2 ms per
                              forward); measured 1.4e-5 on the mel against F32 under equal decisions;
                              MIXED_F16_X3 = MIXED_X3 with the decoder's stored tensors and matrix operands in IEEE binary16 instead
                              of bf16 (three more mantissa bits at the same MFMA rate; saturating stores, see FS2_F16): the
                              front, and with it every decision, is MIXED_X3's bit for bit; the mel leaves as fp32 */
    int32_t n_phones;      /* len(phone2id) */
    int32_t hidden;        /* encoder_hidden == decoder_hidden */
    int32_t n_mels;
    int32_t dvec_dim;      /* 256 */
    int32_t max_frames;    /* int(max_length * sampling_rate / hop_length) = 2756 */
    int32_t pe_len;        /* rows of positional_encoding.pe (5000) */
    int32_t enc_layers, enc_heads, enc_filter, enc_depthwise;
    int32_t enc_kernels[FS2_MAX_LAYERS];
    int32_t dec_layers, dec_heads, dec_filter, dec_depthwise;
    int32_t dec_kernels[FS2_MAX_LAYERS];
    int32_t n_variances;   /* hparams.variances in order; level per variance in var_level (ABI v4), transform in var_cwt */
    char var_names[FS2_MAX_VARIANCES][FS2_NAME_LEN];
    int32_t var_nlayers[FS2_MAX_VARIANCES];
    int32_t var_kernel[FS2_MAX_VARIANCES];
    float var_mean[FS2_MAX_VARIANCES];  /* stats[var]["mean"/"std"] (model.py:406-407,434) */
    float var_std[FS2_MAX_VARIANCES];
    int32_t var_filter, var_nbins, var_depthwise;
    int32_t dur_nlayers, dur_kernel, dur_filter, dur_depthwise;
    int32_t n_priors;      /* hparams.priors (default []): PriorEmbedding rows added after the encoder */
    char prior_names[FS2_MAX_PRIORS][FS2_NAME_LEN];
    int32_t var_cwt[FS2_MAX_VARIANCES];  /* variance_transforms[i] == "cwt" (the class default for pitch, fastspeech2.py:60):
                              the CWT head of VarianceEncoder (model.py:412-431,445-461): predictor.linear is (10, filter),
                              mean_std_linear (2, filter) exists, bins are log-spaced; var_mean/var_std must be 0 / 1 */
    int32_t var_level[FS2_MAX_VARIANCES];  /* ABI v4: 0 = frame level (variance_levels[i] == "frame": predicted on the regulated frames,
                              model.py:315-333), 1 = phone level ("phone", model.py:276-294: predicted on the encoder output after the
                              duration predictor has run, its embedding added BEFORE the length regulator; (B, L) outputs) */
} fs2_config;

typedef struct fs2_engine fs2_engine;

/* Caller-owned DEVICE buffers fs2_decode fills (shapes use T returned by fs2_encode).  Any pointer
 * may be NULL to skip that output.  Mask bytes are 1 = pad, directly usable as torch.bool storage. */
typedef struct fs2_outputs {
    float* mel;                    /* (B, T, n_mels) fp32, pad rows included (fastspeech2.py:723) */
    float* duration_prediction;    /* (B, L) log(1+d) domain, 0 at pads (model.py:259,517-518) */
    int32_t* duration_rounded;     /* (B, L) (model.py:299-309) */
    uint8_t* src_mask;             /* (B, L) phones == 0 (fastspeech2.py:651) */
    uint8_t* tgt_mask;             /* (B, T) t >= total_b (model.py:358-361) */
    float* variances[FS2_MAX_VARIANCES];  /* (B, T) each - (B, L) for a phone-level variance -, 0 at pads (model.py:328); for a CWT
                                             variance the recomposed log-domain signal (exp of it = the reference's "reconstructed_signal") */
    float* var_spectrogram[FS2_MAX_VARIANCES];  /* CWT variances only: (B, T, 10) ((B, L, 10) at phone level) wavelet spectrogram, 0 at pads */
    float* var_mean_std[FS2_MAX_VARIANCES];     /* CWT variances only: (B, 2) utterance-level mean, std (model.py:414-415) */
} fs2_outputs;

int fs2_abi_version(void);
const char* fs2_status_string(int status);
const char* fs2_last_error(const fs2_engine* e);

int fs2_create(const fs2_config* cfg, fs2_engine** out);
int fs2_destroy(fs2_engine* e);
/* A second engine over the same device weights (finalized engines only; the weights are freed with the last holder): own workspace,
 * own host-side state.  One engine serves one caller thread at a time; an engine and its clones may run concurrently on different
 * streams - several forwards of FastSpeech2.forward in flight (generate.py:186-195 feeds the model chunk after chunk). */
int fs2_clone(const fs2_engine* src, fs2_engine** out);

/* One call per state_dict entry, reference key names, fp32 HOST data, torch shape.
 * Unknown names that belong to off-path modules are rejected with FS2_ERR_WEIGHT. */
int fs2_load_weight(fs2_engine* e, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);
/* Packs (conv weights tap-major, grouped 1x1 folded into the following pointwise conv), converts to
 * the arithmetic dtype and uploads.  FS2_ERR_WEIGHT if any tensor of the architecture is missing. */
int fs2_finalize(fs2_engine* e);

/* Phase 1: embedding + encoder + duration predictor + rounding/guard + prefix sums.
 *   phones   (B, L) int64 device, 0 = [PAD];  speaker (B, dvec_dim) fp32 device.
 *   forced_durations: NULL, or (B, L) int32 device durations used instead of the predicted ones.
 * Synchronises the stream once to return T = min(max_b sum_l d[b,l], max_frames). */
int fs2_encode(fs2_engine* e, const int64_t* phones, const float* speaker, int32_t B, int32_t L,
               const int32_t* forced_durations, void* hip_stream, int32_t* T_out);
/* Utterance-level priors for the NEXT fs2_encode (one-shot): (n_priors, B) fp32 device values, row p
 * = targets["priors_<prior_names[p]>"] (fastspeech2.py:687-692; PriorEmbedding, model.py:146-164).
 * Required before every fs2_encode when n_priors > 0. */
int fs2_set_priors(fs2_engine* e, const float* priors_device, int32_t B);
/* duration_stochastic=True (model.py:196-207, 258-268, 299-305): the stochastic duration predictor (fs2_sdp_* below) where the
 * conv + LayerNorm duration predictor runs, and its rounding rule (fs2_op_durations_stochastic).  Legal only between fs2_create and
 * the first fs2_load_weight (FS2_ERR_STATE later).  n_flows = dur_nlayers, hidden_channels = dur_filter, kernel_size = dur_kernel of
 * the config; dur_depthwise != 0 is refused (FS2_ERR_SHAPE, as the reference refuses it), and so is a shape fs2_sdp_supported
 * does not cover (hidden > 256 among them).  The conv predictor's rule dur_filter == hidden for dur_nlayers > 1 does not apply to this
 * predictor: fs2_create accepts such a config and the rule is judged at the first fs2_load_weight / at fs2_finalize of an engine that
 * was NOT switched (FS2_ERR_SHAPE there).  The engine then expects "variance_adaptor.duration_predictor.sdp.*" (training-only tensors accepted and
 * dropped) in place of the deterministic predictor's tensors.  fs2_clone shares the weights.  With fs2_set_graphs the encode phase
 * of a stochastic engine takes the plain path (the noise is a one-shot pointer of the call); the decode phase may still replay. */
int fs2_set_stochastic_duration(fs2_engine* e, int32_t on);
/* The noise of the NEXT fs2_encode of a stochastic engine (one-shot, like fs2_set_priors): (B, 2, L) fp32 device, standard normal
 * already scaled by noise_scale (sdp.py:335-338).  Required before every fs2_encode of a stochastic engine, forced durations or
 * not (FS2_ERR_STATE from fs2_encode otherwise); fs2_encode copies it into the engine's own buffer on its stream. */
int fs2_set_duration_noise(fs2_engine* e, const float* noise_device, int32_t B, int32_t L);
/* Per-utterance frame totals (untruncated) and zero-duration-guard flags of the last fs2_encode. */
int fs2_last_totals(const fs2_engine* e, int32_t* totals_host, int32_t* guard_host, int32_t B);
/* Phase 2: length regulator + variance encoders + decoder + mel linear, into caller buffers. */
int fs2_decode(fs2_engine* e, const fs2_outputs* out, void* hip_stream);

/* Workspace.  By default the engine keeps two grow-only device arenas of its own.  A caller that
 * wants every byte to come from its allocator (torch's caching allocator in the host mirror) asks for the sizes
 * and hands the buffers over; the engine then never calls hipMalloc/hipFree on the forward path.
 *   persist: live from fs2_encode to the end of fs2_decode (encoder output, durations, prefix sums); depends on (B, L)
 *   scratch: per-phase; for T = 0 the size fs2_encode needs, for T > 0 max(encode, decode at T frames)
 * fs2_set_workspace(NULL, 0, NULL, 0) returns to engine-owned arenas.  Between fs2_encode and fs2_decode only the
 * scratch buffer may be replaced (the usual pattern: T is known only after fs2_encode).  Buffers 256-byte aligned;
 * a buffer that is too small makes the next phase fail with FS2_ERR_NOMEM and the needed size in fs2_last_error. */
int fs2_workspace_bytes(const fs2_engine* e, int32_t B, int32_t L, int32_t T, size_t* persist_bytes, size_t* scratch_bytes);
int fs2_set_workspace(fs2_engine* e, void* persist_device, size_t persist_bytes, void* scratch_device, size_t scratch_bytes);
/* Data-parallel "global pad" mode: after fs2_encode, raise this shard's frame count to the maximum over
 * all ranks so that fs2_decode pads exactly as the whole batch would (T can only grow, <= max_frames). */
int fs2_set_frames(fs2_engine* e, int32_t T);
/* on = 1: fs2_decode writes zeros into the mel rows of pad frames (t >= the utterance's total) instead of the
 * reference's deterministic pad-row values - what the multi-GPU mel gather ships, fused into the mel GEMM's store. */
int fs2_set_zero_pad_mel(fs2_engine* e, int32_t on);

/* Parity taps: copy an intermediate of the last forward as fp32 into a caller DEVICE buffer.
 * what = "encoder_out" (B,L,H) | "regulated" | "adaptor_out" | "decoder_out" (B,T,H) |
 *        "bucket_<var>" (B,T) int32.  Requires fs2_set_debug(e, 1) before fs2_encode. */
int fs2_set_debug(fs2_engine* e, int32_t on);
/* A/B and parity aid: on = 0 runs every VariancePredictor as per-layer conv+LayerNorm launches, 1
 * (default) as the single-launch kernel where the shape allows it (bf16, filter 256, k = 3, dense). */
int fs2_set_fused_predictor(fs2_engine* e, int32_t on);
/* 1: fs2_decode replays its launches (~50: variance adaptor after the length regulator, decoder, mel head) as a hipGraph once
 * the same shape AND buffer addresses (outputs, arenas) are seen again - first sight runs plainly, second captures, later calls
 * are one hipGraphLaunch on an engine-owned stream ordered against the caller's with events.  Same kernels, same arguments:
 * results are bit-identical.  Off by default; debug taps, per-class profiling and forced buckets always take the
 * plain path; a caller workspace (fs2_set_workspace) is part of the signature.  fs2_graph_replays: how many decodes were replays (tests, diagnostics). */
int fs2_set_graphs(fs2_engine* e, int32_t on);
int64_t fs2_graph_replays(const fs2_engine* e);
/* A/B and parity aid: hidden sizes above 256 with depth-wise blocks (LightSpeech, model.py:73-93,541-558) run LayerNorm
 * deferred (default 1): the GEMM in front of a LayerNorm leaves pre-norm rows + row statistics, the depth-wise conv / the
 * next residual add normalise on load and the remaining LayerNorms are normalise-only passes; 0 = GEMM launch + LayerNorm
 * launch everywhere (the round-1 path). */
int fs2_set_deferred_layernorm(fs2_engine* e, int32_t on);
/* A/B: 1 (default) = inside a stack of wide depth-wise blocks (bf16) a block's closing LayerNorm is not materialised either: the
 * next block's in-projection runs on the pre-norm rows with gamma / beta folded into its weights (fs2_op_gemm_rowscale) and its
 * out-projection normalises the residual on load; 0 = one normalise-only pass per block.  Needs deferred LayerNorm on. */
int fs2_set_folded_layernorm(fs2_engine* e, int32_t on);
/* one kernel-selection switch of THIS engine: the values of fs2_op_set_gemm_variant below; clones made afterwards inherit it */
int fs2_set_tuning(fs2_engine* e, int32_t knob);
/* Parity aid (the analogue of the reference's teacher forcing of variance targets,
 * model.py:417-422): the NEXT fs2_decode embeds these (B, T) int32 device bucket indices for
 * variance `variance_index` instead of bucketizing its own prediction.  One-shot.  For a PHONE-level variance the indices
 * are (B, L) and are consumed by the NEXT fs2_encode (call before it). */
int fs2_force_buckets(fs2_engine* e, int32_t variance_index, const int32_t* idx_device);
/* Teacher forcing as the reference's non-inference forward does it (model.py:317-325,417-422): the
 * NEXT fs2_decode embeds bucketize(target*std + mean) of these (B, T) fp32 device target values for
 * variance `variance_index`; the prediction is still computed and returned.  One-shot.  Together
 * with fs2_encode's forced_durations (= targets["duration"], model.py:296-297) this is
 * FastSpeech2.forward(batch, inference=False) without the loss.  A PHONE-level variance (model.py:278-286) takes (B, L)
 * targets, consumed by the NEXT fs2_encode (call before it). */
int fs2_force_variance_targets(fs2_engine* e, int32_t variance_index, const float* target_device);
int fs2_debug_copy(fs2_engine* e, const char* what, void* dst_device, void* hip_stream);

/* Kernel timing with HIP events on the launch stream (bench.py roofline).  kernel_class: */
enum fs2_kernel_class {
    FS2_K_CONV_GEMM = 0,   /* every implicit-GEMM Conv1d launch (taps > 1) */
    FS2_K_GEMM = 1,        /* pointwise / linear GEMM launches */
    FS2_K_ATTENTION = 2,
    FS2_K_ROWOPS = 3,
    FS2_K_DEC_FFN_CONV1 = 4, /* the decoder FFN's first conv only: the single dominant launch shape */
    FS2_K_DEC_ATTENTION = 5, /* the decoder stack's self-attention launches only: the MFMA-bound attention instance (north_star) */
    FS2_K_ENC_MHA = 6,     /* the encoder stack's whole self-attention block: in-projection + attention + out-projection (+ residual +
                            * LayerNorm) launches - nn.MultiheadAttention inside ConformerEncoderLayer.forward, model.py:108-116 */
    FS2_K_PREDICTOR = 7,   /* the decode phase's single-launch VariancePredictor launches (model.py:482-522 at the frame level): the dominant
                            * kernel of the decision-safe modes, whose matrix work is three bf16 MFMAs per product (r06) */
    FS2_K_COUNT = 8
};
int fs2_profile_enable(fs2_engine* e, int32_t kernel_class, int32_t enable);
/* pre-create the event pairs of `pairs` bracketed launches (otherwise they are created on first use, inside the caller's timed region) */
int fs2_profile_reserve(fs2_engine* e, int32_t kernel_class, int32_t pairs);
/* Sums elapsed ms / launches / algorithmic flops / algorithmic bytes since enable; syncs the events. */
int fs2_profile_read(fs2_engine* e, int32_t kernel_class, double* total_ms, int64_t* launches,
                     double* flops, double* bytes);

/* ---- single-operator entry points (device pointers; used by the parity tests) ------------- */
/* Kernel-selection switches for the parity tests and A/B runs.  They are NOT process state: fs2_op_set_gemm_variant sets a switch of
 * the CALLING THREAD, read by the operator-level entry points below (fs2_op_*) that thread calls; an engine owns its own set
 * (defaults at fs2_create; fs2_set_tuning changes one; fs2_clone copies them) and never looks at a thread's.  An undefined value is
 * FS2_ERR_ARG.  Every non-default form is pinned bit-identical (or within a stated tolerance) to the default by a test.
 *   0       auto (by problem size)
 *   1       128x128 register-staged GEMM      (2, the 128x256 LDS-DMA ring GEMM, is retired: FS2_ERR_ARG; tools/probes/gemm_forms)
 *   3/4/5   slab kernel, 128/192/256-row tiles   6/7   slab kernel, 32/64-row tiles
 *   200/201/202 slab kernel tile order: plain / XCD-contiguous (default) / XCD-contiguous with column-tile PAIRS per XCD where the launch
 *           has 4, 8 or 16 column tiles and a weight panel larger than an XCD's L2 (the decoder FFN conv1: 109 MB fetched instead of 139,
 *           1 % slower - measured r05); same results
 *   220/221 bf16 pointwise launches of more tiles than CUs: one tile per workgroup / the persistent kernel (default); bit-identical
 *   230/231 wide depth-wise predictors: the last LayerNorm + Linear(filter, 1) head as a normalise pass over stored activations / from
 *           row sums the last GEMM's epilogue leaves (fs2_op_gemm_head, default); equal to fp32 rounding of another summation order
 *   240..242 slab kernel K loop, 16-bit operands stored as they came in: two weight stages, a tile requested one step before it is read /
 *           the lead-2 loop (three weight stages, the tile of step s + 2 requested at step s behind a counted wait) for the launch
 *           classes that measured faster with it (default) / wherever it exists: pointwise launches at tiles of up to 128 rows (192 with the plain epilogue), conv
 *           launches with k = 3 or 9 taps at up to 128 rows; bit-identical outputs (211, the r04 ring of whole operand stages, stays retired)
 *   500/501 fp32 slab-kernel launches: fp32 MFMA (default) / bf16 x 3 split products (what FS2_MIXED_X3 uses in its front; operator level)
 *   700/701 bf16 fs2_op_bgemm tile order: plain / XCD-contiguous (default)
 *   800/801 bf16 fs2_op_bgemm: generic instantiation only / the bounds-free one for full, aligned tiles (default)
 *   900/901 fs2_op_attention_bwd, dK / dV launch: one (default, also 909) / two 16-row blocks per wave, 905/906 three / four (one wave
 *              per SIMD; measured no faster inside the training step);  902/903/904 the dQ launch: one / two / by size (default),
 *              907/908 three / four
 *   1000/1001 bf16 fs2_op_bgemm: 256 x 256 LDS-DMA kernel for eligible TN products off / on (default)
 *   1100/1101 fs2_op_col_sum: two launches (default) / one (last workgroup reduces; measured slower)
 *   1200..1204 fused attention: 1200 = the phase-serial kernel only; 1201 / 1202 / 1204 = the software-pipelined kernel (bf16, head dim
 *              128, no attention dropout) with 32 / 64 / 96 queries per wave; 1203 = by size (default)
 *   1400..1402 bf16 GEMMs with K = 256 (no fused epilogue): slab kernel / weight-resident kernel from three row tiles per
 *              workgroup on (default) / wherever it applies; bit-identical outputs
 *   1320/1321  inference engine, bf16: the VarianceEncoder's bucketize + embedding add as the tail of its predictor's launch: off / on (default;
 *              bit-identical either way)
 *   1340/1341  inference engine, bf16, H = 256 with two heads, sequences of up to 768 rows (the encoder stack; the decoder stack for short
 *              utterances): self-attention and out-projection + residual + LayerNorm as two launches / as one (attn_out_ln_kernel, default; r06): the attention rows are the same bits, the out-projection sums its 256
 *              products in another order (equal to fp32 rounding before the bf16 store)
 *   1500/1501  fp32-storage split modes: attention on fp32 MFMA / on bf16 x 3 split products (default)
 * (Removed in r05, measured slower or neutral in r02-r04 and kept until then behind switches: 1211 resident-K/V attention, 211 operand
 *  ring, 1301 / 1302 tall / paired predictor tiles, 301 in-place wide-row LayerNorm epilogue, 311 256-row deferred epilogue.
 *  Removed in r06: 250..253, three one-wave-per-SIMD / operand-ring / producer-consumer forms of the slab GEMM that measured 5-25 % slower
 *  in r05 - their sources and measurements are kept as probes under tools/probes/gemm_forms/, outside the library.) */
int fs2_op_set_gemm_variant(int32_t variant);
/* The two vocoder knobs below are PER CALLING THREAD, like fs2_op_set_gemm_variant: fs2_voc_synthesize reads the switches of the thread
 * that calls it - a value set on the main thread does not reach a vocoder driven from a pipeline / executor worker thread (set it there).
 * tuning knob: cap (KiB) on the LDS operand slab of a vocoder conv workgroup: the conv kernel takes the tallest of its tile heights
 * (14, 8, 4, 2 sixteen-row fragments per wave) whose slab fits; the shortest is taken up to the 150 KiB a workgroup can have whatever the
 * cap says.  0 = built-in heuristic (110 KiB), 1..150 = that cap; anything else FS2_ERR_ARG (the knob is left as it was). */
int fs2_op_set_vocoder_lds_limit(int32_t kib);
/* A/B knob: which resblocks of the 32 / 64 / 128-channel stages run on LDS-resident tiles (vocoder_resblock.hip) and in which form.
 * A form is 100 * waves + sixteen-row fragments per wave: 408 = 4 waves on <= 76 KiB (two workgroups per CU), 808 / 804 = 8 waves on
 * <= 150 KiB at full / half height; a form is taken only while at least 80 % (408: 85 %) of its rows are outside the halo.
 *   0        conv by conv everywhere: no resident launch
 *   1        (default) a whole block in one launch where taps * channels <= 224, pair by pair otherwise; 408 first, then 808, then 804;
 *            between two resident launches, and behind the upsampler of a stage whose every pair is resident, the stream is stored
 *            as LeakyReLU(x)
 *   2        as 1, pairs only: never a whole block per launch
 *   4        as 1 without 408: the 8-wave forms only
 *   7        as 1 without the taps * channels <= 224 rule: a whole block per launch wherever it fits
 *   9        as 1 with every stream between launches stored raw
 *   50..100  as 1 with that percentage in place of 408's 85 (1 is the same as 85)
 * Anything else (negatives, 3, 5, 6, 8, 10..49, above 100) is FS2_ERR_ARG and leaves the knob as it was. */
int fs2_op_set_vocoder_fused_resblock(int32_t on);
/* The two choices the vocoder engine makes per layer, as pure shape functions (host only, no device needed); both read the calling
 * thread's two knobs above.  dtype: FS2_F32, FS2_BF16 or FS2_F16.
 * fs2_op_vocoder_resblock_form: the form (408 / 808 / 804, above) a whole block (npairs = 3, dilations[0..2]) or one (c1, c2) pair
 *   (npairs = 1, dilations[0]) of `channels` channels and `taps` taps runs in; 0 = not on resident tiles; negative = bad argument.
 * fs2_op_vocoder_conv_tile: the tile height (14 / 8 / 4 / 2) of the conv kernel for a layer of n output and cin input channels
 *   (shift != 0: the two tap windows of a transposed conv; post != 0: conv_post), 0 = no slab fits; *cin_pad (may be NULL) receives the
 *   padded channel stride: 32 / 64 / 128 / 256 / 512 run a compile-time-stride build, anything else the runtime-stride one. */
int32_t fs2_op_vocoder_resblock_form(int32_t dtype, int32_t channels, int32_t taps, const int32_t* dilations, int32_t npairs);
int32_t fs2_op_vocoder_conv_tile(int32_t dtype, int32_t n, int32_t cin, int32_t taps, int32_t dil, int32_t shift, int32_t post,
                                 int32_t* cin_pad);
int fs2_op_gemm(int32_t dtype, int32_t out_dtype, const void* x, const void* w, const float* bias, void* c,
                int32_t M, int32_t N, int32_t Cin, int32_t taps, int32_t S, int32_t relu, void* hip_stream);
/* c = dropout(relu(x w^T + bias)) with fs2_op_dropout's mask over the (M, N) product in the store (the FFN's hidden tensor in training
 * mode: no read-modify-write pass over the (M, filter) tensor).  FS2_ERR_SHAPE when the shape does not run on the slab kernel. */
int fs2_op_gemm_relu_dropout(int32_t dtype, const void* x, const void* w, const float* bias, void* c, int32_t M, int32_t N, int32_t Cin,
                             int32_t taps, int32_t S, float p, uint64_t seed, uint64_t key, void* hip_stream);
/* c = x w^T + bias + addend, addend (M, N) in the launch dtype; addend == c is allowed (a workgroup reads its own tile of it before it
 * writes it): the accumulating data-gradient products of the training step (dx += dy . W) without an elementwise pass behind them.
 * FS2_ERR_SHAPE when the shape does not run on the slab kernel (N < 192, M % S != 0, even tap count). */
int fs2_op_gemm_add(int32_t dtype, const void* x, const void* w, const float* bias, const void* addend, void* c, int32_t M, int32_t N,
                    int32_t Cin, int32_t taps, int32_t S, void* hip_stream);
/* c = LayerNorm(v) w0^T + bias0 evaluated on the PRE-norm rows v = x (bf16): the caller folds gamma / beta into the operands
 * (w = w0 diag(gamma) as stored in bf16, bias = bias0 + w0 beta, wg[n] = sum_k w[n][k]) and hands over v's finished row
 * statistics rowstats (M) float2 (rstd, rstd * mean) (fs2_op_rowstats_finish); the epilogue applies
 * c[m][n] = rstd[m] * acc - rstd[m] * mean[m] * wg[n] + bias[n].  What the engine's in-projection does behind a deferred norm2
 * (litfass/fastspeech2/model.py:113-115) instead of a normalise-only pass, and the mel Linear behind the last decoder block's
 * (fastspeech2.py:723; N < 192: the 128 x 128 kernel's epilogue).  bf16 only; FS2_ERR_SHAPE otherwise. */
int fs2_op_gemm_rowscale(const void* x, const void* w, const float* bias, const float* rowstats, const float* wg,
                         void* c, int32_t M, int32_t N, int32_t Cin, void* hip_stream);
/* The same with the operand type named: dtype = FS2_BF16 or FS2_F16 (x, w), out_dtype = dtype, or FS2_F32 for a narrow head (N < 192). */
int fs2_op_gemm_rowscale_dt(int32_t dtype, int32_t out_dtype, const void* x, const void* w, const float* bias, const float* rowstats,
                            const float* wg, void* c, int32_t M, int32_t N, int32_t Cin, void* hip_stream);
/* The deferred-LayerNorm epilogue by itself (N >= 192): c = v = act(x w^T + bias) [+ res] (res may be NULL) stored unnormalised, and per
 * row and 256-column tile the partial (sum v, sum v^2) -> stats (M, ceil(N / 256)) float2, the input of fs2_op_rowstats_finish.
 * dtype (x, w, res, c) = FS2_F32, FS2_BF16 or FS2_F16; a residual behind a ReLU is FS2_ERR_SHAPE. */
int fs2_op_gemm_stats(int32_t dtype, const void* x, const void* w, const float* bias, const void* res, void* c, float* stats, int32_t M,
                      int32_t N, int32_t Cin, int32_t relu, void* hip_stream);
/* parts (M, nparts) float2 partial (sum, sum of squares) over ncols columns per row - what the deferred-LayerNorm GEMM epilogue
 * leaves, one per 256-column tile - -> out (M) float2 (rstd, rstd * mean) */
int fs2_op_rowstats_finish(const float* parts, int32_t nparts, int32_t ncols, float eps, float* out, int32_t M, void* hip_stream);
/* The last layer of a wide VariancePredictor (litfass/fastspeech2/model.py:512-518,538: ... -> ReLU -> LayerNorm -> Linear(N, 1) ->
 * masked_fill) without storing its activations: v = act(x w^T + bias) (bf16 operands, fp32 v) is reduced in the GEMM epilogue to the
 * row statistics stats_out (M, ceil(N/256)) float2 (sum, sum of squares per 256-column tile) and head_out (M, ceil(N/256)) =
 * sum_n v[m][n] * head_gw[n] per tile, head_gw = gamma * w_head; fs2_op_head_finish then gives
 * pred[m] = mask[m] ? 0 : rstd * (sum of head_out[m][:] - mean * sum_gw) + cst  =  LayerNorm(v)[m] . w_head + b_head with
 * sum_gw = sum_n head_gw[n], cst = beta . w_head + b_head.  bf16, N >= 192, N % 8 == 0, Cin % 128 == 0; FS2_ERR_SHAPE otherwise. */
int fs2_op_gemm_head(const void* x, const void* w, const float* bias, const float* head_gw, float* stats_out, float* head_out, int32_t M,
                     int32_t N, int32_t Cin, int32_t relu, void* hip_stream);
int fs2_op_head_finish(const float* parts, const float* dots, int32_t nparts, int32_t ncols, float eps, float sum_gw, float cst,
                       const uint8_t* mask, float* pred, int32_t M, void* hip_stream);
/* Split-K form for long reductions over few row tiles (training step: the encoder-side data-gradient convs, M = B L rows, K = taps x
 * filter): ksplit (from fs2_op_gemm_splitk_choice; 1 = not worth it -> use fs2_op_gemm) slices of the input channels run as separate
 * workgroups of ONE launch into fp32 planes part (ksplit, M, N), a second launch adds the planes in order:
 * c (out_dtype) = [c +] sum_s part[s].  No bias / ReLU.  FS2_ERR_SHAPE when the shape does not run on the slab kernel. */
int fs2_op_gemm_splitk_choice(int32_t dtype, int32_t M, int32_t N, int32_t Cin, int32_t taps, int32_t S);
/* Which kernel a GEMM / conv request would run on under the calling thread's switches: host arithmetic, no GPU needed (the routing
 * of every fs2_op_gemm* entry and of the engine is this function's).  present: one bit per optional member of the request, from bit 0:
 * bias, res, ln_g, dot_w, z_out, ln_tmp, stats_out, epi_res, gate, drop_p > 0, rs_stats + rs_wg, head_out + head_gw, zero_rows, C_lo,
 * split, w_presplit, relu.  bias_aligned: the bias pointer is 16-byte aligned.  Returns -status where the request is refused, else
 * family | mi << 4 | flags << 8 | two_launch << 16 with family 0 nothing to do / 1 128x128 / 2 slab / 3 persistent / 4 weight-resident,
 * mi = tile rows / 32 (slab, persistent), flags bit 0-5 = the slab kernel's LN, SPLIT, DEFER, XPRE, the 128x128 kernel's zero_rows form,
 * weights packed on the fly; two_launch = a LayerNorm request served as GEMM into ln_tmp + the LayerNorm kernel. */
int32_t fs2_op_gemm_route(int32_t dtype, int32_t out_dtype, int32_t M, int32_t N, int32_t Cin, int32_t taps, int32_t S, int32_t ksplit,
                          uint32_t present, int32_t bias_aligned);
/* The same request's K loop on the slab kernel: 0 = two weight stages (also: another family), 1 / 2 = the lead-2 loop's pointwise / conv
 * form (switches 240..242); -status where the request is refused. */
int32_t fs2_op_gemm_route_lead(int32_t dtype, int32_t out_dtype, int32_t M, int32_t N, int32_t Cin, int32_t taps, int32_t S, int32_t ksplit,
                               uint32_t present, int32_t bias_aligned);
int fs2_op_gemm_splitk(int32_t dtype, int32_t out_dtype, const void* x, const void* w, void* c, float* part, int32_t M, int32_t N,
                       int32_t Cin, int32_t taps, int32_t S, int32_t ksplit, int32_t accumulate, void* hip_stream);
/* ... with the ReLU (and dropout) backward of a data-gradient product folded into the store: c = gate > 0 ? scale * (x w^T + bias)
 * : 0, gate (M, N) in the launch dtype (training step: dh = (dc2 . W2) o [h > 0] / (1 - p), h = dropout(relu(.)) of the forward:
 * h > 0 <=> kept and pre-activation > 0, model.py:84-90 backwards).  FS2_ERR_SHAPE when the shape does not run on the slab kernel
 * (N < 192, M % S != 0, even tap count): the caller then uses fs2_op_gemm + fs2_op_dropout + fs2_op_ew(op 1). */
int fs2_op_gemm_gated(int32_t dtype, const void* x, const void* w, const float* bias, const void* gate, float scale, void* c,
                      int32_t M, int32_t N, int32_t Cin, int32_t taps, int32_t S, void* hip_stream);
int fs2_op_attention(int32_t dtype, const void* qkv, const uint8_t* key_pad_mask, void* out, void* vt_scratch,
                     uint64_t* bits_scratch, int32_t B, int32_t S, int32_t H, int32_t heads, void* hip_stream);
/* The same attention (nn.MultiheadAttention inside ConformerEncoderLayer.forward, litfass/fastspeech2/model.py:108-116) in the
 * split arithmetic of the fp32x3 / mixed3 modes: qkv fp32 (B*S, 3H) is split into bf16 heads and tails (split_scratch: 2 x B*S*3H
 * bf16), every q.k and p.v product is three bf16 MFMAs (lo*hi + hi*lo + hi*hi, fp32 accumulate), softmax fp32; out fp32 (B*S, H). */
int fs2_op_attention_x3(const float* qkv, const uint8_t* key_pad_mask, float* out, void* split_scratch, uint64_t* bits_scratch,
                        int32_t B, int32_t S, int32_t H, int32_t heads, void* hip_stream);
/* fp32 GEMM c = x w^T + bias (split != 0: bf16 x 3 split products) whose result leaves as TWO bf16 (M, N) tensors, c_hi + c_lo = c
 * up to 2^-17 |c| - how the engine's in-projection feeds the split-arithmetic attention without an extra pass.  N >= 192. */
int fs2_op_gemm_split_out(const void* x, const void* w, const float* bias, void* c_hi, void* c_lo, int32_t M, int32_t N, int32_t Cin,
                          int32_t split, void* hip_stream);
/* GEMM/conv with the fused row epilogue  y = LayerNorm(act(xW^T + b) [+ res]) [, pred = head(y)]
 * (y or pred may be NULL; tmp = (M, N) scratch used when the shape cannot be fused) */
int fs2_op_gemm_ln(int32_t dtype, const void* x, const void* w, const float* bias, const void* res,
                   const float* ln_g, const float* ln_b, const float* dot_w, float dot_b, const uint8_t* mask,
                   float* pred, void* y, void* tmp, int32_t M, int32_t N, int32_t Cin, int32_t taps, int32_t S,
                   int32_t relu, void* hip_stream);
/* The same fused launch for the training tape: y = LayerNorm(z) * g + b with z = act(x W^T + bias) [+ res], and z itself stored
 * too (z_out, (M, N), the activation dtype) - what LayerNorm's backward needs (the forward of ConformerEncoderLayer's
 * x = norm(x + sublayer(x)), model.py:114-115, and of a predictor layer's conv -> ReLU -> LayerNorm, model.py:528-538, without a
 * stand-alone LayerNorm launch).  FS2_ERR_SHAPE (nothing launched) where the epilogue does not apply (N > 256, shapes the slab
 * kernel does not take): the caller keeps its GEMM + LayerNorm launches. */
int fs2_op_gemm_ln_tape(int32_t dtype, const void* x, const void* w, const float* bias, const void* res, const float* ln_g,
                        const float* ln_b, void* y, void* z_out, int32_t M, int32_t N, int32_t Cin, int32_t taps, int32_t S,
                        int32_t relu, void* hip_stream);
/* ... with nn.Dropout between the product and the residual add (the residual sites of ConformerEncoderLayer in training mode, model.py:
 * 117-121): z = dropout(act(x w^T + bias)) + res, y = LayerNorm(z); the mask is fs2_op_dropout's over the (M, N) product with this
 * (p, seed, key), so fs2_op_dropout on the gradient regenerates it. */
int fs2_op_gemm_ln_tape_dropout(int32_t dtype, const void* x, const void* w, const float* bias, const void* res, const float* ln_g,
                                const float* ln_b, void* y, void* z_out, int32_t M, int32_t N, int32_t Cin, int32_t taps, int32_t S,
                                int32_t relu, float p, uint64_t seed, uint64_t key, void* hip_stream);
size_t fs2_op_attention_scratch_bytes(int32_t dtype, int32_t B, int32_t S, int32_t H, int32_t heads, size_t* bits_bytes);
int fs2_op_layernorm(int32_t dtype, const void* x, const void* res, const float* gamma, const float* beta, void* y,
                     const float* dot_w, float dot_b, const uint8_t* mask, float* pred, int32_t M, int32_t H,
                     void* hip_stream);
int fs2_op_dwconv(int32_t dtype, const void* x, const float* w, const float* bias, void* y, int32_t B, int32_t S,
                  int32_t C, int32_t k, void* hip_stream);
int fs2_op_durations(const float* dur_pred, const uint8_t* src_mask, const int32_t* forced, int32_t* dur,
                     int32_t* cum, int32_t* totals, int32_t* guard, int32_t B, int32_t L, void* hip_stream);
int fs2_op_regulate(int32_t dtype, const void* x, const int32_t* cum, const int32_t* totals, void* y,
                    uint8_t* tgt_mask, int32_t B, int32_t L, int32_t T, int32_t H, void* hip_stream);
int fs2_op_bucket_embed(int32_t dtype, const void* x, const float* pred, const float* bins, const float* emb,
                        int32_t nbins, float std, float mean, const float* pe, const float* spk, void* y,
                        int32_t* idx_out, int32_t B, int32_t T, int32_t H, void* hip_stream);
int fs2_op_embed(int32_t dtype, const int64_t* phones, const float* table, const float* pe, const float* spk,
                 void* x, uint8_t* src_mask, int32_t B, int32_t L, int32_t H, int32_t n_phones, void* hip_stream);
int fs2_op_spk_proj(const float* dvec, const float* w, const float* b, float* spk, int32_t B, int32_t H,
                    int32_t Din, void* hip_stream);
/* The encoder-side fused launch (r06; nn.MultiheadAttention's core + out_proj + the residual + norm1 of ConformerEncoderLayer.forward,
 * model.py:108-116, behind the in-projection GEMM): out = LayerNorm(res + softmax(q k^T / sqrt(d) + key padding) v w_out^T + bias), bf16
 * or f16 (dtype names the type of qkv, w_out, res and out), H = 256, two heads.  qkv (B*S, 3H), key_pad_mask (B, S) 1 = pad, w_out (H, H), res / out (B*S, H) in that dtype (out may alias res),
 * scratch = H * H * 2 + B * ceil(S / 64) * 8 bytes.  FS2_ERR_SHAPE for other shapes / dtypes. */
int fs2_op_attn_out_ln(int32_t dtype, const void* qkv, const uint8_t* key_pad_mask, const void* w_out, const float* bias, const void* res,
                       const float* ln_g, const float* ln_b, void* out, void* scratch, int32_t B, int32_t S, int32_t H, int32_t heads,
                       void* hip_stream);
/* VariancePredictor (model.py:482-522), dense k=3, H=256, bf16, one launch: w = (nlayers, H, taps*H)
 * tap-major rows, bias / ln_g / ln_b = (nlayers, H) fp32, packed_scratch = nlayers * H * taps * H * 2
 * bytes (fragment-ordered copy of w, built by this call).  FS2_ERR_SHAPE if the shape is not covered. */
int fs2_op_predictor(int32_t dtype, const void* x, const void* w, const float* bias, const float* ln_g,
                     const float* ln_b, const float* head_w, float head_b, const uint8_t* mask, float* pred,
                     void* packed_scratch, int32_t B, int32_t S, int32_t H, int32_t nlayers, int32_t taps,
                     void* hip_stream);
/* The same for DEPTH-WISE layers (VarianceConvolutionLayer with depthwise=True, model.py:541-558: Conv1d(H, H, 3, groups = H) ->
 * Conv1d(H, H, 1) -> ReLU -> LayerNorm), H = 256, bf16, one launch: dw_w = (nlayers, 3, H) fp32 tap-major depth-wise taps, dw_b =
 * (nlayers, H), w = (nlayers, H, H) bf16 pointwise weights, bias their bias; packed_scratch = nlayers * H * H * 2 bytes. */
int fs2_op_predictor_dw(int32_t dtype, const void* x, const float* dw_w, const float* dw_b, const void* w, const float* bias,
                        const float* ln_g, const float* ln_b, const float* head_w, float head_b, const uint8_t* mask, float* pred,
                        void* packed_scratch, int32_t B, int32_t S, int32_t H, int32_t nlayers, void* hip_stream);
/* FastSpeech2Loss.get_loss for "l1" / "mse" (litfass/fastspeech2/loss.py:57-81, called from forward :83-213):
 * out2[0] = mean over the rows whose pad_mask is 0 of |pred - truth| (kind 0) or (pred - truth)^2 (kind 1),
 * out2[1] = number of selected elements; pred = (rows, inner) fp32; truth_kind 0: fp32 (rows, inner),
 * 1: int64 target durations compared as log(d + 1) (loss.py:176); ws = fs2_op_masked_loss_ws_bytes() device
 * bytes, zero-filled once by the caller and reusable across calls on one stream.  Deterministic (fp64
 * partials added in a fixed order, no float atomics).  All device pointers. */
size_t fs2_op_masked_loss_ws_bytes(void);
int fs2_op_masked_loss(const float* pred, const void* truth, int32_t truth_kind, const uint8_t* pad_mask, int64_t rows,
                       int32_t inner, int32_t kind, void* ws, float* out2, void* hip_stream);
/* Soft-DTW value of B sequence pairs (litfass/third_party/softdtw/__init__.py:8-24,110-117 = the validation metric of
 * fastspeech2.py:1149-1156; the same recursion is the arithmetic of the "soft_dtw" loss kind, loss.py:57-81):
 * out[b] = R[N, M] with D[i,j] = |x[b,i] - y[b,j]|^2 (fp32), the recursion in fp64.  x (B, N, D), y (B, M, D), out (B): fp32
 * device pointers.  One workgroup per pair; the sequences are staged in LDS when both fit beside the three fp64
 * anti-diagonals (e.g. 2 x 240 frames of an 80-bin mel), else read through the caches; FS2_ERR_SHAPE for N > 6800. */
int fs2_op_soft_dtw(const float* x, const float* y, int32_t B, int32_t N, int32_t M, int32_t D, float gamma, float* out,
                    void* hip_stream);
/* The same value plus its gradient with respect to x - what loss.backward() yields through the reference's vendored module
 * (third_party/softdtw/__init__.py:27-52 compute_softdtw_backward on the float32 R / D that _SoftDTW.forward saves, :56-77;
 * autograd through calc_distance_matrix :85-92): grad_x[b,i,:] = 2 sum_j E[b,i,j] (x[b,i,:] - y[b,j,:]).  The "soft_dtw" loss
 * kind of loss.py:36,62-81 differentiates exactly this, chunk by chunk, with respect to the prediction only.  scratch: device
 * memory of fs2_op_soft_dtw_grad_scratch_bytes(B, N, M) bytes (R, D and E of every pair).  Deterministic. */
size_t fs2_op_soft_dtw_grad_scratch_bytes(int32_t B, int32_t N, int32_t M);
int fs2_op_soft_dtw_grad(const float* x, const float* y, int32_t B, int32_t N, int32_t M, int32_t D, float gamma, float* out,
                         float* grad_x, void* scratch, size_t scratch_bytes, void* hip_stream);
/* dtype conversion helpers for tests: fp32 <-> engine dtype (FS2_BF16 or FS2_F16; fp32 -> FS2_F16 saturates, see fs2_dtype), n elements,
 * device pointers */
int fs2_op_convert(int32_t src_dtype, int32_t dst_dtype, const void* src, void* dst, size_t n, void* hip_stream);
/* The same fp32 -> FS2_F16 conversion on the HOST (host pointers, no device needed): the routine fs2_finalize converts the decoder's
 * weights with in FS2_MIXED_F16_X3, bit for bit what a device store gives - clamp to +-65504, round to nearest-even, NaN kept.  For
 * callers that prepare FS2_F16 operands of the fs2_op_* entry points themselves. */
int fs2_host_f32_to_f16(const float* src, uint16_t* dst, size_t n);

/* ================================================================================================
 * Training step: the operators the reference gets from autograd in
 * FastSpeech2.training_step (litfass/fastspeech2/fastspeech2.py:786-797: loss.backward()) and from
 * torch.optim.AdamW + gradient_clip_val (fastspeech2.py:1166-1182, scripts/train.sh:16).  The tape itself
 * (which tensor feeds which gradient) lives in the host mirror, lightningfastspeech2_amd/training.py.
 * All device pointers; fp32 (FS2_F32) arithmetic on the exact fp32 MFMA.
 * ================================================================================================ */
/* C[b1][b2](m, n) = alpha * sum_k A(m, k) B(k, n) + bias[n] + beta * C, operands by element strides (one stride of each
 * operand is 1), two batch levels, optional deterministic split-K, and the two implicit 'same'-padded Conv1d forms over
 * (B*S, C) time-major rows with utterances of `seg` rows:
 *   data gradient (taps > 1):  K = taps * Kin; the k-tiles of tap j read A rows m + a_shift0 + j * a_shift_step
 *                              (zero outside the row's utterance) and B from + j * sBtap;
 *   weight gradient (taps <= 1, seg > 0): batch index b2 reads B's k rows at k + b_shift0 + b2 * b_shift_step. */
typedef struct fs2_bgemm_desc {
    int32_t M, N, K;
    int64_t sAm, sAk, sBk, sBn, ldc;
    int32_t nb1, nb2;
    int64_t sA1, sA2, sB1, sB2, sC1, sC2;
    float alpha, beta;
    int32_t splitk;
    int32_t seg, taps, Kin, a_shift0, a_shift_step;
    int64_t sBtap;
    int32_t b_shift0, b_shift_step;
    int32_t c_dtype;   /* fs2_dtype of C: FS2_F32 operands write fp32; FS2_BF16 operands write bf16 or fp32 */
} fs2_bgemm_desc;
size_t fs2_op_bgemm_ws_bytes(const fs2_bgemm_desc* d);  /* split-K slabs (0 when splitk <= 1) */
/* 1 when bf16 operands of this shape run on the 256 x 256 tile kernel (TN product, M % 256 == N % 256 == K % 32 == 0, fp32 C):
 * the caller sizes splitk for 4x fewer, 512-thread workgroups (one per CU) then */
int32_t fs2_op_bgemm_tn256(const fs2_bgemm_desc* d);
int fs2_op_bgemm(int32_t dtype, const fs2_bgemm_desc* d, const void* A, const void* B, void* C, const float* bias,
                 float* ws, void* hip_stream);
/* The fused (flash) attention of the inference path on the training path: also writes lse2 (B, heads, S) - per query, log2 of
 * the softmax denominator in the scaled scores' log2 units - and applies nn.MultiheadAttention's attention-weight dropout
 * (drop_p = 0: none; mask regenerated from (seed, key) over the (b, head, query, key) index); and its recomputing backward
 * (bf16, head dim 128: fs2_op_attention_bwd_supported): dqkv (B*S, 3H) from dout (B*S, H), qkv, lse2 and
 * delta = fs2_op_attn_delta(dout, out); neither the probabilities nor their gradients reach HBM.  Two launches, no atomics. */
int fs2_op_attention_train(int32_t dtype, const void* qkv, const uint8_t* key_pad_mask, void* out, void* vt_scratch,
                           uint64_t* bits_scratch, float* lse2, int32_t B, int32_t S, int32_t H, int32_t heads, float drop_p,
                           uint64_t drop_seed, uint64_t drop_key, void* hip_stream);
int32_t fs2_op_attention_bwd_supported(int32_t dtype, int32_t H, int32_t heads);
int fs2_op_attention_bwd(int32_t dtype, const void* qkv, const void* dout, const float* lse2, const float* delta,
                         const uint8_t* key_pad_mask, void* dqkv, int32_t B, int32_t S, int32_t H, int32_t heads, float drop_p,
                         uint64_t drop_seed, uint64_t drop_key, void* hip_stream);
/* attention backward without a dP tensor: C = dS = alpha * P o (dropout(A B) - delta) where A B = dO V^T is the product the
 * descriptor states, P (C's layout and dtype) are the forward's probabilities, delta (nb1, nb2, M) = fs2_op_attn_delta(dO, O)
 * (= sum_k dP P) and the dropout is the forward's attention-weight dropout (drop_p = 0: none), regenerated from (seed, key) */
int fs2_op_bgemm_softmax_bwd(int32_t dtype, const fs2_bgemm_desc* d, const void* A, const void* B, void* C, const void* P,
                             const float* delta, float drop_p, uint64_t drop_seed, uint64_t drop_key, void* hip_stream);
int fs2_op_attn_delta(int32_t dtype, const void* dout, const void* out, float* delta, int32_t B, int32_t S, int32_t H,
                      int32_t heads, void* hip_stream);
/* LayerNorm backward of y = LN(z [+ res]) * gamma + beta: dz (M, H); relu_mask = 1 when z is a ReLU output and dz should be
 * the gradient of the pre-activation (dz zeroed where z <= 0).  part = (fs2_op_layernorm_bwd_parts(M), 3, H) partial column
 * sums of dy * zhat, dy and dz, to be reduced with fs2_op_col_sum over the parts -> dgamma, dbeta and the bias gradient of
 * the layer that produced z.  H % 4 == 0, H <= 1024. */
int32_t fs2_op_layernorm_bwd_parts(int32_t M);
int fs2_op_layernorm_bwd(int32_t dtype, const void* z, const void* res, const void* dy, const float* gamma, void* dz,
                         float* part, int32_t M, int32_t H, int32_t relu_mask, void* hip_stream);
/* ... whose dy is the gradient of dropout(y) (VarianceConvolutionLayer: LayerNorm -> Dropout, model.py:538-539,556-557): the
 * forward's mask (fs2_op_dropout / fs2_op_layernorm_dropout with the same seed, key) is applied to dy on load */
int fs2_op_layernorm_bwd_dropout(int32_t dtype, const void* z, const void* res, const void* dy, const float* gamma, void* dz,
                                 float* part, int32_t M, int32_t H, int32_t relu_mask, float drop_p, uint64_t seed, uint64_t key,
                                 void* hip_stream);
/* ... for y = LayerNorm(res + dropout(u)) (the residual sites): dz as above (the residual's gradient) AND dzm = mask o dz / (1 - out_p),
 * the gradient of u, as a second tensor (mask of fs2_op_dropout(., out_p, seed, out_key) over (M, H)); the third column sum of part is
 * then dzm's (u's bias gradient). */
int fs2_op_layernorm_bwd_masked(int32_t dtype, const void* z, const void* res, const void* dy, const float* gamma, void* dz, void* dzm,
                                float* part, int32_t M, int32_t H, int32_t relu_mask, float out_p, uint64_t seed, uint64_t out_key,
                                void* hip_stream);
/* fs2_op_layernorm with its fused Linear(H, 1) head reading the bias from DEVICE memory (a parameter being trained: the host
 * copy would cost a read-back + stream sync per step) */
int fs2_op_layernorm_head(int32_t dtype, const void* x, const void* res, const float* gamma, const float* beta, void* y,
                          const float* dot_w, const float* dot_b_dev, const uint8_t* mask, float* pred, int32_t M, int32_t H,
                          void* hip_stream);
/* y = dropout(LayerNorm(x [+ res])) in one launch; the mask is fs2_op_dropout's over the (M, H) element index */
int fs2_op_layernorm_dropout(int32_t dtype, const void* x, const void* res, const float* gamma, const float* beta, void* y,
                             int32_t M, int32_t H, float drop_p, uint64_t seed, uint64_t key, void* hip_stream);
/* out[s][n] (+)= scale * sum over the rows of segment s of x[row][n]; seg = rows per segment (0: one segment).  Per-chunk
 * partials in ws (fs2_op_col_sum_ws_bytes), added in chunk order (deterministic).  ws starts with 8192 32-bit counters for the
 * one-launch variant (fs2_op_set_gemm_variant 1101; off by default, measured slower): the caller zeroes them ONCE, when it
 * allocates ws; every launch leaves them zero again.
 * fs2_op_col_sum2: one segment, columns [0, n1) to out and [n1, N) to out2, each with its own accumulate flag. */
size_t fs2_op_col_sum_ws_bytes(int32_t M, int32_t N, int32_t seg);
int fs2_op_col_sum(int32_t dtype, const void* x, float* out, float* ws, int32_t M, int32_t N, int32_t ldx, int32_t seg,
                   int32_t accumulate, float scale, void* hip_stream);
int fs2_op_col_sum2(int32_t dtype, const void* x, float* out, float* out2, int32_t n1, float* ws, int32_t M, int32_t N,
                    int32_t ldx, int32_t accumulate, int32_t accumulate2, float scale, void* hip_stream);
/* out[n] (+)= scale * sum_r row_w[r] * x[r][n]: the weight gradient of a Linear(H, 1) head (row_w = the loss gradient per row) */
int fs2_op_col_sum_weighted(int32_t dtype, const void* x, const float* row_w, float* out, float* ws, int32_t M, int32_t N,
                            int32_t ldx, int32_t accumulate, float scale, void* hip_stream);
/* masked softmax over the key axis of (B, heads, S, S) fp32 scores -> probabilities p in the activation dtype (the training
 * path materialises them; p may alias s for FS2_F32), and its backward ds = scale * P o (dP - sum_k dP o P) from fp32 dP */
int fs2_op_softmax_fwd(int32_t dtype, const float* s, const uint8_t* key_pad, void* p, int32_t B, int32_t heads, int32_t S,
                       float scale, void* hip_stream);
int fs2_op_softmax_bwd(int32_t dtype, const float* dp, const void* p, void* ds, int32_t B, int32_t heads, int32_t S,
                       float scale, void* hip_stream);
/* elementwise over the activation dtype: op 0: out = alpha*a + beta*b (b may be NULL)   1: out = a where b > 0 else 0
 * (ReLU backward)   2: out = alpha*a */
int fs2_op_ew(int32_t dtype, int32_t op, const void* a, const void* b, void* out, size_t n, float alpha, float beta,
              void* hip_stream);
/* embedding backward: table[idx[r]] += x[r] for r < R (int32 or int64 indices), row skip_row untouched (padding_idx).
 * ws: fs2_op_scatter_rows_ws_bytes(R, H, V) bytes when that is non-zero (long index lists over tables of <= 256 rows take a
 * chunked two-phase form; ws follows fs2_op_col_sum's zero-once rule), else NULL; NULL always selects the one-launch kernel.
 * Either form is deterministic. */
size_t fs2_op_scatter_rows_ws_bytes(int32_t R, int32_t H, int32_t V);
int fs2_op_scatter_rows(int32_t dtype, const void* x, const int32_t* idx32, const int64_t* idx64, float* table, float* ws,
                        int32_t R, int32_t H, int32_t V, int32_t skip_row, void* hip_stream);
/* LengthRegulator backward: dx[b][p] = sum of dy[b][t] over the frames phone p was repeated to (truncated at T) */
int fs2_op_regulate_bwd(int32_t dtype, const void* dy, const int32_t* cum, void* dx, int32_t B, int32_t L, int32_t T,
                        int32_t H, void* hip_stream);
/* gradient of alpha * fs2_op_masked_loss(...) with respect to pred; stat = that call's out2 (the count is read on device) */
int fs2_op_masked_loss_bwd(const float* pred, const void* truth, int32_t truth_kind, const uint8_t* pad_mask,
                           const float* stat, float* dpred, int64_t rows, int32_t inner, int32_t kind, float alpha,
                           void* hip_stream);
/* PriorEmbedding (model.py:146-164) on the training path: y[b, t] = x[b, t] + emb[bucketize(values[b], bins)] for every row of
 * utterance b; emb is the caller's relu(embedding.weight) (relu(E[i]) == relu(E)[i]); idx_out (B*T) receives the bucket per row */
int fs2_op_bucket_embed_utt(int32_t dtype, const void* x, const float* values, const float* bins, const float* emb, int32_t nbins,
                            void* y, int32_t* idx_out, int32_t B, int32_t T, int32_t H, void* hip_stream);
/* nn.Dropout in training mode: y = x * keep / (1 - p) (y may alias x).  The mask is a counter-based hash of (seed, key, element
 * index) - nothing is stored; the backward applies the same call to the gradient.  Not the reference's random stream (torch's
 * Philox), the same distribution. */
int fs2_op_dropout(int32_t dtype, const void* x, void* y, size_t n, float p, uint64_t seed, uint64_t key, void* hip_stream);
/* pred[m] = mask[m] ? 0 : y[m] . w + b[0]: the VariancePredictor head (model.py:512-518) when a dropout layer sits between the
 * last LayerNorm and the Linear (otherwise fs2_op_layernorm's fused head does it) */
int fs2_op_row_dot(int32_t dtype, const void* y, const float* w, const float* b, const uint8_t* mask, float* pred, int64_t M,
                   int32_t H, void* hip_stream);
/* CWT head of a VariancePredictor in training (model.py:413-415, 505-520), one pass over out_conv (B*S, F) in `dtype`
 * (FS2_F32 / FS2_BF16; F a multiple of 64, 64..1024; anything else is FS2_ERR_ARG):
 *   spec_out (B*S, 10) = mask ? 0 : out_conv w10^T + b10;  ybar_out (B, F) = mean over ALL S rows of an utterance (pads included);
 *   mean_std_out (B, 2) = ybar ms_w^T + ms_b.
 * Column sums by per-workgroup partials in ws (fs2_op_cwt_head_train_ws_bytes), added in a fixed order; fp32 accumulation. */
size_t fs2_op_cwt_head_train_ws_bytes(int32_t B, int32_t S, int32_t F);
int fs2_op_cwt_head_train(int32_t dtype, const void* out_conv, const float* w10, const float* b10, const float* ms_w, const float* ms_b,
                          const uint8_t* mask, float* spec_out, float* ybar_out, float* mean_std_out, float* ws, int32_t B, int32_t S,
                          int32_t F, void* hip_stream);
/* ... and its backward, one pass again: dy (B*S, F) in `dtype` = dspec w10 + (1 / S) dms[b] ms_w (pad rows, whose dspec is 0, get the
 * second term too);  g_w10 (10, F) += dspec^T out_conv,  g_b10 (10) += column sums of dspec  (per-workgroup partials in ws, added
 * in workgroup order);  g_ms_w (2, F) += dms^T ybar,  g_ms_b (2) += column sums of dms.  Same inputs, same bits.
 * ws: fs2_op_cwt_head_bwd_ws_bytes, zero before its first use (it starts with a fs2_op_col_sum workspace, whose counters so keep one address for every shape). */
size_t fs2_op_cwt_head_bwd_ws_bytes(int32_t B, int32_t S, int32_t F);
int fs2_op_cwt_head_bwd(int32_t dtype, const void* out_conv, const float* dspec, const float* dms, const float* ybar, const float* w10,
                        const float* ms_w, void* dy, float* g_w10, float* g_b10, float* g_ms_w, float* g_ms_b, float* ws, int32_t B,
                        int32_t S, int32_t F, void* hip_stream);
/* depth-wise Conv1d (model.py:75-81, 545-551) backward: data gradient = the same conv with the taps reversed and no bias;
 * weight / bias gradient as per-chunk partials part (fs2_op_dwconv_wgrad_parts(B, S), C * (k + 1)): [c * k + j] then [C * k + c],
 * reduced with fs2_op_col_sum into the adjacent (C, k) weight and (C) bias gradients */
int fs2_op_dwconv_dgrad(int32_t dtype, const void* dy, const float* w, void* dx, int32_t B, int32_t S, int32_t C, int32_t k,
                        void* hip_stream);
int32_t fs2_op_dwconv_wgrad_parts(int32_t B, int32_t S);
int fs2_op_dwconv_wgrad(int32_t dtype, const void* dy, const void* x, float* part, int32_t B, int32_t S, int32_t C, int32_t k,
                        void* hip_stream);
/* the depth-wise layer's conv2 = Sequential(grouped 1x1 conv, groups = H over F channels; pointwise F -> H) (model.py:84-93)
 * as one linear map Wf (H, F) = W21 blockdiag(G), bf = b21 + W21 bg (what the inference engine folds once at load time), and
 * the chain rule from (dWf, dbf) back to the four parameter gradients (accumulated) */
int fs2_op_fold_conv2(int32_t wf_dtype, const float* G, const float* bg, const float* W21, const float* b21, void* Wf, float* bf,
                      int32_t H, int32_t F, void* hip_stream);
int fs2_op_unfold_conv2(const float* dWf, const float* dbf, const float* G, const float* bg, const float* W21, float* dG,
                        float* dbg, float* dW21, float* db21, int32_t H, int32_t F, void* hip_stream);
/* the data-gradient kernel of a Conv1d / Linear: dst (Cin, taps*N), dst[ci][j'*N + n] = src[n][(taps-1-j')*Cin + ci] for
 * src (N, taps*Cin) tap-major, so that dX = fs2_op_gemm(x = dY, w = dst, M, N = Cin, Cin = N, taps, S) */
int fs2_op_transpose_weight(int32_t dtype, const void* src, void* dst, int32_t N, int32_t Cin, int32_t taps, void* hip_stream);
/* ... for many bf16 weights in one launch: table_dev = n rows of 6 int64 ON THE DEVICE, {src, dst, N, Cin, taps, first tile},
 * a weight owning fs2_op_transpose_weight_tiles(N, Cin, taps) consecutive tiles from its first tile; tiles = their total */
int64_t fs2_op_transpose_weight_tiles(int32_t N, int32_t Cin, int32_t taps);
int fs2_op_transpose_weight_batch(const int64_t* table_dev, int32_t n, int64_t tiles, void* hip_stream);
/* out[0] = sum of squares of x (fp64 partials, fixed order) */
size_t fs2_op_sum_sq_ws_bytes(size_t n);
int fs2_op_sum_sq(const float* x, size_t n, float* ws, float* out, void* hip_stream);
/* torch.optim.AdamW step over flat fp32 buffers; g is scaled by grad_scale and, when gnorm_sq (device scalar, sum of
 * squares of g) is given, by the clip_grad_norm_ coefficient min(1, max_norm / (grad_scale * sqrt(gnorm_sq) + 1e-6)) */
int fs2_op_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int32_t step, const float* gnorm_sq, float max_norm, float grad_scale,
                 void* hip_stream);
/* ... that also writes the updated weights rounded to bf16 (shadow_bf16, n elements: the mixed-precision path's operands) */
int fs2_op_adamw_shadow(float* p, const float* g, float* m, float* v, void* shadow_bf16, size_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int32_t step, const float* gnorm_sq, float max_norm,
                        float grad_scale, void* hip_stream);
/* teacher-forced VarianceEncoder embedding (model.py:417-422): y = x + Emb[bucketize(target * std + mean)] (+ pe + spk) */
int fs2_op_bucket_embed_target(int32_t dtype, const void* x, const float* target, const float* bins, const float* emb,
                               int32_t nbins, float std, float mean, const float* pe, const float* spk, void* y,
                               int32_t* idx_out, int32_t B, int32_t T, int32_t H, void* hip_stream);
/* the CWT pitch head on its own (VarianceEncoder.forward's CWT branch behind the predictor, model.py:412-431 + cwt.py:18-21,49-50; for
 * the operator tests): out_conv (B*T, F) rows of the last predictor layer in `dtype`, spec (B*T, ld_spec >= 10) fp32 head rows whose
 * first 10 columns are the scales, mask (B*T) 1 = pad or null -> mean_std (B, 2), pred (B, T), spec_out (B, T, 10) or null */
int fs2_op_cwt_head(int32_t dtype, const void* out_conv, const float* spec, int32_t ld_spec, const uint8_t* mask,
                    const float* ms_w, const float* ms_b, float* mean_std, float* pred, float* spec_out, int32_t B, int32_t T,
                    int32_t F, void* hip_stream);
/* Waveform finishing behind the generator, one launch (what Synthesiser.__call__ and int16_samples_to_float32 do on the host,
 * third_party/hifigan/__init__.py:39-43, synthesis/generator.py:24-33): wav (B, T * hop) fp32 device, lengths (B) int32 device frame
 * counts (clamped to [0, T]; never read by the host) or NULL for full rows.  offsets (B + 1) int64 device, written here:
 * offsets[b] = hop * sum(lengths[< b]), offsets[B] = the packed total.  Utterance b's first lengths[b] * hop samples land contiguously
 * at out + offsets[b]; pads are neither read nor written, out beyond offsets[B] is left alone.  kind FS2_WAV_I16: out is int16,
 * q = (int16)(int32)trunc(x * 32768.0f) - toward zero, low 16 bits kept, so +1.0f gives -32768 as numpy's cast does on the host;
 * FS2_WAV_F32: out is float32, (float)q / 32767.0f, IEEE division.  out_capacity (elements) < B * T * hop is FS2_ERR_ARG: the packed
 * total is not known to the host at launch time.  Any hop; 16 B accesses where an utterance's rows are 16 B aligned. */
#define FS2_WAV_I16 0
#define FS2_WAV_F32 1
int fs2_op_wav_pack(const float* wav, const int32_t* lengths, int32_t B, int32_t T, int32_t hop, int32_t kind, void* out,
                    int64_t out_capacity, int64_t* offsets, void* hip_stream);

/* ================================================================================================
 * Waveform augmentation on the packed buffer (csrc/augment.hip, DESIGN.md "Augmentation"): what the reference's SpeechGenerator does
 * on the host per utterance behind the vocoder (generate.py:82-104 RoomSimulator + AddGaussianSNR, generator.py:181,197-201 resample),
 * restated from the definitions below - no library is pinned.  Stateless entry points on the layout fs2_op_wav_pack writes: `in`
 * (packed) float32 holds utterance b's n_b = offsets[b + 1] - offsets[b] samples contiguously, offsets (B + 1) int64 ON THE DEVICE.
 * The host knows capacities only: max_len is a host upper bound on every n_b and sizes the grids (an n_b beyond it is clamped to
 * it; a negative one counts as 0).  Where lengths change the entry point writes out_offsets (B + 1) itself.  Samples outside an
 * utterance's [0, n_b) count as zero: they are never read from a neighbour and nothing at or past offsets[B] is read; out beyond
 * out_offsets[B] is left alone.  out_capacity (elements) below the worst case for (max_len, B, mode) is FS2_ERR_ARG.  Every argument
 * (FS2_ERR_ARG) or shape (FS2_ERR_SHAPE; also B > 65535, max_len > 2^30) error is answered before any device call.  The heavy sums
 * are exact-fp32 MFMA GEMMs whose order depends on (position in the tile, R, table shape) only: results are bitwise batch-invariant.
 * Nothing is allocated, nothing synchronises.  out must not overlap in (except fs2_op_wav_add_noise, where out == in is allowed).
 *
 * fs2_op_wav_resample, orig_freq -> new_freq (torchaudio's published sinc_interp_hann definition; not pinned against its output):
 *   orig = orig_freq / gcd, new = new_freq / gcd, lpw = 6, rolloff = 0.99, base = min(orig, new) * rolloff,
 *   width = ceil(lpw * orig / base), K = 2 * width + orig; for p < new, q < K:
 *   t = clip((-p / new + (q - width) / orig) * base, -lpw, lpw), tab[p][q] = sinc(pi t) * cos^2(pi t / (2 lpw)) * base / orig.
 *   m_b = ceil(new * n_b / orig) (int64), y[i * new + p] = sum_q tab[p][q] * x[i * orig + q - width] for i * new + p < m_b.
 *   tab: (new, K) float32 row-major ON THE DEVICE, built by the caller in float64 and rounded once (augment.resample_table).
 *   Worst case m = ceil(new * max_len / orig) per utterance.  Supported: new <= 640, K <= 1024; else FS2_ERR_SHAPE.
 * fs2_op_wav_convolve: y_b[t] = sum_{k < R} h[k] x_b[t - k], h = row rir_index[b] of the bank rir (n_rir, R_max) float32,
 *   R = rir_len[that row] (clamped to [1, R_max]); rir_len (n_rir) int32, rir_index (B) int32, all on the device.  rir_index[b] < 0
 *   (or >= n_rir) copies the utterance bit for bit, in either mode.  FS2_CONV_SAME keeps t < n_b (audiomentations'
 *   leave_length_unchanged), FS2_CONV_FULL t < n_b + R - 1 (an empty utterance stays empty).  No rescaling: the response is applied as
 *   given.  1 <= R_max <= 16384; larger is FS2_ERR_SHAPE.  Worst case per utterance: max_len (SAME), max_len + R_max - 1 (FULL).
 * fs2_op_wav_add_noise (AddGaussianSNR's rule, noise_rms = signal_rms / 10^(snr / 20)): rms_b = sqrt(sum x^2 / n_b), the sum in fp64
 *   in a fixed order; scale_b = (float)(rms_b / 10^(snr_b / 20)) evaluated in fp64 and rounded once (0 for an empty utterance);
 *   y = x + scale_b * z as one fp32 multiply and one fp32 add, uncontracted.  snr (B) float32 device, +inf = leave the utterance
 *   alone bit for bit (scale 0); z = packed float32 noise addressed by the same offsets; scales_out (B) float32 is written for the
 *   caller.  ws: fs2_op_wav_add_noise_ws_bytes(B, max_len) device bytes, 8-byte aligned (FS2_ERR_NOMEM if short).
 * fs2_op_wav_convolve_tile is DIAGNOSTIC (as fs2_mel_tile_frames): the consecutive outputs one workgroup of the convolution owns,
 *   counted from the utterance's first sample - where its tile seams lie.
 *   fs2_op_wav_resample_tile likewise: the consecutive INPUT samples (a multiple of 32 * orig) one workgroup of the resampler owns for
 *   this table shape, 0 for a shape fs2_op_wav_resample refuses.
 * ================================================================================================ */
#define FS2_CONV_SAME 0
#define FS2_CONV_FULL 1
int fs2_op_wav_resample(const float* in, const int64_t* in_offsets, int32_t B, int64_t max_len, const float* tab, int32_t orig,
                        int32_t new_rate, int32_t width, float* out, int64_t out_capacity, int64_t* out_offsets, void* hip_stream);
int fs2_op_wav_convolve(const float* in, const int64_t* in_offsets, int32_t B, int64_t max_len, const float* rir,
                        const int32_t* rir_len, const int32_t* rir_index, int32_t n_rir, int32_t R_max, int32_t mode, float* out,
                        int64_t out_capacity, int64_t* out_offsets, void* hip_stream);
size_t fs2_op_wav_add_noise_ws_bytes(int32_t B, int64_t max_len);
int fs2_op_wav_add_noise(const float* in, const int64_t* offsets, int32_t B, int64_t max_len, const float* z, const float* snr,
                         void* ws, size_t ws_bytes, float* out, float* scales_out, void* hip_stream);
int32_t fs2_op_wav_convolve_tile(void);
int32_t fs2_op_wav_resample_tile(int32_t orig, int32_t new_rate, int32_t width);

/* ================================================================================================
 * Analysis front end: waveform -> log-mel spectrogram and frame energy (csrc/analysis.hip, DESIGN.md "Analysis front end").
 * What the reference computes per item on the CPU with torchaudio and librosa (TTSDataset.__getitem__ / _create_variances,
 * litfass/dataset/datasets.py:183-199,369-380,600-618,630-648), for a padded batch, on the device.  For one utterance x of
 * n >= 1 samples, s = 1 / max|x| when peak_normalize is set and the maximum is > 0 (else 1; the reference divides unconditionally
 * and gives NaN on silence), x~ = s x:
 *   mel     T = 1 + n / hop frames; frame t = x~[t hop - n_fft / 2 + k], k < n_fft, zero outside [0, n) (the padding sits at the
 *           utterance's own ends); periodic Hann window of win_length, zero-padded symmetrically to n_fft as torch.stft does;
 *           mel_t[m] = sum_f basis[m][f] |X_t[f]|; the output is log10 or ln of max(mel, clip), or (FS2_MEL_LINEAR) mel_t itself,
 *           unclamped - the quantity an accuracy figure is taken on: a float32 logarithm rounds away what separates two DFTs
 *   energy  Te = ceil(n / hop) frames; e[t] = sqrt(sum_{j = t hop}^{min(t hop + win_length, n) - 1} x~[j]^2 / win_length)
 * Samples at or past lengths[b] are never read (they may hold NaN).  fp32 throughout: the DFT and the mel product are exact-fp32
 * MFMA GEMMs against tables built in float64 at create; sums never depend on the batch, so results are bitwise batch-invariant.
 * The configuration is passed as scalars (no struct): n_fft a power of two in [256, 2048], 1 <= win_length <= n_fft, hop dividing
 * n_fft, 1 <= n_mels <= 128, clip > 0, log_kind FS2_MEL_LOG10 / FS2_MEL_LN / FS2_MEL_LINEAR; anything else is FS2_ERR_SHAPE (geometry) or
 * FS2_ERR_ARG (abi_version, null / non-finite basis, clip, log_kind), decided before any device call.  mel_basis is HOST memory,
 * (n_mels, n_fft / 2 + 1) row-major; only the bins between its first and last non-zero column become DFT columns.  As with
 * fs2_create the handle is returned on failure too, for fs2_mel_last_error; destroy it.
 * ================================================================================================ */
#define FS2_MEL_LOG10 0
#define FS2_MEL_LN 1
#define FS2_MEL_LINEAR 2
typedef struct fs2_mel fs2_mel;
int fs2_mel_create(int32_t abi_version, int32_t n_fft, int32_t win_length, int32_t hop, int32_t n_mels, float clip, int32_t log_kind,
                   const float* mel_basis_host, fs2_mel** out);
int fs2_mel_destroy(fs2_mel* m);
const char* fs2_mel_last_error(const fs2_mel* m);
/* The next two are DIAGNOSTIC: they describe how this build runs a configuration (for tests that place lengths at the kernel's tile
 * seams and for tools/bench_analysis.py's byte counts), nothing a caller of fs2_mel_run needs.
 * frames one workgroup owns (64, or 32 / 16 where a 64-frame sample span does not fit LDS): where the kernel's tile seams lie */
int32_t fs2_mel_tile_frames(const fs2_mel* m);
/* the DFT columns kept: bins first_bin .. first_bin + n_columns - 1 (n_columns a multiple of 32, zero-weight beyond the basis' last bin) */
int fs2_mel_used_bins(const fs2_mel* m, int32_t* first_bin, int32_t* n_columns);
/* bytes of device workspace fs2_mel_run needs for a (B, S) batch (the per-utterance peaks) */
size_t fs2_mel_ws_bytes(const fs2_mel* m, int32_t B, int32_t S);
/* wav (B, S) fp32, lengths (B) int32 (clamped to [0, S]; 0 = no frames): device.  mel (B, T_max, n_mels) with T_max >= 1 + S / hop,
 * energy (B, Te_max) with Te_max >= ceil(S / hop) or NULL (Te_max is ignored then), mel_frames (B) int32, energy_frames (B) int32 or
 * NULL: device, all written in full - rows at or past an utterance's own count are zeros.  ws: fs2_mel_ws_bytes(m, B, S) device bytes
 * (required in every mode).  Enqueues a memset and up to three launches on the caller's stream; allocates nothing, never synchronises.
 * Every argument error (FS2_ERR_ARG; FS2_ERR_NOMEM for a short workspace; FS2_ERR_STATE for a handle whose create failed) is
 * answered before the first launch. */
int fs2_mel_run(fs2_mel* m, const float* wav, const int32_t* lengths, int32_t B, int32_t S, int32_t peak_normalize, float* mel,
                int32_t T_max, float* energy, int32_t Te_max, int32_t* mel_frames, int32_t* energy_frames, void* ws, size_t ws_bytes,
                void* hip_stream);
/* Phone-level reduction of a frame-level variance (datasets.py:631-648): values (B, T) fp32, frames (B) int32 valid frames per row or
 * NULL (= T), durations (B, L) int32 -> out (B, L): with pos_j = sum of the durations before j and the segment [pos_j, pos_j + d_j)
 * clipped to the row's frames, out[j] = (mean of the segment - mean) / std, and (empty_value - mean) / std for an empty segment (the
 * reference's 1e-7).  The segment is summed in order in fp32.  std must be finite and non-zero (1 and mean 0: no normalisation). */
int fs2_op_segment_mean(const float* values, const int32_t* frames, const int32_t* durations, int32_t B, int32_t T, int32_t L,
                        float empty_value, float mean, float std, float* out, void* hip_stream);

/* ================================================================================================
 * Training targets from audio: frame SNR, contour finishing, priors (csrc/analysis.hip, DESIGN.md "Analysis front end").  What
 * TTSDataset._create_variances (litfass/dataset/datasets.py:562-650) and __getitem__ (:398-463) do to the "snr" and "pitch"
 * variances and for the priors, on the device.  The raw F0 contour in frames, 0 where unvoiced, is the caller's (pyworld's, as in the
 * reference) or the project's own tracker's (fs2_mel_pitch below).  The "cwt" transform is fs2_op_cwt_decompose further below; "srmr" is not here.
 *
 * 1. Windowed WADA (SNR.windowed_wada(window = win_length, stride = hop / win_length, use_samples = True), litfass/dataset/snr.py:
 *    194-271, 328-371).  Per utterance x of n >= 1 samples, s and x~ = s x (an fp32 product) as in fs2_mel_run; Te = ceil(n / hop)
 *    windows, window t = [t hop, min(t hop + win_length, n)) - the framing of the energy output.  win_length % hop == 0 is required
 *    (FS2_ERR_SHAPE from fs2_mel_snr otherwise).  The statistic of a window:
 *        a_j = max(|x~_j|, 1e-20),  v1 = max(1e-20, mean a),  v2 = mean ln a,  v3 = ln v1 - v2
 *    (the terms |x~_j| and ln a_j in fp32 - the accurate logarithm -, every sum, the two means and v3 in fp64; the means divide by the
 *    samples the window has).  The table g[0 .. K - 1] (double) belongs to the dB values db_lo + i; the reference has K = 121,
 *    db_lo = -20.  i* = max{ i : g[i] < v3 } - NOT a binary search: the reference's table is not monotone (index 2 -> 3), so the
 *    largest index that satisfies the predicate is the definition.  No i*, or i* = K - 1: the window is NaN.  Otherwise
 *        out = i* + (v3 - g[i*]) / (g[i* + 1] - g[i*])
 *    in double, rounded once to fp32, and NaN unless out < K - 1.  That is the reference's snr + 20 for -20 < snr < 100 (out = snr -
 *    db_lo: db_lo names the table's first entry and does not enter the arithmetic).  DELIBERATE DIFFERENCE: the reference then
 *    splits the window's energy with that estimate and returns 10 log10(dSigEng / dNoiseEng), which is the estimate again to
 *    float64 rounding; that round trip is not reproduced.  A window is also NaN when every |x~_j| is zero, or when the sum of
 *    x~_j^2 is zero in fp32.  Rows t >= Te are zeros; samples at or past lengths[b] are never read; no sum's order depends on the
 *    batch, on S or on a row's alignment: results are bitwise batch-invariant, as the mel is.
 *    THE TABLE IS AN ARGUMENT, the project ships none: it is Kim & Stern's WADA table for gamma shape 0.4, which a litfass
 *    installation has as litfass/data/wada_values.npy.  fs2_mel_set_snr_table uploads it (HOST memory; it allocates, waits for the
 *    device when it replaces an earlier table, and may be called again): table non-null, n in [2, 512], every entry and db_lo finite,
 *    else FS2_ERR_ARG; FS2_ERR_STATE on a handle whose create failed.
 *    fs2_mel_snr: wav, lengths, B, S, peak_normalize, ws as fs2_mel_run (ws: fs2_mel_ws_bytes; the peaks are computed again, nothing
 *    is shared with an earlier fs2_mel_run); snr (B, Te_max) with Te_max >= ceil(S / hop), snr_frames (B) int32 or NULL: device, written
 *    in full.  Enqueues a memset and two launches on the caller's stream; allocates nothing, never synchronises.  FS2_ERR_STATE
 *    before a table is set; every argument error is answered before the first launch.
 *
 * 2. Contour finishing (datasets.py:576-598, _interpolate :831-837), for the SNR and the pitch alike.  values (B, T) fp32 the raw
 *    frame contour, frames (B) int32 valid frames per row or NULL (= T), durations (B, L) int32 (negatives count as 0, as in
 *    fs2_op_segment_mean), phone_silent (B, L) int32 (non-zero = a silent phone) or NULL -> out (B, T) fp32, frames_out (B) int32,
 *    prior (B) fp32 or NULL.  Per row: F = min(sum of durations, frames[b]) = frames_out[b]; frame t < F belongs to the phone whose
 *    duration segment contains it.  A frame is MISSING if its value is NaN, or zero_is_missing is set and it is 0, or its phone is
 *    silent.  If every frame of [0, F) is missing, y[t] = all_missing_value (the reference: 1e-7 for pitch, 0 for SNR); otherwise
 *    y[t] is the value where present and np.interp elsewhere: v[l] + (t - l) (v[r] - v[l]) / (r - l) between the nearest present
 *    frames l < t < r, in double and rounded once; the first present value before it, the last present value after it.
 *    prior[b] = the mean of y[t] over the frames of non-silent phones, before normalisation (fp64 sums of consecutive frames in frame
 *    order, added in order), NaN if there are none.  out[t] = (y[t] - mean) / std for t < F (in double, rounded once), zeros for
 *    t >= F.  std must be finite and non-zero (FS2_ERR_ARG).  LIMITS: T <= 4096 frames, L <= 2048 phones (one workgroup holds an
 *    utterance in LDS; the reference caps an utterance at 2756 frames), FS2_ERR_SHAPE beyond.
 *    Phone level: finish with mean 0, std 1, then fs2_op_segment_mean with the stats.  DELIBERATE DIFFERENCE: the reference writes
 *    the phone means in place into the frame array it is still reading (datasets.py:633-640), so after leading zero-duration phones
 *    a later phone can read an entry that already holds a phone mean; here every phone averages the original frames.  The two agree
 *    whenever sum_{i < j} d_i >= j for every j.
 *
 * 3. fs2_op_masked_row_mean: values (B, N) fp32, counts (B) int32 or NULL (= N; clamped to [0, N]), skip (B, N) int32 or NULL ->
 *    out (B): the mean over j < counts[b] with skip[b][j] == 0 (fp64 sums of consecutive entries in order, added in order), NaN for
 *    an empty set.  The phone-level priors (over the phone means) and the duration prior (durations as fp32), datasets.py:412-435.
 * ================================================================================================ */
int fs2_mel_set_snr_table(fs2_mel* m, const double* table_host, int32_t n, float db_lo);
int fs2_mel_snr(fs2_mel* m, const float* wav, const int32_t* lengths, int32_t B, int32_t S, int32_t peak_normalize, float* snr,
                int32_t Te_max, int32_t* snr_frames, void* ws, size_t ws_bytes, void* hip_stream);
int fs2_op_contour_finish(const float* values, const int32_t* frames, const int32_t* durations, const int32_t* phone_silent, int32_t B,
                          int32_t T, int32_t L, int32_t zero_is_missing, float all_missing_value, float mean, float std, float* out,
                          int32_t* frames_out, float* prior, void* hip_stream);
int fs2_op_masked_row_mean(const float* values, const int32_t* counts, const int32_t* skip, int32_t B, int32_t N, float* out,
                           void* hip_stream);

/* ================================================================================================
 * F0 tracking: YIN contours from the waveform (csrc/analysis.hip, DESIGN.md "F0 tracking on the device").  The tracker is YIN
 * (de Cheveigne & Kawahara, "YIN, a fundamental frequency estimator for speech and music", JASA 111(4), 2002), written from the
 * published definition.  It is NOT PINNED AGAINST PYWORLD'S OUTPUT: the reference takes its contour from pw.dio + pw.stonemask
 * (litfass/dataset/datasets.py:567-575), pyworld is no dependency of this project and was not available to compare with, and the
 * contours of the two trackers differ.  Statistics that normalise a contour (mean / std, bins) must come from the tracker that made
 * it.  Only the CONTRACT of the output is pyworld's, so it goes into fs2_op_contour_finish(zero_is_missing = 1) unchanged: one value
 * per frame in Hz, 0 where unvoiced, Tf = 1 + n / hop frames, frame t centred on sample t hop.
 *
 * Per utterance x of n >= 1 samples, x[j] = 0 outside [0, n); W = win_length and hop of the handle;
 *     tau_max = ceil(sr / f0_floor),  tau_min = max(2, floor(sr / f0_ceil))
 * (pyworld's range 71 .. 800 Hz at 22050 Hz: 27 .. 311; the usual threshold is 0.1).
 *   1. frames t = 0 .. Tf - 1, Tf = 1 + n / hop, s = t hop - W / 2
 *   2. difference function, tau = 0 .. tau_max + 1:  d(tau) = sum_{j = 0}^{W - 1} (x[s + j] - x[s + j + tau])^2
 *   3. cumulative mean normalised difference:  d'(0) = 1,  d'(tau) = d(tau) tau / sum_{k = 1}^{tau} d(k),  1 where that sum is 0
 *   4. pick: the smallest tau in [tau_min, tau_max] with d'(tau) < threshold; then, while tau + 1 <= tau_max and
 *      d'(tau + 1) < d'(tau), step forward.  No lag below the threshold: the frame is unvoiced, f0 = 0 and dmin = min d' over
 *      [tau_min, tau_max]
 *   5. refinement on d':  a, b, c = d'(tau - 1), d'(tau), d'(tau + 1),  curv = a - 2 b + c,
 *      delta = (a - c) / (2 curv) clamped to [-0.5, 0.5] if curv > 0, else 0;  f0 = sr / (tau + delta),  dmin = b
 *   6. frames at or past Tf are zeros in every output
 * The definition is scale-invariant (d' is a ratio of sums of squares), so there is no peak normalisation and no workspace.
 * Arithmetic: the direct form (x[j] - x[j + tau])^2 in fp32 - no cancellation, unlike e(0) + e(tau) - 2 r(tau); where W % hop == 0
 * per-hop partial sums, a frame's W / hop added left to right; the running sum of step 3, the quotient and step 5 in fp64, rounded
 * once.  No sum's order depends on B, S, the padding or the row: results are bitwise batch-invariant.  Samples at or past
 * lengths[b] are never read.
 *
 * fs2_mel_pitch: wav (B, S) fp32, lengths (B) int32 (clamped to [0, S]; 0 = no frames): device.  f0 (B, Tf_max) fp32 with
 * Tf_max >= 1 + S / hop; f0_frames (B) int32 or NULL; dmin (B, Tf_max) or NULL; cmnd (B, Tf_max, n_lags) or NULL - DIAGNOSTIC, d' for
 * tau = 0 .. n_lags - 1, what the tests hold the continuous stage to; n_lags must equal tau_max + 2 when cmnd is given and is ignored
 * otherwise.  Device, each written in full.  One launch on the caller's stream; allocates nothing, never synchronises.
 * FS2_ERR_SHAPE when tau_max + 2 > 1024, tau_min >= tau_max, threshold lies outside (0, 1], sample_rate, f0_floor or f0_ceil is not
 * positive, hop is no multiple of 4 (the span is read in 16-byte words), or one frame's span and partials do not fit LDS;
 * FS2_ERR_ARG for NULL wav / lengths / f0, B or S < 1, Tf_max too small, a wrong n_lags; B > 65535 is FS2_ERR_SHAPE.  Every error is
 * answered before the launch, with a message in fs2_mel_last_error, and writes nothing.
 * fs2_mel_pitch_lags validates (sample_rate, f0_floor, f0_ceil) on the host alone and reports the lag range.
 * fs2_mel_pitch_tile_frames is DIAGNOSTIC (as fs2_mel_tile_frames): the consecutive frames one workgroup owns - where the kernel's
 * seams lie -, 0 for a range fs2_mel_pitch_lags would refuse.
 * ================================================================================================ */
int fs2_mel_pitch(fs2_mel* m, const float* wav, const int32_t* lengths, int32_t B, int32_t S, int32_t sample_rate, float f0_floor,
                  float f0_ceil, float threshold, float* f0, int32_t Tf_max, int32_t* f0_frames, float* dmin, float* cmnd, int32_t n_lags,
                  void* hip_stream);
int fs2_mel_pitch_lags(fs2_mel* m, int32_t sample_rate, float f0_floor, float f0_ceil, int32_t* tau_min, int32_t* tau_max);
int32_t fs2_mel_pitch_tile_frames(fs2_mel* m, int32_t sample_rate, float f0_floor);

/* ================================================================================================
 * CWT and log variance targets: CWT.decompose on the device (csrc/cwt.hip, DESIGN.md "CWT decomposition on the device").  What the
 * reference's transform step does to a variance whose transform is "cwt" (litfass/dataset/datasets.py:641-642, dataset/cwt.py:30-46)
 * over scipy.signal.cwt and scipy.signal.ricker AS SCIPY 1.14 PUBLISHED THEM, written from that definition.  It is NOT PINNED AGAINST
 * scipy.signal.cwt'S OUTPUT: SciPy removed both functions in 1.15 and they were not available to compare with; tests/_cwt_ref.py
 * restates them and is held to the reference's own text where that tree is present.
 *
 * values (B, S) fp32, a finished contour per row (frame level: fs2_op_contour_finish; phone level: fs2_op_segment_mean); counts (B)
 * int32 clamped to [0, S], or NULL (= S); n_scales in 1 .. 16 (the reference: 10); tau (the reference: 0.2833425).  Per row, n = count:
 *   1. original[j] = values[j], an exact 0 (of either sign) replaced by float32(1e-7)
 *   2. signal[j] = log(original[j]) in fp64, rounded to fp32; a negative entry gives NaN, as numpy does
 *   3. mean = the mean of signal[0 .. n), std = the population standard deviation sqrt(mean((signal - mean)^2)): fp64; entry j is
 *      added to partial j mod 256 in ascending order and the 256 partials by a binary tree - an order that depends on n alone.
 *      mean_std[b] = {float32(mean), float32(std)}
 *   4. x[j] = (signal[j] - mean) / (std + float32(1e-7)) with the fp32 operands and fp32 arithmetic the reference has
 *   5. per scale i = 1 .. n_scales:  w = 2^(i + 1) tau;  N = min(10 w, n), a real number, an integer only when n truncates it;
 *      M = ceil(N) points;  r[m] = A (1 - v^2 / w^2) exp(-v^2 / (2 w^2)) with v = m - (N - 1) / 2 and A = 2 / (sqrt(3 w) pi^(1/4)) -
 *      for a non-integer N the wavelet is NOT symmetric about its middle sample, and that is reproduced;
 *          c_i[k] = sum_j x[j] r[M - 1 - (k + (M - 1) / 2 - j)]     (integer division; over the j whose index lies in [0, M))
 *      - scipy.signal.convolve(x, r[::-1], mode = "same") as SciPy centres it -;  spectrogram[k][i - 1] = float32(c_i[k] (i + 2.5)^(-5/2)).
 *      Wavelet values, products and sums are fp64: one accumulator per output from +0, taps in ascending order of j (fused
 *      multiply-adds), so the result is the fp32 rounding of what the reference computes in float64.
 *   6. every entry of original, signal and spectrogram at or past n is written as zero.  n = 0: mean_std[b] is NaN (numpy's mean of
 *      nothing) and nothing else of the row is written.  n = 1 or a constant row: std = 0 exactly and a spectrogram of exact zeros.
 * No sum's order depends on B, S or the row's place in the batch: results are bitwise batch-invariant.  values at or past a row's
 * count are never read.
 *
 * fs2_op_cwt_decompose: original (B, S), signal (B, S), spectrogram (B, S, n_scales), mean_std (B, 2): fp32, device, each may be
 * NULL (a NULL spectrogram skips steps 4 and 5).  One launch on the caller's stream; allocates nothing, never synchronises, needs no
 * workspace.  LIMITS: S <= 4096 (fs2_op_contour_finish's cap) and B <= 65535, FS2_ERR_SHAPE beyond; FS2_ERR_ARG for NULL values,
 * B or S < 1, n_scales outside 1 .. 16, tau outside [1e-100, 1e100] or NaN.  A refusal writes nothing.
 * The "log" transform (datasets.py:643-644) needs no operator: it is the log of the unnormalised variance.
 * ================================================================================================ */
int fs2_op_cwt_decompose(const float* values, const int32_t* counts, int32_t B, int32_t S, int32_t n_scales, double tau, float* original,
                         float* signal, float* spectrogram, float* mean_std, void* hip_stream);

/* ================================================================================================
 * Stochastic duration predictor at inference (duration_stochastic=True: the VITS spline-flow predictor of
 * litfass/third_party/stochastic_duration_predictor/sdp.py:249-349 with reverse=True, as StochasticDurationPredictorWrapper calls it,
 * litfass/fastspeech2/model.py:463-479).  A handle of its own, in the pattern of fs2_mel_*: create validates on the host alone.
 *   fs2_sdp_create: H = in_channels (the encoder width), F = hidden_channels, k = kernel_size, n_flows = the wrapper's nlayers.
 *    Supported: F == 256, k == 3, 1 <= n_flows <= 8, H a multiple of 16 in 16 .. 256 (`pre` runs inside the conditioning launch);
 *    anything else is FS2_ERR_SHAPE and fs2_sdp_supported answers 0.  A bad abi_version is FS2_ERR_ARG.  As with fs2_mel_create the
 *    handle is returned on failure too, for fs2_sdp_last_error; destroy it.
 *   fs2_sdp_load_weight: fp32 HOST data under the reference's state_dict names relative to "variance_adaptor.duration_predictor."
 *    ("sdp.pre.weight", "sdp.convs.convs_sep.0.weight", "sdp.convs.norms_1.0.gamma", "sdp.flows.0.translation",
 *    "sdp.flows.2.proj.weight", ...) with the reference's shapes.  The training-only tensors (sdp.post_pre / post_convs / post_proj /
 *    post_flows.*, and sdp.flows.1.*, the ConvFlow the inference loop drops) are shape-checked and dropped.  An unknown name or a wrong
 *    shape is FS2_ERR_WEIGHT.
 *   fs2_sdp_finalize packs and uploads; FS2_ERR_WEIGHT names the first on-path tensor that is missing.
 *   fs2_sdp_forward: x (B, L, H) of x_dtype (FS2_F32, FS2_BF16, FS2_F16; converted to fp32 as the rows are read), pad_mask (B, L)
 *    1 = pad, noise (B, 2, L) fp32 standard normal ALREADY scaled by noise_scale, logw (B, L) fp32 out, 0 at pads; all device.
 *    workspace: fs2_sdp_workspace_bytes(h, B, L) device bytes, 16-byte aligned (FS2_ERR_NOMEM if short; n_flows == 1 needs none).
 *    Launches: one for the text conditioning, one per ConvFlow that runs (n_flows - 1 of them: CF_n .. CF_2), the ElementwiseAffine
 *    folded into the last; n_flows == 1 is a single row launch.  fs2_sdp_launches reports the count.  All arithmetic is fp32 (1x1 convs
 *    on the fp32 MFMA) with accurate exp / log / erf / sqrt, whatever x_dtype.  The bits of an utterance's logw do not depend on B, on
 *    L, or on where its rows fall in a tile.  Allocates nothing, never synchronises.
 *   fs2_sdp_tile_rows: the finished rows per workgroup (tiles start at its multiples from an utterance's first row).
 *   fs2_op_rq_spline_inverse: out[i] = the inverse of the unconstrained rational-quadratic spline with linear tails (tail_bound 5,
 *    10 bins; transforms.py:51-191) at x1[i] with parameters h29[i][0..28] (widths and heights are divided by sqrt(F)); the device
 *    function of the flow launch.  Where the reference asserts a non-negative discriminant this clamps it at 0.
 *   fs2_op_durations_stochastic: fs2_op_durations with the stochastic model's rule (model.py:302-309):
 *    d = int(clamp(ceil(exp(logw + 1e-9)), 0)) in float32 as written, 0 where logw == 0; then the same zero-duration guard, forced
 *    durations and prefix sums.  A value beyond int32 SATURATES at INT32_MAX and NaN gives 0, as in fs2_op_durations.
 * ================================================================================================ */
typedef struct fs2_sdp fs2_sdp;
int fs2_sdp_supported(int32_t H, int32_t F, int32_t k, int32_t n_flows);
int fs2_sdp_create(int32_t abi_version, int32_t H, int32_t F, int32_t k, int32_t n_flows, fs2_sdp** out);
int fs2_sdp_destroy(fs2_sdp* h);
const char* fs2_sdp_last_error(const fs2_sdp* h);
int32_t fs2_sdp_tile_rows(const fs2_sdp* h);
int fs2_sdp_launches(const fs2_sdp* h);
int fs2_sdp_load_weight(fs2_sdp* h, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);
int fs2_sdp_finalize(fs2_sdp* h);
int fs2_sdp_workspace_bytes(const fs2_sdp* h, int32_t B, int32_t L, size_t* bytes);
int fs2_sdp_forward(fs2_sdp* h, int32_t x_dtype, const void* x, const uint8_t* pad_mask, const float* noise, float* logw,
                    void* workspace, size_t workspace_bytes, int32_t B, int32_t L, void* hip_stream);
int fs2_op_rq_spline_inverse(const float* x1, const float* h29, int32_t F, float* out, int32_t rows, void* hip_stream);
int fs2_op_durations_stochastic(const float* logw, const uint8_t* src_mask, const int32_t* forced, int32_t* dur, int32_t* cum,
                                int32_t* totals, int32_t* guard, int32_t B, int32_t L, void* hip_stream);

/* ================================================================================================
 * HiFi-GAN generator: the step right after the mel forward.  Replaces
 * litfass.third_party.hifigan.Synthesiser.__call__ -> Generator.forward
 * (litfass/third_party/hifigan/__init__.py:19-43, models.py:112-165), resblock type "1".
 * Weights are passed under the generator's own state_dict names AFTER remove_weight_norm
 * ("conv_pre.weight", "ups.0.weight" (Cin, Cout, k), "resblocks.3.convs1.0.weight", "conv_post.bias" ...);
 * the host mirror (lightningfastspeech2_amd/hifigan.py) folds weight_g / weight_v pairs.
 * ================================================================================================ */
#define FS2_VOC_MAX_STAGES 8
#define FS2_VOC_MAX_KERNELS 4
typedef struct fs2_voc_config {
    int32_t abi_version;      /* FS2_ABI_VERSION */
    int32_t dtype;            /* FS2_F32 (parity mode, fp32 MFMA), FS2_BF16 (throughput mode) or FS2_F16: bf16's kernels, tiles and byte
                                 counts with every stored tensor - the packed weights, the mel at conv_pre's slab fill, the streams
                                 between launches, the LDS slabs of the resident resblocks, the stage means - in IEEE binary16 under
                                 FS2_F16's storage rule (saturating stores).  Accumulation, biases, the 1 / n_kernels scale, conv_post,
                                 tanh and the wav are fp32 in all three.  The engine modes (FS2_MIXED*, FS2_F32_X3) are FS2_ERR_ARG. */
    int32_t n_mels;           /* 80 */
    int32_t initial_channel;  /* upsample_initial_channel (config.json:13); halves per stage, multiples of 32 */
    int32_t n_stages;
    int32_t up_rates[FS2_VOC_MAX_STAGES];     /* upsample_rates; kernel - 2 * padding must equal the rate */
    int32_t up_kernels[FS2_VOC_MAX_STAGES];   /* upsample_kernel_sizes */
    int32_t n_kernels;                        /* len(resblock_kernel_sizes) */
    int32_t rb_kernels[FS2_VOC_MAX_KERNELS];  /* odd */
    int32_t rb_dilations[FS2_VOC_MAX_KERNELS][3];
} fs2_voc_config;
typedef struct fs2_vocoder fs2_vocoder;

int fs2_voc_create(const fs2_voc_config* cfg, fs2_vocoder** out);
void fs2_voc_destroy(fs2_vocoder* v);
const char* fs2_voc_last_error(const fs2_vocoder* v);
/* host fp32 data; ndim/shape as torch reports them */
int fs2_voc_load_weight(fs2_vocoder* v, const char* name, const float* data, const int64_t* shape, int32_t ndim);
int fs2_voc_finalize(fs2_vocoder* v);
/* samples per mel frame = prod(up_rates) */
int32_t fs2_voc_hop(const fs2_vocoder* v);
/* mel: (B, T, n_mels) fp32 device (FastSpeech2's output layout); lengths: (B) int32 device valid frames
 * per utterance or NULL; wav: (B, T * hop) fp32 device in [-1, 1] (samples past an utterance's length
 * are left untouched).  Each utterance is synthesised as the reference does it: alone, zero padding at
 * its own ends in every layer (generator.py:163-170). */
int fs2_voc_synthesize(fs2_vocoder* v, const float* mel, const int32_t* lengths, int32_t B, int32_t T, float* wav,
                       void* hip_stream);
/* parity tap: copy stage output `stage` (0 = conv_pre, i = after upsample stage i) of the last call as
 * fp32 (B, T * up_i, C_i) into a device buffer */
int fs2_voc_debug_copy(fs2_vocoder* v, int32_t stage, float* dst, void* hip_stream);
/* Which kernel instantiation every launch of the last fs2_voc_synthesize was, in launch order (host only; written by the launchers
 * where they pick the instantiation).  Returns the number of launches and copies the first min(count, cap) codes to `codes` (host
 * memory; may be NULL with cap 0); negative = bad argument.  A code, from bit 0:
 *   bit 0        0 = vocoder_conv_kernel<T, MI16, CP>, 1 = vocoder_resblock_kernel<T, MI16, CH, NW, MID>
 *   bits 1-3     T as FS2_F32 / FS2_BF16 / FS2_F16
 *   conv:        bits 4-7 MI16 (14 / 8 / 4 / 2); bits 8-17 CP (0 = the runtime-stride build); bit 18 the input is the fp32 mel (conv_pre);
 *                bit 19 conv_post; bit 20 two tap windows (a transposed conv)
 *   resblock:    bits 4-13 the form 100 * NW + MI16 (408 / 808 / 804); bits 14-21 CH; bits 22-23 pairs in the launch (3 / 1);
 *                bit 24 MID (the result is stored activated); bit 25 the input stream is stored activated */
int32_t fs2_voc_last_launches(const fs2_vocoder* v, int32_t* codes, int32_t cap);

/* ================================================================================================
 * FastDiff vocoder at inference (litfass/third_party/fastdiff/FastDiff.py:91-195, module/modules.py:116-343,
 * module/util.py:158-237, 305-343): SpeechGenerator(fastdiff=True)'s model.fastdiff_model.inference(mel, N).  A handle of its own in the
 * pattern of fs2_sdp_*: create validates on the host alone and returns the handle on failure too (fs2_fd_last_error, then destroy).
 *   Architecture: the reference's defaults ONLY - inner_channels 32, cond_channels 80, upsample_ratios {8, 8, 4}, 4 LVC layers of kernel
 *    3, kpnet_hidden 64, kpnet_conv 3, step embedding 128 / 512 / 512.  Anything else: fs2_fd_supported answers 0, create FS2_ERR_SHAPE.
 *   dtype: FS2_F32 (parity mode: fp32 MFMA, accurate exp / tanh) or FS2_BF16 (the packed conv weights, the predicted kernels and biases,
 *    the conditioning and every 32 / 64-channel stream between launches are stored in bf16, each MFMA operand is rounded to bf16 after its
 *    input LeakyReLU; accumulation, first_audio_conv, final_conv, the gate, the diffusion state x, the noise, eps, the sampler update and
 *    the peak scale stay fp32).  Other dtypes: FS2_ERR_ARG.
 *   fs2_fd_load_weight: host fp32 under the reference's state_dict names after remove_weight_norm ("first_audio_conv.weight",
 *    "fc_t1.weight", "downsample.0.conv.1.bias", "lvc_blocks.2.kernel_predictor.kernel_conv.weight", "lvc_blocks.0.upsample.weight"
 *    (Cin, Cout, 2r), "lvc_blocks.1.fc_t.weight", "final_conv.0.weight" ...).  Unknown name / wrong shape: FS2_ERR_WEIGHT.
 *   fs2_fd_finalize packs (MFMA fragment order; kernel_conv's rows permuted into the order the LVC launch reads) and uploads.
 *   Every utterance is computed alone, with zero padding at its own ends in every layer (generator.py:163-168); lengths (B) int32 device
 *    valid frames or NULL (= T).  The bits of an utterance's result do not depend on B, T or its place in the batch: every launch tiles
 *    an utterance in fs2_fd_tile_rows rows from its own first row.  The batch is walked in chunks of utterances so that the workspace
 *    stays under a cap: fs2_fd_set_chunk(h, n) limits a chunk to n utterances (0 = the default, as many as fit 2 GiB, at least one);
 *    fs2_fd_workspace_bytes reports the bytes for (B, T) under the current limit (device, 256-byte aligned; FS2_ERR_NOMEM if short).
 *   fs2_fd_denoise: one eps evaluation, FastDiff.forward(x, c, ts): x (B, T*hop) fp32, mel (B, T, 80) fp32, step = the (fractional)
 *    diffusion step, eps (B, T*hop) fp32 out; rows past an utterance's length are left untouched.
 *   fs2_fd_sample: FastDiff.inference(c, N), ddim off, N in {3, 4, 6, 8} (others FS2_ERR_SHAPE): noise (N, B, T*hop) fp32 -
 *    noise[0] is x_T, noise[j] (j >= 1) the draw added after reverse step n = N - j (the reference's order of drawing) - and
 *    wav (B, T*hop) fp32 = x_0 / max|x_0| over the utterance's own samples; samples past its length are left untouched.
 *   fs2_fd_launches(h, N): kernel launches per chunk of fs2_fd_sample with N steps; N = 0: of fs2_fd_denoise.
 *   fs2_fd_schedule (host only): beta, alpha-bar, sigma and the mapped fractional steps of N, float32 as the reference computes them.
 *   All launches go to the caller's stream; nothing is allocated and nothing synchronises on the call path.  Every argument, the
 *   schedule and the workspace size are judged on the host before the first launch.
 *   Pieces for tests:
 *   fs2_fd_predict_kernels: block's kernel predictor on mel + fc_t(step embedding): kernels (B, T, 24576) and bias (B, T, 256) in the
 *    handle's dtype, kernels in the LVC launch's order: fs2_fd_kernel_index(dtype, layer, in, out, k) is the position of the reference's
 *    kernels[layer, in, out, k] inside a frame's 24576; bias is in the reference's order (layer * 64 + out).
 *   fs2_op_lvc: one location-variable convolution with gate and residual (modules.py:214-217): with l = t / hop,
 *    o[t, n] = bias[l, layer*64 + n] + sum_{c < 32, k < 3} y[t + k - 1, c] * K[l, layer, c, n, k]  (y = 0 outside the utterance only),
 *    out[t, c] = x[t, c] + sigmoid(o[t, c]) * tanh(o[t, 32 + c]) (+ add[t, c] when add is not NULL); y, x, add, out (B, T*hop, 32),
 *    kernels, bias as above, all of dtype; hop in {8, 64, 256}; out may alias x.
 *   fs2_op_fd_dblock: DiffusionDBlock `block` (0, 1, 2: factors 4, 8, 8) of the handle: x (B, S, 32) -> out (B, S / f, 32) in the
 *    handle's dtype, S = T * 256 / {1, 4, 32}, an utterance's rows = lengths * that; tmp: 3 * B * (S / f) * 32 elements.
 * ================================================================================================ */
typedef struct fs2_fd fs2_fd;
int fs2_fd_supported(int32_t inner_channels, int32_t cond_channels, const int32_t* upsample_ratios, int32_t n_ratios, int32_t lvc_layers,
                     int32_t lvc_kernel, int32_t kpnet_hidden, int32_t kpnet_conv, int32_t embed_in, int32_t embed_mid, int32_t embed_out);
int fs2_fd_create(int32_t abi_version, int32_t dtype, int32_t inner_channels, int32_t cond_channels, const int32_t* upsample_ratios,
                  int32_t n_ratios, int32_t lvc_layers, int32_t lvc_kernel, int32_t kpnet_hidden, int32_t kpnet_conv, int32_t embed_in,
                  int32_t embed_mid, int32_t embed_out, fs2_fd** out);
int fs2_fd_destroy(fs2_fd* h);
const char* fs2_fd_last_error(const fs2_fd* h);
int fs2_fd_load_weight(fs2_fd* h, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);
int fs2_fd_finalize(fs2_fd* h);
int32_t fs2_fd_hop(const fs2_fd* h);
int32_t fs2_fd_tile_rows(const fs2_fd* h);
int fs2_fd_launches(const fs2_fd* h, int32_t N);
int fs2_fd_set_chunk(fs2_fd* h, int32_t max_utterances);
int fs2_fd_workspace_bytes(const fs2_fd* h, int32_t B, int32_t T, size_t* bytes);
int fs2_fd_schedule(int32_t N, float* beta, float* alpha, float* sigma, float* step);
int fs2_fd_denoise(fs2_fd* h, const float* x, const float* mel, const int32_t* lengths, float step, float* eps, void* workspace,
                   size_t workspace_bytes, int32_t B, int32_t T, void* hip_stream);
int fs2_fd_sample(fs2_fd* h, const float* mel, const int32_t* lengths, const float* noise, int32_t N, float* wav, void* workspace,
                  size_t workspace_bytes, int32_t B, int32_t T, void* hip_stream);
int fs2_fd_predict_kernels(fs2_fd* h, int32_t block, const float* mel, const int32_t* lengths, float step, void* kernels, void* bias,
                           void* workspace, size_t workspace_bytes, int32_t B, int32_t T, void* hip_stream);
int64_t fs2_fd_kernel_index(int32_t dtype, int32_t layer, int32_t in_channel, int32_t out_channel, int32_t k);
int fs2_op_lvc(int32_t dtype, int32_t hop, int32_t layer, const void* y, const void* kernels, const void* bias, const void* x,
               const void* add, void* out, const int32_t* lengths, int32_t B, int32_t T, void* hip_stream);
int fs2_op_fd_dblock(fs2_fd* h, int32_t block, const void* x, void* out, void* tmp, const int32_t* lengths, int32_t B, int32_t T,
                     void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FS2_H_ */
