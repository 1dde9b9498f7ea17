// Host side of libfs2_hip.so: weight store (reference state_dict names), packing/folding, the
// two-phase forward and the extern "C" surface declared in include/fs2.h.
//
// Forward composition follows FastSpeech2.forward (litfass/fastspeech2/fastspeech2.py:636-731)
// and VarianceAdaptor.forward (litfass/fastspeech2/model.py:249-341); see DESIGN.md for the
// kernel-by-kernel map.
#include <math.h>
#include <string.h>

#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "fs2_host.h"

using namespace fs2;

namespace {

struct ConvW {     // dense conv or pointwise: W (N, taps*Cin) in its side's dtype, bias fp32
    void* w = nullptr;
    float* b = nullptr;
    int N = 0, Cin = 0, taps = 1;
    int dt = FS2_F32;  // dtype of w and of the activations this layer reads
    bool presplit = false;  // split-arithmetic modes: w holds bf16 heads + tails per 32-channel chunk (pack_presplit_weights), not fp32
};
struct DwW {       // depth-wise conv weights fp32 (C, k) + bias
    float* w = nullptr;
    float* b = nullptr;
    int C = 0, k = 1;
};
struct LayerW {
    ConvW in_proj, out_proj;
    void* wo_pk = nullptr;  // out_proj.weight in the single-launch predictor's fragment order (attn_out_ln_kernel; bf16 encoder layers, H = 256, 2 heads)
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
    bool depthwise = false;
    DwW dw;          // conv1.0 (depth-wise only)
    ConvW c1, c2;    // dense: conv1 (k taps) / conv2; depth-wise: conv1.1 / folded conv2.0*conv2.1
    // layer i >= 1 of a stack of wide depth-wise bf16 blocks: the in-projection with the PREVIOUS block's norm2 folded in -
    // W' = W_in diag(gamma2), b' = b_in + W_in beta2, in_wg[n] = sum_k W'[n][k] (of the bf16 values as stored) - for
    // fs2_op_gemm_rowscale's epilogue on the previous block's pre-norm output (no normalise-only pass in between)
    ConvW in_proj_f;
    float* in_wg = nullptr;
    bool has_fold = false;
};
struct PredLayerW {
    bool depthwise = false;
    DwW dw;
    ConvW c;
    float *g = nullptr, *b = nullptr;
};
struct PredictorW {
    int dt = FS2_F32;
    bool cwt = false;   // CWT head: head_mat = Linear(filter, 10) padded to 12 rows, ms_w / ms_b = mean_std_linear
    ConvW head_mat;
    float *ms_w = nullptr, *ms_b = nullptr;
    std::vector<PredLayerW> layers;
    float* head_w = nullptr;
    float head_b = 0.f;
    // wide depth-wise predictors (deferred LayerNorms): the last LayerNorm + head from the last GEMM's epilogue sums (GemmArgs::head_out):
    // head_gw = gamma_last * w_head, its sum, and beta_last . w_head + head_b
    float* head_gw = nullptr;
    float head_sum_gw = 0.f, head_cst = 0.f;
    int filt = 0;
    // one-launch path (predictor_fused.hip): weights in MFMA fragment order, per-layer vectors stacked
    void* wpk = nullptr;
    float *bias_all = nullptr, *g_all = nullptr, *b_all = nullptr;
    // ... of depth-wise layers (H = 256, k = 3; r06): wpk = the pointwise weights, dw_all (nl, 3, H) / dwb_all (nl, H) the depth-wise taps + bias
    float *dw_all = nullptr, *dwb_all = nullptr;
    // ... in the split arithmetic (fp32x3 / mixed3 engines): wpk = the weights' bf16 heads, wpk_lo their tails (launch_predictor_fused_x3)
    void* wpk_lo = nullptr;
};
struct VarianceW {
    PredictorW pred;
    float* bins = nullptr;
    float* emb = nullptr;
};

struct ProfSlot {
    bool enabled = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
    double flops = 0, bytes = 0;
};

struct PersistBufs {  // what fs2_encode leaves for fs2_decode
    float* spk = nullptr;
    void *xA = nullptr, *xB = nullptr;  // (B*L, H) encoder ping-pong; xA = encoder_out
    float* dur_pred = nullptr;
    int32_t *d_dur = nullptr, *d_cum = nullptr, *d_totals = nullptr, *d_guard = nullptr;
    uint8_t* src_mask = nullptr;
    // phone-level variances (fs2_config::var_level; model.py:276-294): predictions (B*L) and, for a CWT head, spectrogram (B*L, 10) +
    // (B, 2) mean / std - produced by fs2_encode, kept in the persist arena, copied out by fs2_decode
    float* pv_pred[FS2_MAX_VARIANCES] = {nullptr, nullptr, nullptr, nullptr};
    float* pv_spec[FS2_MAX_VARIANCES] = {nullptr, nullptr, nullptr, nullptr};
    float* pv_ms[FS2_MAX_VARIANCES] = {nullptr, nullptr, nullptr, nullptr};
};

// An engine is three parts.  Model: what fs2_create / fs2_finalize produce and nobody writes afterwards - fs2_clone shares it (one
// assignment: a field added here reaches every clone).  Switches: the A/B settings a clone inherits.  Everything else in fs2_engine
// is the run state of one engine.
struct Model {
    fs2_config cfg;
    int dt = FS2_F32;          // configured mode (an fs2_dtype engine mode)
    int fdt = FS2_F32, bdt = FS2_F32;  // storage dtype of the front (encoder + variance adaptor: every discrete decision)
                                       // and of the back (decoder + mel head); they differ in the FS2_MIXED* modes (back: bf16 or f16)
    size_t esz = 4;            // bytes per activation element, the larger of the two (arena sizing)
    bool front_split = false;  // FS2_MIXED_X3 / FS2_F32_X3: the fp32 GEMMs / convs (the front's / all of them) run as bf16 x 3 split products
    // device weight blocks: owned jointly by an engine and its fs2_clone()s (freed with the last of them)
    std::shared_ptr<DevAllocs> dev_allocs = std::make_shared<DevAllocs>();
    // device weights
    float *phone_table = nullptr, *pe = nullptr, *spk_w = nullptr, *spk_b = nullptr;
    std::vector<LayerW> enc, dec;
    PredictorW dur;
    std::vector<VarianceW> vars;
    ConvW mel;
    ConvW mel_f;               // the mel head with the last decoder block's norm2 folded in (wide depth-wise bf16 decoders), mel_wg its row sums
    float* mel_wg = nullptr;
    bool mel_fold = false;
    std::vector<VarianceW> priors_w;  // bins + relu(embedding) per prior (predictor unused)
    // duration_stochastic=True (fs2_set_stochastic_duration): the stochastic duration predictor's handle (sdp.hip) stands in for `dur`
    bool dur_stochastic = false;
    std::shared_ptr<fs2_sdp> sdp;
};
struct Switches {
    bool fuse_predictor = true;
    // fs2_set_graphs: the decode phase replayed as a hipGraph (one launch instead of ~50) once a shape / buffer signature repeats
    bool use_graph = false;
    bool zero_pad_mel = false;
    bool defer_ln = true;      // hidden > 256, depth-wise blocks: LayerNorm deferred into its consumers (A/B: fs2_set_deferred_layernorm)
    bool fold_ln = true;       // ... and a block's closing norm2 folded into the next block's in-projection (bf16; A/B: fs2_set_folded_layernorm)
    Tuning tune;               // this engine's A/B switches (fs2_set_tuning; copied by fs2_clone): every launch of the engine points at them
};

}  // namespace

struct fs2_engine : Model, Switches, ErrorBase {
    bool finalized = false;
    bool debug = false;        // (not inherited by a clone)
    struct GraphEntry { std::vector<uint64_t> key; hipGraphExec_t exec = nullptr; uint64_t stamp = 0; bool bad = false; };
    std::vector<GraphEntry> dgraphs, egraphs;  // decode phase / encode phase
    hipStream_t gstream = nullptr;
    hipEvent_t gev_in = nullptr, gev_out = nullptr;
    uint64_t gclock = 0;
    long graph_replays = 0;
    WeightStore w;  // the expected tensors (empty: fs2_create did not succeed) and fs2_load_weight's values, until fs2_finalize has packed them
    const float* priors_dev = nullptr;
    int priors_B = 0;
    bool weight_seen = false;          // a fs2_load_weight has been accepted: the architecture switches are closed
    const float* noise_dev = nullptr;  // fs2_set_duration_noise: the next encode's (B, 2, L) noise, one-shot
    int noise_B = 0, noise_L = 0;
    Arena persist, scratch, dbg, dbg_enc;
    int B = 0, L = 0, T = 0;
    bool encoded = false;
    bool mid_forward = false;  // fs2_encode done, fs2_decode not yet: the persist arena is live
    PersistBufs ps;               // this batch's buffers in the persist arena (layout_persist)
    int32_t* h_pinned = nullptr;  // 2*B ints: totals, guard
    int h_pinned_cap = 0;
    std::vector<int32_t> totals, guard;
    std::map<std::string, std::pair<void*, size_t>> taps;
    const int32_t* forced_idx[FS2_MAX_VARIANCES] = {nullptr, nullptr, nullptr, nullptr};
    const float* forced_tgt[FS2_MAX_VARIANCES] = {nullptr, nullptr, nullptr, nullptr};
    ProfSlot prof[FS2_K_COUNT];
};

namespace {

// ---- expected tensors (mirror of lightningfastspeech2_amd/weights.py:state_dict_spec) -----------
void conformer_spec(fs2_engine* e, const std::string& p, int H, int F, int k, bool dw) {
    auto& s = e->w;
    s.expect(p + ".self_attn.in_proj_weight", {3 * H, H});
    s.expect(p + ".self_attn.in_proj_bias", {3 * H});
    s.expect(p + ".self_attn.out_proj.weight", {H, H});
    s.expect(p + ".self_attn.out_proj.bias", {H});
    s.expect(p + ".norm1.weight", {H});
    s.expect(p + ".norm1.bias", {H});
    s.expect(p + ".norm2.weight", {H});
    s.expect(p + ".norm2.bias", {H});
    if (dw) {
        s.expect(p + ".conv1.0.weight", {H, 1, k});
        s.expect(p + ".conv1.0.bias", {H});
        s.expect(p + ".conv1.1.weight", {F, H, 1});
        s.expect(p + ".conv1.1.bias", {F});
        s.expect(p + ".conv2.0.weight", {F, F / H, 1});
        s.expect(p + ".conv2.0.bias", {F});
        s.expect(p + ".conv2.1.weight", {H, F, 1});
        s.expect(p + ".conv2.1.bias", {H});
    } else {
        s.expect(p + ".conv1.weight", {F, H, k});
        s.expect(p + ".conv1.bias", {F});
        s.expect(p + ".conv2.weight", {H, F, 1});
        s.expect(p + ".conv2.bias", {H});
    }
}
void predictor_spec(fs2_engine* e, const std::string& p, int nl, int cin, int filt, int k, bool dw, int n_out = 1) {
    auto& s = e->w;
    for (int j = 0; j < nl; ++j) {
        const std::string q = p + ".layers." + std::to_string(j) + ".layers";
        if (dw) {
            s.expect(q + ".0.module.0.weight", {cin, 1, k});
            s.expect(q + ".0.module.0.bias", {cin});
            s.expect(q + ".0.module.1.weight", {filt, cin, 1});
            s.expect(q + ".0.module.1.bias", {filt});
        } else {
            s.expect(q + ".0.module.weight", {filt, cin, k});
            s.expect(q + ".0.module.bias", {filt});
        }
        s.expect(q + ".2.weight", {filt});
        s.expect(q + ".2.bias", {filt});
    }
    s.expect(p + ".linear.weight", {n_out, filt});
    s.expect(p + ".linear.bias", {n_out});
}
void build_spec(fs2_engine* e) {
    const fs2_config& c = e->cfg;
    const int H = c.hidden;
    e->w.expect("phone_embedding.weight", {c.n_phones, H});
    for (int i = 0; i < c.enc_layers; ++i)
        conformer_spec(e, "encoder.layers." + std::to_string(i), H, c.enc_filter, c.enc_kernels[i], c.enc_depthwise);
    for (int i = 0; i < c.dec_layers; ++i)
        conformer_spec(e, "decoder.layers." + std::to_string(i), H, c.dec_filter, c.dec_kernels[i], c.dec_depthwise);
    e->w.expect("positional_encoding.pe", {1, c.pe_len, H});
    if (!e->dur_stochastic)  // (a stochastic predictor's tensors are the sdp handle's: fs2_load_weight hands them on)
        predictor_spec(e, "variance_adaptor.duration_predictor", c.dur_nlayers, H, c.dur_filter, c.dur_kernel, c.dur_depthwise);
    for (int v = 0; v < c.n_variances; ++v) {
        const std::string p = std::string("variance_adaptor.encoders.") + c.var_names[v];
        e->w.expect(p + ".bins", {c.var_nbins - 1});
        e->w.expect(p + ".embedding.weight", {c.var_nbins, H});
        predictor_spec(e, p + ".predictor", c.var_nlayers[v], H, c.var_filter, c.var_kernel[v], c.var_depthwise, c.var_cwt[v] ? 10 : 1);
        if (c.var_cwt[v]) {
            e->w.expect(p + ".mean_std_linear.weight", {2, c.var_filter});
            e->w.expect(p + ".mean_std_linear.bias", {2});
        }
    }
    e->w.expect("linear.weight", {c.n_mels, H});
    e->w.expect("linear.bias", {c.n_mels});
    e->w.expect("speaker_embedding.projection.weight", {H, c.dvec_dim});
    e->w.expect("speaker_embedding.projection.bias", {H});
    for (int p = 0; p < c.n_priors; ++p) {
        const std::string q = std::string("prior_embeddings.") + c.prior_names[p];
        e->w.expect(q + ".bins", {c.var_nbins - 1});
        e->w.expect(q + ".embedding.weight", {c.var_nbins, H});
    }
}

int check_config(fs2_engine* e) {
    const fs2_config& c = e->cfg;
    if (c.abi_version != FS2_ABI_VERSION) return e->fail(FS2_ERR_ARG, "abi_version %d != %d", c.abi_version, FS2_ABI_VERSION);
    if (c.dtype != FS2_F32 && c.dtype != FS2_BF16 && c.dtype != FS2_MIXED && c.dtype != FS2_MIXED_X3 && c.dtype != FS2_F32_X3 &&
        c.dtype != FS2_MIXED_F16_X3)  // (FS2_F16 alone is a storage dtype of the operators, not an engine mode)
        return e->fail(FS2_ERR_ARG, "bad dtype");
    const int H = c.hidden;
    if (H <= 0 || H % 64 || H > 1024) return e->fail(FS2_ERR_SHAPE, "hidden=%d must be a multiple of 64, <= 1024", H);
    if (c.enc_layers < 0 || c.enc_layers > FS2_MAX_LAYERS || c.dec_layers < 0 || c.dec_layers > FS2_MAX_LAYERS)
        return e->fail(FS2_ERR_SHAPE, "layer count out of range");
    if (c.n_variances < 0 || c.n_variances > FS2_MAX_VARIANCES) return e->fail(FS2_ERR_SHAPE, "n_variances out of range");
    if (c.n_priors < 0 || c.n_priors > FS2_MAX_PRIORS) return e->fail(FS2_ERR_SHAPE, "n_priors out of range");
    if (c.n_priors && c.var_nbins < 2) return e->fail(FS2_ERR_SHAPE, "variance_nbins < 2");
    const int heads[2] = {c.enc_heads, c.dec_heads};
    for (int i = 0; i < 2; ++i) {
        if (heads[i] <= 0 || H % heads[i]) return e->fail(FS2_ERR_SHAPE, "heads must divide hidden");
        const int d = H / heads[i];
        if (d != 32 && d != 64 && d != 128) return e->fail(FS2_ERR_SHAPE, "head dim %d not in {32,64,128}", d);
    }
    const int F[2] = {c.enc_filter, c.dec_filter};
    const int dw[2] = {c.enc_depthwise, c.dec_depthwise};
    for (int i = 0; i < 2; ++i) {
        if (F[i] <= 0 || F[i] % 64) return e->fail(FS2_ERR_SHAPE, "conv_filter_size must be a multiple of 64");
        if (dw[i] && F[i] % H) return e->fail(FS2_ERR_SHAPE, "depth-wise FFN needs filter %% hidden == 0");
    }
    for (int i = 0; i < c.enc_layers; ++i)
        if (c.enc_kernels[i] < 1 || c.enc_kernels[i] > 31 || !(c.enc_kernels[i] & 1)) return e->fail(FS2_ERR_SHAPE, "encoder kernel sizes must be odd, <= 31");
    for (int i = 0; i < c.dec_layers; ++i)
        if (c.dec_kernels[i] < 1 || c.dec_kernels[i] > 31 || !(c.dec_kernels[i] & 1)) return e->fail(FS2_ERR_SHAPE, "decoder kernel sizes must be odd, <= 31");
    if (c.var_filter % 64 || c.dur_filter % 64 || c.var_filter > 1024 || c.dur_filter > 1024)
        return e->fail(FS2_ERR_SHAPE, "predictor filter sizes must be multiples of 64, <= 1024");
    if (c.dur_nlayers < 1) return e->fail(FS2_ERR_SHAPE, "duration_nlayers < 1");
    if (!(c.dur_kernel & 1) || c.dur_kernel > 31) return e->fail(FS2_ERR_SHAPE, "duration kernel must be odd, <= 31");
    for (int v = 0; v < c.n_variances; ++v) {
        if (c.var_nlayers[v] < 1) return e->fail(FS2_ERR_SHAPE, "variance_nlayers < 1");
        if (c.var_level[v] != 0 && c.var_level[v] != 1) return e->fail(FS2_ERR_ARG, "var_level must be 0 (frame) or 1 (phone)");
        if (c.var_cwt[v] && (c.var_mean[v] != 0.f || c.var_std[v] != 1.f))
            return e->fail(FS2_ERR_ARG, "a CWT variance is bucketised as it is: var_mean / var_std must be 0 / 1");
        if (c.var_nlayers[v] > 1 && c.var_filter != H) return e->fail(FS2_ERR_SHAPE, "variance_filter_size != hidden with nlayers > 1");
        if (!(c.var_kernel[v] & 1) || c.var_kernel[v] > 31) return e->fail(FS2_ERR_SHAPE, "variance kernel must be odd, <= 31");
    }
    if (c.var_nbins < 2 && c.n_variances) return e->fail(FS2_ERR_SHAPE, "variance_nbins < 2");
    if (c.n_mels <= 0 || c.n_mels % 4) return e->fail(FS2_ERR_SHAPE, "n_mels must be a positive multiple of 4");
    if (c.dvec_dim <= 0 || c.max_frames <= 0 || c.pe_len <= 0 || c.n_phones <= 0) return e->fail(FS2_ERR_ARG, "non-positive size");
    return FS2_OK;
}

// The conv + LayerNorm duration predictor chains its layers in_channels -> filter (model.py:497-501).  Judged when the first weight
// arrives, not in fs2_create: until then fs2_set_stochastic_duration may still replace that predictor by one that maps hidden -> filter itself.
int check_deterministic_duration(fs2_engine* e) {
    const fs2_config& c = e->cfg;
    if (!e->dur_stochastic && c.dur_nlayers > 1 && c.dur_filter != c.hidden)
        return e->fail(FS2_ERR_SHAPE, "duration_filter_size != hidden with nlayers > 1");
    return FS2_OK;
}

// ---- upload helpers ---------------------------------------------------------------------------
int dev_alloc(fs2_engine* e, void** p, size_t bytes) { return fs2::dev_alloc(*e, *e->dev_allocs, p, bytes, FS2_ERR_NOMEM); }
int upload_mat(fs2_engine* e, const float* h, size_t n, void** out, int dt) {
    return upload_as(*e, *e->dev_allocs, h, n, dt, out, FS2_ERR_NOMEM);
}
int upload_f32(fs2_engine* e, const float* h, size_t n, float** out) { return upload_mat(e, h, n, (void**)out, FS2_F32); }
const WeightStore::Entry& W(fs2_engine* e, const std::string& n) { return e->w.at(n); }

// conv weight (N, Cin, k) -> (N, k*Cin) tap-major
// GEMM weights of the split-arithmetic modes (FS2_F32_X3, the front of FS2_MIXED_X3): every launch of an fp32-weight layer splits each
// value into a bf16 head and tail - a constant, so it is done here, once; same bytes as fp32.  Layers the slab kernel cannot take
// (fewer than 192 output channels: the mel head, the CWT head) keep fp32 weights and the in-register split.
int upload_gemm_w(fs2_engine* e, const float* h, int N, int K, ConvW* out, int dt) {
    out->presplit = dt == FS2_F32 && e->front_split && gemm_presplit_eligible(N, K);
    if (!out->presplit) return upload_mat(e, h, (size_t)N * K, &out->w, dt);
    FS2_TRY(upload_f32(e, h, (size_t)N * K, (float**)&out->w));
    if (launch_presplit_pack((const float*)out->w, out->w, (size_t)N * K, nullptr) != FS2_OK) return e->fail(FS2_ERR_HIP, "weight split launch failed");
    FS2_HIP(e, hipStreamSynchronize(nullptr));
    return FS2_OK;
}

int make_conv(fs2_engine* e, const std::string& wname, const std::string& bname, ConvW* out, int dt) {
    out->dt = dt;
    const auto& w = W(e, wname);
    const int N = (int)w.shape[0], Cin = (int)w.shape[1], k = w.shape.size() > 2 ? (int)w.shape[2] : 1;
    std::vector<float> packed((size_t)N * Cin * k);
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < Cin; ++c)
            for (int t = 0; t < k; ++t) packed[((size_t)n * k + t) * Cin + c] = w.data[((size_t)n * Cin + c) * k + t];
    out->N = N;
    out->Cin = Cin;
    out->taps = k;
    FS2_TRY(upload_gemm_w(e, packed.data(), N, Cin * k, out, dt));
    const auto& b = W(e, bname);
    return upload_f32(e, b.data.data(), b.data.size(), &out->b);
}
int make_dw(fs2_engine* e, const std::string& wname, const std::string& bname, DwW* out) {
    const auto& w = W(e, wname);  // (C, 1, k)
    out->C = (int)w.shape[0];
    out->k = (int)w.shape[2];
    FS2_TRY(upload_f32(e, w.data.data(), w.data.size(), &out->w));
    const auto& b = W(e, bname);
    return upload_f32(e, b.data.data(), b.data.size(), &out->b);
}
// conv2 = Sequential(grouped k=1 conv (groups=H over F channels), pointwise F->H) has no
// non-linearity in between (model.py:84-93), so it is one linear map: W' = W21 * blockdiag(G),
// b' = W21 * bg + b21.  Folded once here in double precision.
int make_folded_conv2(fs2_engine* e, const std::string& p, int H, int F, ConvW* out, int dt) {
    out->dt = dt;
    const auto& G = W(e, p + ".conv2.0.weight");   // (F, F/H, 1)
    const auto& bg = W(e, p + ".conv2.0.bias");    // (F)
    const auto& W2 = W(e, p + ".conv2.1.weight");  // (H, F, 1)
    const auto& b2 = W(e, p + ".conv2.1.bias");    // (H)
    const int gs = F / H;
    std::vector<float> Wf((size_t)H * F), bf(H);
    for (int o = 0; o < H; ++o) {
        double bacc = b2.data[o];
        for (int f = 0; f < F; ++f) bacc += (double)W2.data[(size_t)o * F + f] * bg.data[f];
        bf[o] = (float)bacc;
        for (int g = 0; g < H; ++g)
            for (int j = 0; j < gs; ++j) {
                double acc = 0;
                for (int i = 0; i < gs; ++i) {
                    const int f = g * gs + i;  // output channel of the grouped conv inside group g
                    acc += (double)W2.data[(size_t)o * F + f] * G.data[(size_t)f * gs + j];
                }
                Wf[(size_t)o * F + g * gs + j] = (float)acc;
            }
    }
    out->N = H;
    out->Cin = F;
    out->taps = 1;
    FS2_TRY(upload_gemm_w(e, Wf.data(), H, F, out, dt));
    return upload_f32(e, bf.data(), bf.size(), &out->b);
}
int up_vec(fs2_engine* e, const std::string& n, float** out) {
    const auto& t = W(e, n);
    return upload_f32(e, t.data.data(), t.data.size(), out);
}
int make_layer(fs2_engine* e, const std::string& p, int H, int F, bool dw, LayerW* L, int dt) {
    L->depthwise = dw;
    FS2_TRY(make_conv(e, p + ".self_attn.in_proj_weight", p + ".self_attn.in_proj_bias", &L->in_proj, dt));
    FS2_TRY(make_conv(e, p + ".self_attn.out_proj.weight", p + ".self_attn.out_proj.bias", &L->out_proj, dt));
    FS2_TRY(up_vec(e, p + ".norm1.weight", &L->g1));
    FS2_TRY(up_vec(e, p + ".norm1.bias", &L->b1));
    FS2_TRY(up_vec(e, p + ".norm2.weight", &L->g2));
    FS2_TRY(up_vec(e, p + ".norm2.bias", &L->b2));
    if (dw) {
        FS2_TRY(make_dw(e, p + ".conv1.0.weight", p + ".conv1.0.bias", &L->dw));
        FS2_TRY(make_conv(e, p + ".conv1.1.weight", p + ".conv1.1.bias", &L->c1, dt));
        FS2_TRY(make_folded_conv2(e, p, H, F, &L->c2, dt));
    } else {
        FS2_TRY(make_conv(e, p + ".conv1.weight", p + ".conv1.bias", &L->c1, dt));
        FS2_TRY(make_conv(e, p + ".conv2.weight", p + ".conv2.bias", &L->c2, dt));
    }
    const bool is_enc = p.compare(0, 8, "encoder.") == 0;
    if (is_16bit(dt) && H == 256 && (is_enc ? e->cfg.enc_heads : e->cfg.dec_heads) == 2) {  // attn_out_ln_kernel's weight stream (a 16-bit shuffle)
        FS2_TRY(dev_alloc(e, &L->wo_pk, predictor_packed_bytes_per_layer(1)));
        FS2_TRY(launch_pack_predictor_weights(L->out_proj.w, L->wo_pk, nullptr, 1));
        FS2_HIP(e, hipStreamSynchronize(nullptr));
    }
    return FS2_OK;
}
// A Linear (weight `lw` (N, H), bias `lb`) with the LayerNorm `norm` in front of it folded in, to run on that norm's pre-norm rows:
// W' = W diag(gamma), b' = b + W beta, wg[n] = sum_k W'[n][k] of the bf16 values as stored (see LayerW::in_proj_f).  bf16 stacks of wide
// depth-wise blocks only (the blocks whose LayerNorms are deferred, conformer()): a block's in-projection behind the previous block's
// norm2, the mel head behind the last decoder block's.
int make_norm_folded(fs2_engine* e, const std::string& lw, const std::string& lb, const std::string& norm, ConvW* out, float** wg_out, int dt) {
    const auto& w = W(e, lw);
    const auto& b = W(e, lb);
    const auto& g = W(e, norm + ".weight");
    const auto& be = W(e, norm + ".bias");
    const int N = (int)w.shape[0], H = (int)w.shape[1];
    std::vector<float> wf((size_t)N * H), bf(N), wg(N);
    for (int n = 0; n < N; ++n) {
        double bacc = b.data[n], gacc = 0;
        for (int k = 0; k < H; ++k) {
            const float v = (float)((double)w.data[(size_t)n * H + k] * g.data[k]);
            wf[(size_t)n * H + k] = v;
            bacc += (double)w.data[(size_t)n * H + k] * be.data[k];
            gacc += (double)(dt == FS2_F16 ? f16_to_f32(f32_to_f16_sat(v)) : bf16_to_f32(f32_to_bf16(v)));  // of the values the MFMAs will multiply with
        }
        bf[n] = (float)bacc;
        wg[n] = (float)gacc;
    }
    out->N = N; out->Cin = H; out->taps = 1; out->dt = dt;
    FS2_TRY(upload_mat(e, wf.data(), wf.size(), &out->w, dt));
    FS2_TRY(upload_f32(e, bf.data(), bf.size(), &out->b));
    return upload_f32(e, wg.data(), wg.size(), wg_out);
}

// The single-launch predictors read one stacked vector each of every layer's conv bias (`bias_name` within the layer) and LayerNorm
// gamma / beta.
int upload_stacked_vectors(fs2_engine* e, const std::string& p, int nl, const char* bias_name, PredictorW* P) {
    std::vector<float> bias, g, b;
    for (int j = 0; j < nl; ++j) {
        const std::string q = p + ".layers." + std::to_string(j) + ".layers";
        const auto &hb = W(e, q + bias_name).data, &hg = W(e, q + ".2.weight").data, &hbe = W(e, q + ".2.bias").data;
        bias.insert(bias.end(), hb.begin(), hb.end());
        g.insert(g.end(), hg.begin(), hg.end());
        b.insert(b.end(), hbe.begin(), hbe.end());
    }
    FS2_TRY(upload_f32(e, bias.data(), bias.size(), &P->bias_all));
    FS2_TRY(upload_f32(e, g.data(), g.size(), &P->g_all));
    return upload_f32(e, b.data(), b.size(), &P->b_all);
}

int make_predictor(fs2_engine* e, const std::string& p, int nl, int filt, bool dw, PredictorW* P, int dt, bool cwt = false) {
    P->filt = filt;
    P->dt = dt;
    P->cwt = cwt;
    P->layers.resize(nl);
    for (int j = 0; j < nl; ++j) {
        const std::string q = p + ".layers." + std::to_string(j) + ".layers";
        PredLayerW& Lw = P->layers[j];
        Lw.depthwise = dw;
        if (dw) {
            FS2_TRY(make_dw(e, q + ".0.module.0.weight", q + ".0.module.0.bias", &Lw.dw));
            FS2_TRY(make_conv(e, q + ".0.module.1.weight", q + ".0.module.1.bias", &Lw.c, dt));
        } else {
            FS2_TRY(make_conv(e, q + ".0.module.weight", q + ".0.module.bias", &Lw.c, dt));
        }
        FS2_TRY(up_vec(e, q + ".2.weight", &Lw.g));
        FS2_TRY(up_vec(e, q + ".2.bias", &Lw.b));
    }
    if (cwt) {  // Linear(filter, 10): a small GEMM (rows padded to 12 for 16-byte fp32 stores)
        const auto& hw = W(e, p + ".linear.weight");
        const auto& hb = W(e, p + ".linear.bias");
        std::vector<float> wp((size_t)12 * filt, 0.f), bp(12, 0.f);
        memcpy(wp.data(), hw.data.data(), (size_t)10 * filt * 4);
        memcpy(bp.data(), hb.data.data(), 10 * 4);
        P->head_mat.N = 12; P->head_mat.Cin = filt; P->head_mat.taps = 1; P->head_mat.dt = dt;
        FS2_TRY(upload_mat(e, wp.data(), wp.size(), &P->head_mat.w, dt));
        FS2_TRY(upload_f32(e, bp.data(), bp.size(), &P->head_mat.b));
        return FS2_OK;  // never the single-launch kernel: its head is the scalar one
    }
    FS2_TRY(up_vec(e, p + ".linear.weight", &P->head_w));
    P->head_b = W(e, p + ".linear.bias").data[0];
    if (dw && nl && filt > 256) {
        const std::string q = p + ".layers." + std::to_string(nl - 1) + ".layers";
        const auto &hw = W(e, p + ".linear.weight").data, &hg = W(e, q + ".2.weight").data, &hbe = W(e, q + ".2.bias").data;
        std::vector<float> gw(filt);
        double sg = 0, cst = P->head_b;
        for (int n = 0; n < filt; ++n) {
            gw[n] = hg[n] * hw[n];
            sg += (double)gw[n];
            cst += (double)hbe[n] * hw[n];
        }
        FS2_TRY(upload_f32(e, gw.data(), gw.size(), &P->head_gw));
        P->head_sum_gw = (float)sg;
        P->head_cst = (float)cst;
    }
    const int taps = nl ? P->layers[0].c.taps : 0, cin = nl ? P->layers[0].c.Cin : 0;
    if (!dw && nl && cin == filt && predictor_fused_supported(dt, filt, taps, nl, 1)) {
        const size_t lb = predictor_packed_bytes_per_layer();
        FS2_TRY(dev_alloc(e, &P->wpk, lb * nl));
        for (int j = 0; j < nl; ++j) FS2_TRY(launch_pack_predictor_weights(P->layers[j].c.w, (char*)P->wpk + lb * j, nullptr));
        FS2_HIP(e, hipStreamSynchronize(nullptr));
        FS2_TRY(upload_stacked_vectors(e, p, nl, ".0.module.bias", P));
    } else if (dw && nl && cin == filt && P->layers[0].dw.k == 3 && P->layers[0].dw.C == filt && predictor_fused_supported(dt, filt, 3, nl, 1)) {
        // depth-wise layers in the single launch (predictor_fused_kernel<..., DW>): the pointwise weights in fragment order (one tap),
        // the depth-wise taps as (layer, tap, channel) fp32
        const size_t lb = predictor_packed_bytes_per_layer(1);
        FS2_TRY(dev_alloc(e, &P->wpk, lb * nl));
        std::vector<float> dww((size_t)nl * 3 * filt), dwb;
        for (int j = 0; j < nl; ++j) {
            const std::string q = p + ".layers." + std::to_string(j) + ".layers";
            FS2_TRY(launch_pack_predictor_weights(P->layers[j].c.w, (char*)P->wpk + lb * j, nullptr, 1));
            const auto &hw = W(e, q + ".0.module.0.weight").data, &hdb = W(e, q + ".0.module.0.bias").data;  // (filt, 1, 3), (filt)
            for (int c2 = 0; c2 < filt; ++c2)
                for (int t = 0; t < 3; ++t) dww[((size_t)j * 3 + t) * filt + c2] = hw[(size_t)c2 * 3 + t];
            dwb.insert(dwb.end(), hdb.begin(), hdb.end());
        }
        FS2_HIP(e, hipStreamSynchronize(nullptr));
        FS2_TRY(upload_stacked_vectors(e, p, nl, ".0.module.1.bias", P));
        FS2_TRY(upload_f32(e, dww.data(), dww.size(), &P->dw_all));
        FS2_TRY(upload_f32(e, dwb.data(), dwb.size(), &P->dwb_all));
    } else if (!dw && nl && cin == filt && dt == FS2_F32 && e->front_split && predictor_fused_x3_supported(filt, taps, nl, 1)) {
        // the same launch in the split arithmetic: the weights' bf16 heads and tails in the kernel's fragment order
        // [layer][step = tap * 8 + kb][32-channel group][2][lane] x 8 values (pack_predictor_weights_kernel's map), packed here
        const size_t per = predictor_packed_bytes_per_layer() / 2;  // bf16 values per layer
        std::vector<unsigned short> hi(per * nl), lo(per * nl);
        for (int j = 0; j < nl; ++j) {
            const std::string q = p + ".layers." + std::to_string(j) + ".layers";
            const auto& w = W(e, q + ".0.module.weight");  // (filt, filt, 3)
            for (int step = 0; step < 24; ++step) {
                const int tap = step / 8, kb = step % 8;
                for (int grp = 0; grp < 8; ++grp)
                    for (int ni = 0; ni < 2; ++ni)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int fr = lane & 15, fg = lane >> 4;
                            const int ch = grp * 32 + (fr >> 2) * 8 + ni * 4 + (fr & 3);
                            const size_t o = (size_t)j * per + ((((size_t)step * 8 + grp) * 2 + ni) * 64 + lane) * 8;
                            for (int k8 = 0; k8 < 8; ++k8) {
                                const int c = kb * 32 + fg * 8 + k8;
                                const float v = w.data[((size_t)ch * filt + c) * 3 + tap];
                                const bf16 h = f32_to_bf16(v);
                                hi[o + k8] = h.v;
                                lo[o + k8] = f32_to_bf16(v - bf16_to_f32(h)).v;
                            }
                        }
            }
        }
        FS2_TRY(dev_alloc(e, &P->wpk, hi.size() * 2));
        FS2_TRY(dev_alloc(e, &P->wpk_lo, lo.size() * 2));
        FS2_HIP(e, hipMemcpy(P->wpk, hi.data(), hi.size() * 2, hipMemcpyHostToDevice));
        FS2_HIP(e, hipMemcpy(P->wpk_lo, lo.data(), lo.size() * 2, hipMemcpyHostToDevice));
        FS2_TRY(upload_stacked_vectors(e, p, nl, ".0.module.bias", P));
    }
    return FS2_OK;
}

// ---- profiling brackets -----------------------------------------------------------------------
struct Bracket {
    fs2_engine* e;
    int cls;
    hipStream_t st;
    hipEvent_t stop = nullptr;
    Bracket(fs2_engine* e_, int cls_, hipStream_t st_, double flops, double bytes, bool active = true)
        : e(e_), cls(cls_), st(st_) {
        ProfSlot& s = e->prof[cls];
        if (!active || !s.enabled) return;
        if (s.used == s.ev.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            s.ev.emplace_back(a, b);
        }
        (void)hipEventRecord(s.ev[s.used].first, st);
        stop = s.ev[s.used].second;
        s.used++;
        s.flops += flops;
        s.bytes += bytes;
    }
    ~Bracket() {
        if (stop) (void)hipEventRecord(stop, st);
    }
};

// ---- op wrappers used by the forward ------------------------------------------------------------
struct Deferred {  // deferred-LayerNorm epilogue of a GEMM (rows wider than one 256-column tile; see GemmArgs)
    const void* res = nullptr;        // residual added to the output ...
    const float* res_stats = nullptr; // ... itself a pre-norm tensor if set: normalised on load with res_g / res_b
    const float* res_g = nullptr;
    const float* res_b = nullptr;
    float* stats_out = nullptr;       // (M, parts) float2
    // the consumer is LayerNorm -> Linear(N, 1): leave sum_n v[n] head_gw[n] per row and column tile in head_out (M, parts) instead of
    // the rows, where the launch can (gemm_head_supported; *head_done says whether it did - if not, the rows were stored as usual)
    const float* head_gw = nullptr;
    float* head_out = nullptr;
    bool* head_done = nullptr;
};
inline int ln_parts(int N) { return (N + 255) / 256; }  // one (sum, sum of squares) per row per 256-column GEMM tile, <= 4

struct LnFuse {  // optional fused epilogue: y = LN(act(gemm) [+ res]) [-> head]
    const void* res = nullptr;
    const float* g = nullptr;
    const float* b = nullptr;
    const float* dot_w = nullptr;
    float dot_b = 0.f;
    const uint8_t* mask = nullptr;
    float* pred = nullptr;
    void* tmp = nullptr;  // (M, N) scratch for the unfused fallback
};

struct RowScale {  // x of the GEMM is a pre-norm tensor whose LayerNorm is folded into w (GemmArgs::rs_stats)
    const float* rowstats;  // (M) float2 (rstd, rstd * mean): launch_rowstats_finish
    const float* wg;
};
// What a gemm() may ask for beyond y = act(x w^T + b).  A call site names the fields it sets, in declaration order: {.ln = &ln}
// (designated initialisers: C++20, which hipcc's clang also takes in its C++17 mode, silently unless -pedantic)
struct GemmOpt {
    const LnFuse* ln = nullptr;
    int extra_class = -1;               // a second profiling class the launch is timed under
    const uint8_t* zero_rows = nullptr; // rows whose mask byte is set are stored as 0
    const Deferred* deferred = nullptr;
    void* c_lo = nullptr;               // the fp32 result stored as bf16 head (c) + tail (c_lo): the split attention's input
    const RowScale* rowscale = nullptr;
};
int gemm(fs2_engine* e, hipStream_t st, const ConvW& w, const void* x, void* c, int M, int S, bool relu, int out_dt, const GemmOpt& o = {}) {
    const LnFuse* ln = o.ln;
    const Deferred* df = o.deferred;
    const RowScale* rs = o.rowscale;
    GemmArgs a;
    a.tune = &e->tune;
    a.zero_rows = o.zero_rows;
    a.C_lo = o.c_lo;
    if (rs) { a.rs_stats = rs->rowstats; a.rs_wg = rs->wg; }
    if (df) {
        a.epi_res = df->res; a.epi_res_stats = df->res_stats; a.epi_res_g = df->res_g; a.epi_res_b = df->res_b;
        a.epi_res_parts = ln_parts(w.N); a.stats_out = df->stats_out; a.ln_eps = 1e-5f;
    }
    a.split = e->front_split && w.dt == FS2_F32;
    a.w_presplit = w.presplit;
    a.X = x;
    a.W = w.w;
    a.bias = w.b;
    a.C = c;
    a.M = M;
    a.N = w.N;
    a.K = w.taps * w.Cin;
    a.ldx = w.Cin;
    a.ldc = w.N;
    a.Cin = w.Cin;
    a.taps = w.taps;
    a.pad = (w.taps - 1) / 2;
    a.S = S;
    a.relu = relu;
    if (ln) {
        a.res = ln->res; a.ln_g = ln->g; a.ln_b = ln->b; a.ln_eps = 1e-5f;
        a.dot_w = ln->dot_w; a.dot_b = ln->dot_b; a.mask = ln->mask; a.pred = ln->pred; a.ln_tmp = ln->tmp;
    }
    if (df && df->head_out && df->head_done) {
        a.head_gw = df->head_gw; a.head_out = df->head_out;
        *df->head_done = gemm_head_supported(a, w.dt, out_dt);
        if (!*df->head_done) { a.head_gw = nullptr; a.head_out = nullptr; }
    }
    const double osz = (double)elem_bytes(out_dt);
    const double fl = 2.0 * M * (double)a.N * a.K;
    const double wsz = (double)elem_bytes(w.dt);
    const double by = (double)M * w.Cin * wsz + (double)a.N * a.K * wsz + (double)M * a.N * osz;
    Bracket br(e, w.taps > 1 ? FS2_K_CONV_GEMM : FS2_K_GEMM, st, fl, by);
    Bracket br2(e, o.extra_class >= 0 ? o.extra_class : FS2_K_COUNT - 1, st, fl, by, o.extra_class >= 0);
    const int r = launch_gemm(a, w.dt, out_dt, st);
    if (r != FS2_OK) return e->fail(r, "gemm launch failed (M=%d N=%d K=%d)", M, a.N, a.K);
    return FS2_OK;
}
struct LnOnLoad { const float* stats; const float* g; const float* b; };  // x of a dwconv is a pre-norm tensor

int dwconv(fs2_engine* e, hipStream_t st, const DwW& w, const void* x, void* y, int B, int S, int dt,
           const LnOnLoad* ln = nullptr) {
    DwConvArgs a;
    if (ln) { a.ln_stats = ln->stats; a.ln_g = ln->g; a.ln_b = ln->b; a.ln_parts = ln_parts(w.C); }
    a.x = x; a.w = w.w; a.bias = w.b; a.y = y;
    a.B = B; a.S = S; a.C = w.C; a.k = w.k; a.pad = (w.k - 1) / 2;
    Bracket br(e, FS2_K_ROWOPS, st, 2.0 * B * S * (double)w.C * w.k, 2.0 * B * S * (double)w.C * (double)elem_bytes(dt));
    const int r = launch_dwconv(a, dt, st);
    if (r != FS2_OK) return e->fail(r, "dwconv launch failed");
    return FS2_OK;
}

int norm_only(fs2_engine* e, hipStream_t st, int dt, const void* v, const float* stats, const float* g, const float* b, void* y,
              int M, int H, const float* dot_w = nullptr, float dot_b = 0.f, const uint8_t* mask = nullptr, float* pred = nullptr) {
    LayerNormArgs l;
    l.pre_stats = stats; l.pre_parts = ln_parts(H);
    l.x = v; l.res = nullptr; l.gamma = g; l.beta = b; l.y = y;
    l.dot_w = dot_w; l.dot_b = dot_b; l.mask = mask; l.pred = pred;
    l.M = M; l.H = H; l.eps = 1e-5f;
    Bracket br(e, FS2_K_ROWOPS, st, 0, 2.0 * M * (double)H * (double)elem_bytes(dt));
    if (launch_layernorm(l, dt, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "normalise-only LayerNorm launch failed");
    return FS2_OK;
}

struct LayerScratch {
    float *st1, *st2;  // deferred-LayerNorm row statistics (M, ln_parts(max width)) float2 each
    float* rsf;        // (M) float2 (rstd, rstd * mean) of a block's pre-norm output (folded LayerNorm)
    float* hd;         // (M, 4) head sums of a predictor's last GEMM (GemmArgs::head_out)
    void *qkv, *att, *proj, *hid, *u, *vt;
    uint64_t* bits;
    int Spad, nw64;
};

// ConformerEncoderLayer.forward, post-LN (model.py:113-115); result back in x (tmp is the other
// half of the ping-pong pair).
// prenorm_in (wide depth-wise bf16 stacks, fs2_set_folded_layernorm): x holds the PREVIOUS block's pre-norm output v2 (its row
// statistics in sc.st2, its norm2 in pg / pb) - this block's in-projection and residual normalise it on the fly; leave_prenorm:
// this block in turn skips its closing normalise-only pass and leaves v2 + statistics for the next one.
int conformer(fs2_engine* e, hipStream_t st, const LayerW& w, void* x, void* tmp, int B, int S, int heads,
              const LayerScratch& sc, bool is_decoder, bool prenorm_in = false, const float* pg = nullptr, const float* pb = nullptr,
              bool leave_prenorm = false) {
    const int H = e->cfg.hidden, M = B * S, dt = w.in_proj.dt;
    const double dsz = (double)elem_bytes(dt);
    // fp32 storage with the bf16 x 3 split products (FS2_F32_X3 / the front of FS2_MIXED_X3): the attention takes the split
    // arithmetic too - the in-projection stores its fp32 result as bf16 head + tail (the same bytes, no extra pass), the attention
    // multiplies them with three bf16 MFMAs per product and hands back fp32 rows (attention.hip, X3)
    // the encoder's whole self-attention block as one timed class (in-projection .. out-projection + LayerNorm): 8 S H^2 + 4 S^2 H flops
    // per utterance (SURVEY 8d's fused-MHA figure), bytes: x in + out, the three weight matrices
    std::optional<Bracket> mha;  // closed behind the out-projection (reset()), or by an error return
    if (!is_decoder) mha.emplace(e, FS2_K_ENC_MHA, st, 8.0 * M * (double)H * H + 4.0 * B * (double)S * S * H, 2.0 * M * H * dsz + 4.0 * H * H * dsz);
    const bool x3 = e->front_split && dt == FS2_F32 && e->tune.attn_x3;
    void* qkv_lo = x3 ? (void*)((char*)sc.qkv + (size_t)M * 3 * H * 2) : nullptr;
    if (prenorm_in) {
        if (!w.has_fold || !(w.depthwise && H > 256 && e->defer_ln)) return e->fail(FS2_ERR_STATE, "pre-norm block input without folded weights");
        const RowScale rs{sc.rsf, w.in_wg};
        FS2_TRY(gemm(e, st, w.in_proj_f, x, sc.qkv, M, M, false, dt, {.rowscale = &rs}));
    } else {
        FS2_TRY(gemm(e, st, w.in_proj, x, sc.qkv, M, M, false, dt, {.c_lo = qkv_lo}));
    }
    const int ffn_class = is_decoder ? FS2_K_DEC_FFN_CONV1 : -1;
    // the block's second half on tmp = LN1(x + out_proj(att)): x = LN2(tmp + conv2(relu(conv1([dwconv] tmp))))
    const auto ffn = [&]() -> int {
        const void* in = tmp;
        if (w.depthwise) {
            FS2_TRY(dwconv(e, st, w.dw, tmp, sc.u, B, S, dt));
            in = sc.u;
        }
        FS2_TRY(gemm(e, st, w.c1, in, sc.hid, M, S, true, dt, {.extra_class = ffn_class}));
        LnFuse ln;
        ln.res = tmp; ln.g = w.g2; ln.b = w.b2; ln.tmp = sc.proj;
        return gemm(e, st, w.c2, sc.hid, x, M, S, false, dt, {.ln = &ln});
    };
    AttnArgs a;
    a.tune = &e->tune;
    a.qkv_lo = qkv_lo;
    a.qkv = sc.qkv; a.vt = sc.vt; a.kbits = sc.bits; a.out = sc.att;
    a.B = B; a.S = S; a.H = H; a.heads = heads; a.Spad = sc.Spad; a.nw64 = sc.nw64;
    a.scale_log2e = (float)(1.4426950408889634 / sqrt((double)(H / heads)));
    // (by the utterance length only, never by the batch: a shard alone must take the kernels its rows take inside the whole batch.  Measured,
    //  tools/bench_ops.py encmha at B = 32: 256 rows 13.7 us against 10.7 + 14.8, 384: 23.8 vs 30.6, 512: 28.4 vs 36.1, 768: 47.7 vs 50.6, 1000:
    //  59.6 vs 53.5 - the 64-query workgroups re-read K / V twice as often as the 128-query ones of the stand-alone kernel; from 1024 rows on the
    //  pipelined attention kernel takes over anyway)
    if (w.wo_pk && S <= 768 && e->tune.enc_attn_out && !x3 && !prenorm_in && attn_out_ln_supported(dt, H, heads, S) &&
        !(w.depthwise && H > 256 && e->defer_ln)) {
        // r06: attention (both heads) + out-projection + residual + norm1 in ONE launch: tmp = LN1(x + out_proj(attention(qkv)))
        AttnOutArgs ao;
        ao.qkv = sc.qkv; ao.kbits = sc.bits; ao.wpk = w.wo_pk; ao.bias = w.out_proj.b; ao.res = x; ao.ln_g = w.g1; ao.ln_b = w.b1; ao.out = tmp;
        ao.B = B; ao.S = S; ao.H = H; ao.heads = heads; ao.nw64 = sc.nw64; ao.scale_log2e = a.scale_log2e; ao.eps = 1e-5f;
        {
            Bracket br(e, FS2_K_ATTENTION, st, 4.0 * B * (double)S * S * H + 2.0 * M * (double)H * H, 5.0 * M * H * dsz + (double)H * H * dsz);
            const int r = launch_attn_out_ln(ao, dt, st);
            if (r != FS2_OK) return e->fail(r, "fused attention + out-projection launch failed");
        }
        mha.reset();
        return ffn();
    }
    {
        Bracket br(e, FS2_K_ROWOPS, st, 0, 2.0 * M * H * dsz);
        const int r = x3 ? FS2_OK : launch_transpose_v(a, dt, st);  // (the split form reads V row-major, like the bf16 one)
        if (r != FS2_OK) return e->fail(r, "transpose_v launch failed");
    }
    {
        Bracket br(e, FS2_K_ATTENTION, st, 4.0 * B * (double)S * S * H, 4.0 * M * H * dsz);
        Bracket br2(e, FS2_K_DEC_ATTENTION, st, 4.0 * B * (double)S * S * H, 4.0 * M * H * dsz, is_decoder);
        const int r = launch_attention(a, dt, st);
        if (r != FS2_OK) return e->fail(r, "attention launch failed");
    }
    if (w.depthwise && H > 256 && e->defer_ln) {
        // Rows wider than one GEMM tile cannot have LayerNorm fused behind the GEMM, and in the depth-wise block every
        // consumer of LN1's output is a row operation.  So LN1 is never materialised: the out-projection's epilogue
        // leaves v1 = x + out_proj(att) and its row statistics, the depth-wise conv normalises v1 as it loads it, and
        // conv2's epilogue normalises v1 once more for the residual; LN2 is a normalise-only pass over conv2's output.
        Deferred d1;
        d1.res = x; d1.stats_out = sc.st1;
        if (prenorm_in) { d1.res_stats = sc.st2; d1.res_g = pg; d1.res_b = pb; }                      // x = LN2_prev(v2_prev), on load
        FS2_TRY(gemm(e, st, w.out_proj, sc.att, tmp, M, M, false, dt, {.deferred = &d1}));               // tmp = v1
        mha.reset();
        LnOnLoad l1{sc.st1, w.g1, w.b1};
        FS2_TRY(dwconv(e, st, w.dw, tmp, sc.u, B, S, dt, &l1));
        FS2_TRY(gemm(e, st, w.c1, sc.u, sc.hid, M, S, true, dt, {.extra_class = ffn_class}));
        Deferred d2;
        d2.res = tmp; d2.res_stats = sc.st1; d2.res_g = w.g1; d2.res_b = w.b1; d2.stats_out = sc.st2;
        FS2_TRY(gemm(e, st, w.c2, sc.hid, x, M, S, false, dt, {.deferred = &d2}));                        // x = v2 (x is free by now)
        if (leave_prenorm) {  // the next block folds LN2 in: its in-projection wants (rstd, rstd * mean) per row
            if (launch_rowstats_finish(sc.st2, ln_parts(H), H, 1e-5f, sc.rsf, M, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "row statistics launch failed");
            return FS2_OK;
        }
        return norm_only(e, st, dt, x, sc.st2, w.g2, w.b2, x, M, H);                                   // x = LN2(v2), in place
    }
    {   // tmp = LN1(x + out_proj(att))
        LnFuse ln;
        ln.res = x; ln.g = w.g1; ln.b = w.b1; ln.tmp = sc.proj;
        FS2_TRY(gemm(e, st, w.out_proj, sc.att, tmp, M, M, false, dt, {.ln = &ln}));
        mha.reset();
    }
    return ffn();
}

// The torch-1.10 container loop (fastspeech2.py:249-262: for layer in layers: x = layer(x, ...), no final norm).  Between two wide
// depth-wise bf16 blocks the closing LayerNorm is never materialised (fs2_set_folded_layernorm): block i leaves v2 + row statistics,
// block i + 1 runs its in-projection on v2 with norm2 folded into the weights and normalises the residual on load.
int run_stack(fs2_engine* e, hipStream_t st, const std::vector<LayerW>& Ls, void* x, void* tmp, int B, int S, int heads,
              const LayerScratch& sc, bool is_decoder, bool leave_last = false, bool* left = nullptr) {
    const int H = e->cfg.hidden;
    bool pre = false;
    for (size_t i = 0; i < Ls.size(); ++i) {
        const LayerW& w = Ls[i];
        const bool deferred = w.depthwise && H > 256 && e->defer_ln;
        const bool leave = e->fold_ln && deferred && (i + 1 < Ls.size() ? Ls[i + 1].has_fold && Ls[i + 1].depthwise : leave_last);
        FS2_TRY(conformer(e, st, w, x, tmp, B, S, heads, sc, is_decoder, pre, pre ? Ls[i - 1].g2 : nullptr, pre ? Ls[i - 1].b2 : nullptr, leave));
        pre = leave;
    }
    if (left) *left = pre;  // the stack's output is the last block's pre-norm v2 (+ finished statistics in sc.rsf): the caller folds norm2 in
    return FS2_OK;
}

// VariancePredictor.forward (model.py:510-522): pred (B*S) fp32, 0 where mask
struct CwtOut {  // where the CWT head's by-products go (scratch or the caller's buffers)
    float* spec12 = nullptr;    // (M, 12) scratch
    float* mean_std = nullptr;  // (B, 2)
    float* spec_out = nullptr;  // (B, S, 10) or null
};

struct EmbedTail {  // the VarianceEncoder's bucketize + embedding add (+ pe + spk) as the tail of the predictor launch (predictor_fused.hip)
    void* y;
    const float* bins;
    const float* emb;
    int nbins;
    float std, mean;
    const float* pe;
    const float* spk;
};

// The CWT ending on the last layer's activations (model.py:412-431): 10-scale head, utterance-level mean / std, recomposition
int cwt_head(fs2_engine* e, hipStream_t st, const PredictorW& P, const void* act, const CwtOut& cw, const uint8_t* mask, float* pred, int B, int S) {
    FS2_TRY(gemm(e, st, P.head_mat, act, cw.spec12, B * S, B * S, false, FS2_F32));
    CwtArgs ca{act, cw.spec12, 12, mask, P.ms_w, P.ms_b, cw.mean_std, pred, cw.spec_out, B, S, P.filt};
    if (launch_cwt_head(ca, P.dt, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "cwt head launch failed");
    return FS2_OK;
}

int predictor(fs2_engine* e, hipStream_t st, const PredictorW& P, const void* x, int B, int S, const uint8_t* mask,
              float* pred, const LayerScratch& sc, const CwtOut* cw = nullptr, const EmbedTail* tail = nullptr, bool* tail_done = nullptr) {
    const int M = B * S;
    if (tail_done) *tail_done = false;
    if (P.cwt && !cw) return e->fail(FS2_ERR_STATE, "CWT predictor without its output buffers");
    // the whole predictor as one launch (predictor_fused.hip): in the split arithmetic (fp32 rows in, and out of the embedding tail), or in bf16
    const int nl = (int)P.layers.size(), taps = P.dw_all ? 3 : P.layers[0].c.taps;
    const bool one_x3 = P.wpk && P.wpk_lo && e->fuse_predictor && P.dt == FS2_F32 && e->front_split && predictor_fused_x3_supported(P.filt, taps, nl, S);
    if (one_x3 || (P.wpk && !P.wpk_lo && e->fuse_predictor && predictor_fused_supported(P.dt, P.filt, taps, nl, S))) {
        PredictorArgs a;
        a.x = x; a.wpk = P.wpk; a.wpk_lo = P.wpk_lo; a.bias = P.bias_all; a.ln_g = P.g_all; a.ln_b = P.b_all;
        a.dw_w = P.dw_all; a.dw_b = P.dwb_all;  // depth-wise layers: wpk = their pointwise halves
        a.head_w = P.head_w; a.head_b = P.head_b; a.mask = mask; a.pred = pred;
        a.B = B; a.S = S; a.H = P.filt; a.nlayers = nl; a.taps = taps; a.eps = 1e-5f;
        const bool with_tail = tail && tail_done && !P.cwt && tail->y != x && tail->nbins >= 2 && tail->nbins - 1 <= 512;
        if (with_tail) {
            a.be_y = tail->y; a.be_bins = tail->bins; a.be_emb = tail->emb; a.be_nbins = tail->nbins;
            a.be_std = tail->std; a.be_mean = tail->mean; a.be_pe = tail->pe; a.be_spk = tail->spk;
        }
        const double rsz = one_x3 ? 4 : 2;  // bytes per element of a row
        const double fl = (P.dw_all ? 2.0 * M * (double)P.filt * (P.filt + 3) : 2.0 * M * (double)P.filt * P.filt * taps) * nl;
        const double by = (double)M * P.filt * rsz + (double)M * 4 + (with_tail ? 2.0 * M * P.filt * rsz : 0.0);
        Bracket br(e, FS2_K_CONV_GEMM, st, fl, by);
        Bracket brp(e, FS2_K_PREDICTOR, st, fl, by, x != e->ps.xA && x != e->ps.xB);
        const int r = one_x3 ? launch_predictor_fused_x3(a, st) : launch_predictor_fused(a, st);
        if (r != FS2_OK) return e->fail(r, "fused predictor%s launch failed (B=%d S=%d)", one_x3 ? " (split arithmetic)" : "", B, S);
        if (with_tail) *tail_done = true;
        return FS2_OK;
    }
    if (P.layers[0].depthwise && P.filt > 256 && e->defer_ln) {
        // depth-wise predictor, wide rows: [dw conv -> pointwise GEMM -> ReLU] leaves the pre-norm activations + row
        // statistics; the NEXT layer's depth-wise conv normalises on load, the last layer's LayerNorm + head is a
        // normalise-only pass that stores nothing but the prediction (or the activations, for the CWT head)
        const void* src = x;
        float* stats[2] = {sc.st1, sc.st2};
        const PredLayerW* prev = nullptr;
        bool head_done = false;
        for (size_t j = 0; j < P.layers.size(); ++j) {
            const PredLayerW& Lw = P.layers[j];
            void* out = (j & 1) ? sc.proj : sc.att;
            LnOnLoad lp{stats[(j + 1) & 1], prev ? prev->g : nullptr, prev ? prev->b : nullptr};
            FS2_TRY(dwconv(e, st, Lw.dw, src, sc.u, B, S, P.dt, prev ? &lp : nullptr));
            Deferred d;
            d.stats_out = stats[j & 1];
            if (j + 1 == P.layers.size() && !P.cwt && P.head_gw) { d.head_gw = P.head_gw; d.head_out = sc.hd; d.head_done = &head_done; }
            FS2_TRY(gemm(e, st, Lw.c, sc.u, out, M, S, true, P.dt, {.deferred = &d}));
            src = out;
            prev = &Lw;
        }
        float* stl = stats[(P.layers.size() - 1) & 1];
        if (head_done) {  // the last LayerNorm + head: a row-sized pass over the epilogue's sums
            Bracket br(e, FS2_K_ROWOPS, st, 0, (double)M * ln_parts(P.filt) * 12);
            if (launch_head_finish(stl, sc.hd, ln_parts(P.filt), P.filt, 1e-5f, P.head_sum_gw, P.head_cst, mask, pred, M, st) != FS2_OK)
                return e->fail(FS2_ERR_HIP, "head finish launch failed");
            return FS2_OK;
        }
        if (!P.cwt) return norm_only(e, st, P.dt, src, stl, prev->g, prev->b, nullptr, M, P.filt, P.head_w, P.head_b, mask, pred);
        FS2_TRY(norm_only(e, st, P.dt, src, stl, prev->g, prev->b, (void*)src, M, P.filt));
        return cwt_head(e, st, P, src, *cw, mask, pred, B, S);
    }
    const void* src = x;
    for (size_t j = 0; j < P.layers.size(); ++j) {
        const PredLayerW& Lw = P.layers[j];
        const bool last = j + 1 == P.layers.size();
        // conv -> ReLU -> LayerNorm fused in the GEMM epilogue; the last layer also applies the
        // Linear(filter, 1) head + mask and never stores its activations.  Outputs ping-pong
        // between att and proj (a conv must not write the buffer it reads neighbours from).
        void* out = (j & 1) ? sc.proj : sc.att;
        void* other = (j & 1) ? sc.att : sc.proj;
        LnFuse ln;
        ln.g = Lw.g; ln.b = Lw.b;
        const bool keep = !last || P.cwt;  // the CWT head needs the last layer's activations themselves
        if (last && !P.cwt) { ln.dot_w = P.head_w; ln.dot_b = P.head_b; ln.mask = mask; ln.pred = pred; }
        if (Lw.depthwise) {
            FS2_TRY(dwconv(e, st, Lw.dw, src, sc.u, B, S, P.dt));
            ln.tmp = other;  // src (= other for j > 0) is dead once the depth-wise conv has run
            FS2_TRY(gemm(e, st, Lw.c, sc.u, keep ? out : nullptr, M, S, true, P.dt, {.ln = &ln}));
        } else {
            ln.tmp = sc.u;
            FS2_TRY(gemm(e, st, Lw.c, src, keep ? out : nullptr, M, S, true, P.dt, {.ln = &ln}));
        }
        src = out;
    }
    return P.cwt ? cwt_head(e, st, P, src, *cw, mask, pred, B, S) : FS2_OK;
}

// ---- workspace layout ---------------------------------------------------------------------------
// One function per region (persist; the scratch of the encode and of the decode phase, each ending in / holding a stack's layer
// scratch) takes the region's buffers from an arena, in a fixed order, and says whether they all fit.  The SIZE of a region is the same
// function run on an arena that only counts (the *_need functions): a new buffer is one take() here and nothing else.
bool layout_layer_scratch(const fs2_engine* e, Arena& ar, int B, int S, LayerScratch* sc) {
    const fs2_config& c = e->cfg;
    const size_t H = c.hidden, M = (size_t)B * S, esz = e->esz;
    size_t Fm = c.enc_filter > c.dec_filter ? c.enc_filter : c.dec_filter;
    size_t Pm = H;
    if ((size_t)c.var_filter > Pm) Pm = c.var_filter;
    if ((size_t)c.dur_filter > Pm) Pm = c.dur_filter;
    sc->Spad = (S + 63) / 64 * 64;
    sc->nw64 = sc->Spad / 64;
    sc->st1 = (float*)ar.take(M * (size_t)ln_parts((int)Pm) * 8);
    sc->st2 = (float*)ar.take(M * (size_t)ln_parts((int)Pm) * 8);
    sc->rsf = (float*)ar.take(M * 8);
    sc->hd = (float*)ar.take(M * 16);
    sc->qkv = ar.take(M * 3 * H * esz);
    sc->att = ar.take(M * Pm * esz);
    sc->proj = ar.take(M * Pm * esz);
    sc->hid = ar.take(M * Fm * esz);
    sc->u = ar.take(M * Pm * esz);
    sc->vt = ar.take((size_t)B * H * sc->Spad * esz);
    sc->bits = (uint64_t*)ar.take((size_t)B * sc->nw64 * 8);
    return !ar.overflow;
}

bool layout_persist(const fs2_engine* e, Arena& ar, int B, int L, PersistBufs* p) {
    const fs2_config& c = e->cfg;
    const size_t H = c.hidden, ML = (size_t)B * L, esz = e->esz;
    p->spk = (float*)ar.take((size_t)B * H * 4);
    p->xA = ar.take(ML * H * esz);
    p->xB = ar.take(ML * H * esz);
    p->dur_pred = (float*)ar.take(ML * 4);
    p->d_dur = (int32_t*)ar.take(ML * 4);
    p->d_cum = (int32_t*)ar.take(ML * 4);
    p->d_totals = (int32_t*)ar.take((size_t)2 * B * 4);  // [totals | guard flags]: one read-back
    p->d_guard = p->d_totals ? p->d_totals + B : nullptr;
    p->src_mask = (uint8_t*)ar.take(ML);
    for (int v = 0; v < FS2_MAX_VARIANCES; ++v) {
        p->pv_pred[v] = p->pv_spec[v] = p->pv_ms[v] = nullptr;
        if (v >= c.n_variances || !c.var_level[v]) continue;
        p->pv_pred[v] = (float*)ar.take(ML * 4);
        if (c.var_cwt[v]) {
            p->pv_spec[v] = (float*)ar.take(ML * 10 * 4);
            p->pv_ms[v] = (float*)ar.take((size_t)B * 8);
        }
    }
    return !ar.overflow;
}

struct EncodeScratch {
    LayerScratch sc;
    float* spec12 = nullptr;  // the CWT head's (M, 12) spectrogram: one buffer that every phone-level CWT variance reuses (encode_body)
    float* sdp_noise = nullptr;  // stochastic durations: the engine's copy of the call's (B, 2, L) noise ...
    void* sdp_ws = nullptr;      // ... and fs2_sdp_forward's workspace
    size_t sdp_ws_bytes = 0;
};
bool layout_encode_scratch(const fs2_engine* e, Arena& ar, int B, int L, EncodeScratch* s) {
    const fs2_config& c = e->cfg;
    layout_layer_scratch(e, ar, B, L, &s->sc);
    bool phone_cwt = false;
    for (int v = 0; v < c.n_variances; ++v) phone_cwt = phone_cwt || (c.var_level[v] && c.var_cwt[v]);
    s->spec12 = phone_cwt ? (float*)ar.take((size_t)B * L * 12 * 4) : nullptr;
    if (e->dur_stochastic) {
        s->sdp_noise = (float*)ar.take((size_t)B * 2 * L * 4);
        if (fs2_sdp_workspace_bytes(e->sdp.get(), B, L, &s->sdp_ws_bytes) != FS2_OK) s->sdp_ws_bytes = 0;
        s->sdp_ws = ar.take(s->sdp_ws_bytes);
    }
    return !ar.overflow;
}

struct DecodeScratch {
    void *yA, *yB;  // (B*T, H) ping-pong
    uint8_t* tmask;
    float* vpred[FS2_MAX_VARIANCES];  // frame-level variances
    int last_frame_v;                 // the last FRAME-level variance: pe + spk ride in its embedding add
    float *cw_spec, *cw_ms;           // a frame-level CWT head's (M, 12) spectrogram + (B, 2) mean / std
    LayerScratch sc;
};
// mask / variance predictions go straight into the caller's buffers when it wants them (out); out == nullptr: the caller's worst
// case, no buffer of its own
bool layout_decode_scratch(const fs2_engine* e, Arena& ar, int B, int T, const fs2_outputs* out, DecodeScratch* s) {
    const fs2_config& c = e->cfg;
    const size_t H = c.hidden, MT = (size_t)B * T, esz = e->esz;
    s->yA = ar.take(MT * H * esz);
    s->yB = ar.take(MT * H * esz);
    s->tmask = out && out->tgt_mask ? out->tgt_mask : (uint8_t*)ar.take(MT);
    s->last_frame_v = -1;
    bool frame_cwt = false;
    for (int v = 0; v < FS2_MAX_VARIANCES; ++v) {
        s->vpred[v] = nullptr;
        if (v >= c.n_variances || c.var_level[v]) continue;
        s->last_frame_v = v;
        frame_cwt = frame_cwt || c.var_cwt[v];
        s->vpred[v] = out && out->variances[v] ? out->variances[v] : (float*)ar.take(MT * 4);
    }
    s->cw_spec = frame_cwt ? (float*)ar.take(MT * 12 * 4) : nullptr;
    s->cw_ms = frame_cwt ? (float*)ar.take((size_t)B * 8) : nullptr;
    layout_layer_scratch(e, ar, B, T, &s->sc);
    return !ar.overflow;
}

size_t persist_need(const fs2_engine* e, int B, int L) {
    Arena a = Arena::counting();
    PersistBufs p;
    layout_persist(e, a, B, L, &p);
    return a.off;
}
size_t encode_scratch_need(const fs2_engine* e, int B, int L) {
    Arena a = Arena::counting();
    EncodeScratch s;
    layout_encode_scratch(e, a, B, L, &s);
    return a.off;
}
size_t decode_scratch_need(const fs2_engine* e, int B, int T) {
    Arena a = Arena::counting();
    DecodeScratch s;
    layout_decode_scratch(e, a, B, T, nullptr, &s);
    return a.off;
}
// Grow-only engine arena, or the caller's buffer (fs2_set_workspace) which must already be large enough.
int ensure_arena(fs2_engine* e, Arena& ar, size_t need, const char* what) {
    if (need > ar.cap && !ar.external) FS2_HIP(e, hipDeviceSynchronize());  // earlier work may still read the old block
    if (ar.reserve(need) != FS2_OK)
        return e->fail(FS2_ERR_NOMEM, ar.external ? "caller workspace too small: %s needs %zu bytes (fs2_workspace_bytes)"
                                                  : "%s arena: hipMalloc of %zu bytes failed", what, need);
    return FS2_OK;
}

int tap_store(fs2_engine* e, hipStream_t st, const std::string& name, const void* src, size_t n, int src_dt,
              Arena* arena = nullptr) {
    void* dst = (arena ? arena : &e->dbg)->take(n * 4);
    if (!dst) return e->fail(FS2_ERR_NOMEM, "debug arena too small");
    ConvertArgs a{src, dst, n};
    const int r = launch_convert(a, src_dt, FS2_F32, st);
    if (r != FS2_OK) return e->fail(r, "convert launch failed");
    e->taps[name] = {dst, n * 4};
    return FS2_OK;
}

void drop_graphs(fs2_engine* e) {
    for (auto& g : e->dgraphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    for (auto& g : e->egraphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    e->dgraphs.clear();
    e->egraphs.clear();
}

}  // namespace

// =================================================================================================
extern "C" {

int fs2_abi_version(void) { return FS2_ABI_VERSION; }

const char* fs2_status_string(int s) {
    switch (s) {
        case FS2_OK: return "ok";
        case FS2_ERR_HIP: return "HIP runtime error";
        case FS2_ERR_SHAPE: return "unsupported shape/config";
        case FS2_ERR_ARG: return "bad argument";
        case FS2_ERR_WEIGHT: return "weight error";
        case FS2_ERR_STATE: return "call order violated";
        case FS2_ERR_NOMEM: return "out of device memory";
    }
    return "unknown status";
}

const char* fs2_last_error(const fs2_engine* e) { return e ? e->err : "null engine"; }

int fs2_host_f32_to_f16(const float* src, uint16_t* dst, size_t n) {
    if ((!src || !dst) && n) return FS2_ERR_ARG;
    for (size_t i = 0; i < n; ++i) dst[i] = f32_to_f16_sat(src[i]).v;
    return FS2_OK;
}

int fs2_create(const fs2_config* cfg, fs2_engine** out) {
    if (!cfg || !out) return FS2_ERR_ARG;
    fs2_engine* e = new fs2_engine();
    e->cfg = *cfg;
    *out = e;  // returned even on failure so the caller can read fs2_last_error, then destroy
    const int r = check_config(e);
    if (r != FS2_OK) return r;
    e->dt = cfg->dtype;
    e->fdt = cfg->dtype == FS2_BF16 ? FS2_BF16 : FS2_F32;
    e->bdt = (cfg->dtype == FS2_F32 || cfg->dtype == FS2_F32_X3) ? FS2_F32 : (cfg->dtype == FS2_MIXED_F16_X3 ? FS2_F16 : FS2_BF16);
    e->esz = elem_bytes(e->fdt) > elem_bytes(e->bdt) ? elem_bytes(e->fdt) : elem_bytes(e->bdt);
    // every fp32-weight GEMM / conv as bf16 x 3 split products (nothing in the front looks at bdt: FS2_MIXED_F16_X3's front IS FS2_MIXED_X3's)
    e->front_split = cfg->dtype == FS2_MIXED_X3 || cfg->dtype == FS2_F32_X3 || cfg->dtype == FS2_MIXED_F16_X3;
    build_spec(e);
    return FS2_OK;
}

// A second engine over the SAME device weights (read-only after fs2_finalize): its own workspace arenas, host-side state, graphs,
// profiling slots - what a second forward in flight needs (lightningfastspeech2_amd.model.ForwardPipeline).  One engine = one caller
// thread at a time; an engine and its clones may run concurrently on different streams.
int fs2_clone(const fs2_engine* src, fs2_engine** out) {
    if (!src || !out) return FS2_ERR_ARG;
    if (!src->finalized) return FS2_ERR_STATE;
    fs2_engine* e = new fs2_engine();
    static_cast<Model&>(*e) = *src;     // shared: the weights stay where they are (dev_allocs counts the owners)
    static_cast<Switches&>(*e) = *src;  // inherited
    e->finalized = true;
    *out = e;
    return FS2_OK;
}

int fs2_destroy(fs2_engine* e) {
    if (!e) return FS2_OK;
    (void)hipDeviceSynchronize();
    e->dev_allocs.reset();  // frees the weights unless a clone still holds them
    e->persist.release();
    e->scratch.release();
    e->dbg.release();
    e->dbg_enc.release();
    if (e->h_pinned) (void)hipHostFree(e->h_pinned);
    drop_graphs(e);
    if (e->gev_in) (void)hipEventDestroy(e->gev_in);
    if (e->gev_out) (void)hipEventDestroy(e->gev_out);
    if (e->gstream) (void)hipStreamDestroy(e->gstream);
    for (auto& s : e->prof)
        for (auto& ev : s.ev) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    delete e;
    return FS2_OK;
}

int fs2_load_weight(fs2_engine* e, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!e || !name || !data || !shape || ndim < 0) return FS2_ERR_ARG;
    if (e->finalized) return e->fail(FS2_ERR_STATE, "weights already finalized");
    static const char kDur[] = "variance_adaptor.duration_predictor.";
    if (e->dur_stochastic && !strncmp(name, kDur, sizeof(kDur) - 1)) {
        const int r = fs2_sdp_load_weight(e->sdp.get(), name + sizeof(kDur) - 1, data, shape, ndim);
        if (r != FS2_OK) return e->fail(r, "%s (stochastic duration predictor: '%s')", fs2_sdp_last_error(e->sdp.get()), name);
        e->weight_seen = true;
        return FS2_OK;
    }
    FS2_TRY(check_deterministic_duration(e));
    FS2_TRY(e->w.load(*e, name, data, shape, ndim));
    e->weight_seen = true;
    return FS2_OK;
}

int fs2_finalize(fs2_engine* e) {
    if (!e) return FS2_ERR_ARG;
    if (e->finalized) return FS2_OK;
    FS2_TRY(check_deterministic_duration(e));
    if (const char* missing = e->w.first_missing()) return e->fail(FS2_ERR_WEIGHT, "missing weight '%s'", missing);
    const fs2_config& c = e->cfg;
    const int H = c.hidden;
    FS2_TRY(up_vec(e, "phone_embedding.weight", &e->phone_table));
    FS2_TRY(up_vec(e, "positional_encoding.pe", &e->pe));
    FS2_TRY(up_vec(e, "speaker_embedding.projection.weight", &e->spk_w));
    FS2_TRY(up_vec(e, "speaker_embedding.projection.bias", &e->spk_b));
    e->enc.resize(c.enc_layers);
    for (int i = 0; i < c.enc_layers; ++i)
        FS2_TRY(make_layer(e, "encoder.layers." + std::to_string(i), H, c.enc_filter, c.enc_depthwise, &e->enc[i], e->fdt));
    e->dec.resize(c.dec_layers);
    for (int i = 0; i < c.dec_layers; ++i)
        FS2_TRY(make_layer(e, "decoder.layers." + std::to_string(i), H, c.dec_filter, c.dec_depthwise, &e->dec[i], e->bdt));
    if (H > 256) {  // stacks of wide depth-wise 16-bit (bf16 / f16) blocks: norm2 of block i - 1 folded into the in-projection of block i
        const auto fold_in_proj = [&](const std::string& stack, int i, LayerW* L) -> int {
            const std::string p = stack + std::to_string(i) + ".self_attn.in_proj_";
            FS2_TRY(make_norm_folded(e, p + "weight", p + "bias", stack + std::to_string(i - 1) + ".norm2", &L->in_proj_f, &L->in_wg, L->in_proj.dt));
            L->has_fold = true;
            return FS2_OK;
        };
        for (int i = 1; i < c.enc_layers && c.enc_depthwise && e->fdt == FS2_BF16; ++i) FS2_TRY(fold_in_proj("encoder.layers.", i, &e->enc[i]));
        for (int i = 1; i < c.dec_layers && c.dec_depthwise && is_16bit(e->bdt); ++i) FS2_TRY(fold_in_proj("decoder.layers.", i, &e->dec[i]));
    }
    if (e->dur_stochastic) {
        const int r = fs2_sdp_finalize(e->sdp.get());
        if (r != FS2_OK) return e->fail(r, "stochastic duration predictor: %s", fs2_sdp_last_error(e->sdp.get()));
    } else {
        FS2_TRY(make_predictor(e, "variance_adaptor.duration_predictor", c.dur_nlayers, c.dur_filter, c.dur_depthwise, &e->dur, e->fdt));
    }
    e->vars.resize(c.n_variances);
    for (int v = 0; v < c.n_variances; ++v) {
        const std::string p = std::string("variance_adaptor.encoders.") + c.var_names[v];
        FS2_TRY(make_predictor(e, p + ".predictor", c.var_nlayers[v], c.var_filter, c.var_depthwise, &e->vars[v].pred, e->fdt, c.var_cwt[v] != 0));
        if (c.var_cwt[v]) {
            FS2_TRY(up_vec(e, p + ".mean_std_linear.weight", &e->vars[v].pred.ms_w));
            FS2_TRY(up_vec(e, p + ".mean_std_linear.bias", &e->vars[v].pred.ms_b));
        }
        FS2_TRY(up_vec(e, p + ".bins", &e->vars[v].bins));
        FS2_TRY(up_vec(e, p + ".embedding.weight", &e->vars[v].emb));
    }
    FS2_TRY(make_conv(e, "linear.weight", "linear.bias", &e->mel, e->bdt));
    // (the row-scaled product with an fp32 store exists for narrow heads only - route_gemm's GF_RS_NARROW row: N < 192 -; a wider mel head keeps the
    //  normalise-only pass + the plain mel GEMM)
    if (H > 256 && c.dec_layers > 0 && c.dec_depthwise && is_16bit(e->bdt) && c.n_mels < 192) {
        // mel = Linear(LN2_last(v2)) evaluated on v2
        FS2_TRY(make_norm_folded(e, "linear.weight", "linear.bias", "decoder.layers." + std::to_string(c.dec_layers - 1) + ".norm2", &e->mel_f, &e->mel_wg, e->bdt));
        e->mel_fold = true;
    }
    e->priors_w.resize(c.n_priors);
    for (int p = 0; p < c.n_priors; ++p) {
        const std::string q = std::string("prior_embeddings.") + c.prior_names[p];
        FS2_TRY(up_vec(e, q + ".bins", &e->priors_w[p].bins));
        // relu(Embedding[idx]) (model.py:161) == Embedding'[idx] with the table rectified once here
        std::vector<float> t = W(e, q + ".embedding.weight").data;
        for (float& v : t) v = v > 0.f ? v : 0.f;
        FS2_TRY(upload_f32(e, t.data(), t.size(), &e->priors_w[p].emb));
    }
    e->w.drop();
    e->finalized = true;
    return FS2_OK;
}

int fs2_set_fused_predictor(fs2_engine* e, int32_t on) {
    if (!e) return FS2_ERR_ARG;
    e->fuse_predictor = on != 0;
    return FS2_OK;
}

int fs2_set_debug(fs2_engine* e, int32_t on) {
    if (!e) return FS2_ERR_ARG;
    e->debug = on != 0;
    return FS2_OK;
}

int fs2_set_deferred_layernorm(fs2_engine* e, int32_t on) {
    if (!e) return FS2_ERR_ARG;
    e->defer_ln = on != 0;
    return FS2_OK;
}

// One A/B switch of THIS engine (the values of fs2_op_set_gemm_variant, include/fs2.h); clones made afterwards inherit it.
int fs2_set_tuning(fs2_engine* e, int32_t knob) {
    if (!e) return FS2_ERR_ARG;
    // knobs no launch of the engine reads (the training step's backward kernels, the strided-batched GEMM, fs2_op_col_sum, the operator-level
    // on-the-fly weight split - which allocates per launch and cannot run under graph capture): accepted by fs2_op_set_gemm_variant on the
    // calling thread only; here they would label a default-configuration measurement as switched
    const bool op_only = (knob >= 900 && knob <= 909) || knob == 1000 || knob == 1001 || knob == 1100 || knob == 1101 ||
                         knob == 700 || knob == 701 || knob == 800 || knob == 801 || knob == 500 || knob == 501;
    if (op_only) return e->fail(FS2_ERR_ARG, "fs2_set_tuning(%d): an operator-level switch no engine launch reads (use fs2_op_set_gemm_variant on the calling thread)", (int)knob);
    const int r = apply_knob(e->tune, knob);
    if (r != FS2_OK) return e->fail(r, "fs2_set_tuning(%d): not a defined switch", (int)knob);
    return FS2_OK;
}

int fs2_set_folded_layernorm(fs2_engine* e, int32_t on) {
    if (!e) return FS2_ERR_ARG;
    e->fold_ln = on != 0;
    return FS2_OK;
}

int fs2_set_zero_pad_mel(fs2_engine* e, int32_t on) {
    if (!e) return FS2_ERR_ARG;
    e->zero_pad_mel = on != 0;
    return FS2_OK;
}

int fs2_workspace_bytes(const fs2_engine* e, int32_t B, int32_t L, int32_t T, size_t* persist, size_t* scratch) {
    if (!e || B <= 0 || L <= 0 || T < 0) return FS2_ERR_ARG;
    if (persist) *persist = persist_need(e, B, L);
    if (scratch) {
        const size_t enc = encode_scratch_need(e, B, L), dec = T > 0 ? decode_scratch_need(e, B, T) : 0;
        *scratch = enc > dec ? enc : dec;
    }
    return FS2_OK;
}

int fs2_set_workspace(fs2_engine* e, void* persist, size_t persist_bytes_, void* scratch, size_t scratch_bytes_) {
    if (!e || (persist == nullptr) != (scratch == nullptr)) return e ? e->fail(FS2_ERR_ARG, "give both buffers or neither") : FS2_ERR_ARG;
    if (((uintptr_t)persist | (uintptr_t)scratch) & 255) return e->fail(FS2_ERR_ARG, "workspace buffers must be 256-byte aligned");
    if (e->mid_forward && (char*)persist != e->persist.base)
        return e->fail(FS2_ERR_STATE, "the persist buffer holds the encoder state between fs2_encode and fs2_decode: only scratch may change there");
    if (!e->mid_forward) e->persist.adopt(persist, persist_bytes_);
    e->scratch.adopt(scratch, scratch_bytes_);
    return FS2_OK;
}

int fs2_set_frames(fs2_engine* e, int32_t T) {
    if (!e) return FS2_ERR_ARG;
    if (!e->encoded) return e->fail(FS2_ERR_STATE, "fs2_set_frames without a preceding successful fs2_encode");
    if (T < e->T) return e->fail(FS2_ERR_ARG, "fs2_set_frames can only pad: T=%d < this batch's %d", T, e->T);
    if (T > e->cfg.max_frames || T > e->cfg.pe_len) return e->fail(FS2_ERR_SHAPE, "T=%d exceeds max_frames/positional table", T);
    e->T = T;
    return FS2_OK;
}

static int encode_body(fs2_engine* e, const int64_t* phones, const float* speaker, const int32_t* forced, const EncodeScratch& es, hipStream_t st);

// One VarianceEncoder.forward (model.py:409-441) on the (B*S, H) rows x: the predictor, then x += Embedding[bucketize(pred * std + mean)]
// (or of the forced indices / targets: model.py:417-422), optionally + pe + spk behind the last frame-level variance
// (fastspeech2.py:705-718).  Used at the frame level by the decode phase (model.py:315-333) and at the phone level by the encode
// phase (model.py:276-294).  x / xalt are the ping-pong pair: swapped when the embedding rode in the predictor launch.
static int variance_stage(fs2_engine* e, hipStream_t st, int v, void*& x, void*& xalt, int B, int S, const uint8_t* mask, float* vpred,
                          const LayerScratch& sc, const CwtOut* cwo, bool add_pe_spk, Arena& dbg) {
    const fs2_config& c = e->cfg;
    const size_t M = (size_t)B * S, H = c.hidden, esz = e->esz;
    // the encoder's bucketize + embedding add rides in the predictor launch where nothing else wants its by-products
    // (bucket indices for the debug taps, forced buckets / targets of the teacher-forced and oracle paths)
    const bool tail_ok = e->tune.pred_fuse_embed && !e->debug && !e->forced_idx[v] && !e->forced_tgt[v] && !c.var_cwt[v] &&
                         (e->fdt == FS2_BF16 || (e->fdt == FS2_F32 && e->front_split && e->vars[v].pred.wpk_lo)) && H == 256;
    const EmbedTail tl{xalt, e->vars[v].bins, e->vars[v].emb, c.var_nbins, c.var_std[v], c.var_mean[v],
                       add_pe_spk ? e->pe : nullptr, add_pe_spk ? e->ps.spk : nullptr};
    bool tail_done = false;
    FS2_TRY(predictor(e, st, e->vars[v].pred, x, B, S, mask, vpred, sc, cwo, tail_ok ? &tl : nullptr, &tail_done));
    if (tail_done) {
        std::swap(x, xalt);
        return FS2_OK;
    }
    int32_t* idx = nullptr;
    if (e->debug) {
        idx = (int32_t*)dbg.take(M * 4);
        if (!idx) return e->fail(FS2_ERR_NOMEM, "debug arena too small");
        e->taps[std::string("bucket_") + c.var_names[v]] = {idx, M * 4};
    }
    Bracket br(e, FS2_K_ROWOPS, st, 0, 2.0 * M * H * esz);
    BucketArgs ba{x, vpred, e->vars[v].bins, e->vars[v].emb, c.var_nbins, c.var_std[v], c.var_mean[v],
                  add_pe_spk ? e->pe : nullptr, add_pe_spk ? e->ps.spk : nullptr, x, idx, B, S, (int)H,
                  e->forced_idx[v], 0, e->forced_tgt[v]};
    if (launch_bucket_embed(ba, e->fdt, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "bucket_embed launch failed");
    return FS2_OK;
}
static int run_phase(fs2_engine* e, std::vector<fs2_engine::GraphEntry>& cache, const std::vector<uint64_t>& key, bool plain,
                     hipStream_t st, const std::function<int(hipStream_t)>& body);

int fs2_encode(fs2_engine* e, const int64_t* phones, const float* speaker, int32_t B, int32_t L,
               const int32_t* forced, void* stream, int32_t* T_out) {
    if (!e || !phones || !speaker || !T_out || B <= 0 || L <= 0) return e ? e->fail(FS2_ERR_ARG, "bad encode argument") : FS2_ERR_ARG;
    if (!e->finalized) return e->fail(FS2_ERR_STATE, "fs2_finalize not called");
    if (L > e->cfg.pe_len) return e->fail(FS2_ERR_SHAPE, "L=%d exceeds positional table %d", L, e->cfg.pe_len);
    if (e->dur_stochastic && (!e->noise_dev || e->noise_B != B || e->noise_L != L))
        return e->fail(FS2_ERR_STATE, "fs2_set_duration_noise(B=%d, L=%d) required before fs2_encode of a stochastic engine", B, L);
    hipStream_t st = (hipStream_t)stream;
    const fs2_config& c = e->cfg;
    e->encoded = false;
    e->mid_forward = false;
    e->B = B;
    e->L = L;
    e->taps.clear();
    // the arenas are reused across calls: earlier work on this stream that still reads them is
    // ordered before the kernels below; a (rare) growth reallocates after a device sync
    FS2_TRY(ensure_arena(e, e->persist, persist_need(e, B, L), "persist"));
    FS2_TRY(ensure_arena(e, e->scratch, encode_scratch_need(e, B, L), "scratch"));
    if (!layout_persist(e, e->persist, B, L, &e->ps)) return e->fail(FS2_ERR_NOMEM, "persist arena too small");
    EncodeScratch es;
    if (!layout_encode_scratch(e, e->scratch, B, L, &es)) return e->fail(FS2_ERR_NOMEM, "scratch arena too small");
    bool pv_forced = false;
    for (int v = 0; v < c.n_variances; ++v) pv_forced = pv_forced || (c.var_level[v] && (e->forced_idx[v] || e->forced_tgt[v]));
    if (e->h_pinned_cap < 2 * B) {
        if (e->h_pinned) (void)hipHostFree(e->h_pinned);
        e->h_pinned = nullptr;
        FS2_HIP(e, hipHostMalloc((void**)&e->h_pinned, (size_t)2 * B * 4, hipHostMallocDefault));
        e->h_pinned_cap = 2 * B;
        drop_graphs(e);  // captured copies point at the old pinned block
    }
    // every launch of the phase (no host decision among them), plainly or as a replayed hipGraph (fs2_set_graphs)
    {
        std::vector<uint64_t> key = {(uint64_t)B, (uint64_t)L, (uint64_t)e->persist.base, (uint64_t)e->scratch.base, (uint64_t)phones,
                                     (uint64_t)speaker, (uint64_t)forced, (uint64_t)e->h_pinned, (uint64_t)e->fuse_predictor, (uint64_t)e->tune.gen,
                                     (uint64_t)e->defer_ln, (uint64_t)e->front_split, (uint64_t)e->fold_ln};
        // a prior tensor / a phone-level forced target / the duration noise is a one-shot pointer of the call
        const bool plain = c.n_priors != 0 || pv_forced || e->dur_stochastic;
        FS2_TRY(run_phase(e, e->egraphs, key, plain, st, [&](hipStream_t s2) { return encode_body(e, phones, speaker, forced, es, s2); }));
    }
    FS2_HIP(e, hipStreamSynchronize(st));  // the one host sync of the forward (output shape)
    e->totals.assign(e->h_pinned, e->h_pinned + B);
    e->guard.assign(e->h_pinned + B, e->h_pinned + 2 * B);
    int mx = 0;
    for (int b = 0; b < B; ++b) mx = e->totals[b] > mx ? e->totals[b] : mx;
    e->T = mx < c.max_frames ? mx : c.max_frames;                            // model.py:355
    if (e->T > c.pe_len) return e->fail(FS2_ERR_SHAPE, "T=%d exceeds positional table %d", e->T, c.pe_len);
    *T_out = e->T;
    e->encoded = true;
    e->mid_forward = true;
    return FS2_OK;
}

static int encode_body(fs2_engine* e, const int64_t* phones, const float* speaker, const int32_t* forced, const EncodeScratch& es, hipStream_t st) {
    const fs2_config& c = e->cfg;
    const PersistBufs& ps = e->ps;
    const LayerScratch& sc = es.sc;
    const int B = e->B, L = e->L;
    const size_t H = c.hidden, ML = (size_t)B * L, esz = e->esz;
    {   // speaker projection + phone embedding + PE                       fastspeech2.py:651-660
        Bracket br(e, FS2_K_ROWOPS, st, 0, ML * H * esz);
        SpkProjArgs sp{speaker, e->spk_w, e->spk_b, ps.spk, B, (int)H, c.dvec_dim};
        if (launch_spk_proj(sp, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "spk_proj launch failed");
        EmbedArgs em{phones, e->phone_table, e->pe, ps.spk, ps.xA, ps.src_mask, B, L, (int)H, c.n_phones};
        if (launch_embed(em, e->fdt, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "embed launch failed");
        MaskBitsArgs mb{ps.src_mask, sc.bits, B, L, sc.nw64};
        if (launch_mask_bits(mb, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "mask_bits launch failed");
    }
    FS2_TRY(run_stack(e, st, e->enc, ps.xA, ps.xB, B, L, c.enc_heads, sc, false));  // fastspeech2.py:685
    if (e->debug) {  // the reference's encoder output, i.e. before the prior embeddings are added
        const size_t need_d = al(ML * H * 4) + (size_t)c.n_variances * al(ML * 4) + 4096;
        if (need_d > e->dbg_enc.cap) FS2_HIP(e, hipDeviceSynchronize());
        if (e->dbg_enc.reserve(need_d) != FS2_OK) return e->fail(FS2_ERR_NOMEM, "debug arena");
        FS2_TRY(tap_store(e, st, "encoder_out", ps.xA, ML * H, e->fdt, &e->dbg_enc));
    }
    if (c.n_priors) {                                                        // fastspeech2.py:687-692
        if (!e->priors_dev || e->priors_B != B) return e->fail(FS2_ERR_STATE, "fs2_set_priors(B=%d) required before fs2_encode", B);
        for (int p = 0; p < c.n_priors; ++p) {
            BucketArgs ba{ps.xA, e->priors_dev + (size_t)p * B, e->priors_w[p].bins, e->priors_w[p].emb, c.var_nbins,
                          1.0f, 0.0f, nullptr, nullptr, ps.xA, nullptr, B, L, (int)H, nullptr, 1};
            if (launch_bucket_embed(ba, e->fdt, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "prior embedding launch failed");
        }
        e->priors_dev = nullptr;  // one-shot
    }
    // duration predictor + rounding + prefix sums                          model.py:259,299-309
    if (e->dur_stochastic) {  // model.py:260-268: the flow predictor on encoder_out.detach(), noise from the caller (sdp.py:335-338)
        FS2_HIP(e, hipMemcpyAsync(es.sdp_noise, e->noise_dev, (size_t)B * 2 * L * 4, hipMemcpyDeviceToDevice, st));
        e->noise_dev = nullptr;  // one-shot
        const int r = fs2_sdp_forward(e->sdp.get(), e->fdt, ps.xA, ps.src_mask, es.sdp_noise, ps.dur_pred, es.sdp_ws, es.sdp_ws_bytes, B, L, st);
        if (r != FS2_OK) return e->fail(r, "stochastic duration predictor: %s", fs2_sdp_last_error(e->sdp.get()));
    } else {
        FS2_TRY(predictor(e, st, e->dur, ps.xA, B, L, ps.src_mask, ps.dur_pred, sc));
    }
    // phone-level variance encoders (variance_levels[i] == "phone"), in list order, AFTER the duration predictor has seen x and BEFORE
    // the length regulator: each adds its embedding to the rows that get regulated                      model.py:276-294
    // The rows ping-pong between xA and xB through local pointers (variance_stage swaps them where the embedding rode in the predictor
    // launch) and end in xA, where decode regulates them from: a replayed graph does not run this body (run_phase).
    void* x = ps.xA;
    void* xalt = ps.xB;
    for (int v = 0; v < c.n_variances; ++v) {
        if (!c.var_level[v]) continue;
        const CwtOut cwo{es.spec12, ps.pv_ms[v], ps.pv_spec[v]};
        FS2_TRY(variance_stage(e, st, v, x, xalt, B, L, ps.src_mask, ps.pv_pred[v], sc, c.var_cwt[v] ? &cwo : nullptr, false, e->dbg_enc));
        e->forced_idx[v] = nullptr, e->forced_tgt[v] = nullptr;  // one-shot, consumed here
    }
    if (x != ps.xA) FS2_HIP(e, hipMemcpyAsync(ps.xA, x, ML * H * esz, hipMemcpyDeviceToDevice, st));  // an odd number of swaps
    // stochastic: ceil(exp(logw)), 0 where logw == 0 (model.py:302-305) in front of the same guard and prefix sums
    DurationArgs da{ps.dur_pred, ps.src_mask, forced, ps.d_dur, ps.d_cum, ps.d_totals, ps.d_guard, B, L, e->dur_stochastic ? 1 : 0};
    if (launch_durations(da, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "durations launch failed");
    FS2_HIP(e, hipMemcpyAsync(e->h_pinned, ps.d_totals, (size_t)2 * B * 4, hipMemcpyDeviceToHost, st));
    return FS2_OK;
}

int fs2_set_priors(fs2_engine* e, const float* priors_device, int32_t B) {
    if (!e || !priors_device || B <= 0) return FS2_ERR_ARG;
    if (e->cfg.n_priors == 0) return e->fail(FS2_ERR_STATE, "this engine was configured without priors");
    e->priors_dev = priors_device;
    e->priors_B = B;
    return FS2_OK;
}

int fs2_set_stochastic_duration(fs2_engine* e, int32_t on) {
    if (!e) return FS2_ERR_ARG;
    if (e->finalized || e->weight_seen)
        return e->fail(FS2_ERR_STATE, "fs2_set_stochastic_duration is legal only between fs2_create and the first fs2_load_weight");
    if (e->w.empty()) return e->fail(FS2_ERR_STATE, "fs2_create did not succeed");
    const fs2_config& c = e->cfg;
    std::shared_ptr<fs2_sdp> h;
    if (on) {
        if (c.dur_depthwise)
            return e->fail(FS2_ERR_SHAPE, "duration_stochastic with duration_depthwise_conv: the reference builds no such predictor (model.py:196-200)");
        fs2_sdp* raw = nullptr;
        const int r = fs2_sdp_create(FS2_ABI_VERSION, c.hidden, c.dur_filter, c.dur_kernel, c.dur_nlayers, &raw);
        h.reset(raw, [](fs2_sdp* p) { if (p) (void)fs2_sdp_destroy(p); });
        if (r != FS2_OK) return e->fail(r, "stochastic duration predictor: %s", raw ? fs2_sdp_last_error(raw) : "out of memory");
    }
    e->dur_stochastic = on != 0;
    e->sdp = h;
    e->w.clear();
    build_spec(e);
    return FS2_OK;
}

int fs2_set_duration_noise(fs2_engine* e, const float* noise_device, int32_t B, int32_t L) {
    if (!e || !noise_device || B <= 0 || L <= 0) return FS2_ERR_ARG;
    if (!e->dur_stochastic) return e->fail(FS2_ERR_STATE, "this engine's duration predictor is not stochastic (fs2_set_stochastic_duration)");
    e->noise_dev = noise_device;
    e->noise_B = B;
    e->noise_L = L;
    return FS2_OK;
}

int fs2_last_totals(const fs2_engine* e, int32_t* totals, int32_t* guard, int32_t B) {
    if (!e || !e->encoded || B != e->B) return FS2_ERR_STATE;
    if (totals) memcpy(totals, e->totals.data(), (size_t)B * 4);
    if (guard) memcpy(guard, e->guard.data(), (size_t)B * 4);
    return FS2_OK;
}

static int decode_body(fs2_engine* e, const fs2_outputs* out, hipStream_t st) {
    const fs2_config& c = e->cfg;
    const int B = e->B, L = e->L, T = e->T;
    const size_t H = c.hidden, MT = (size_t)B * T, ML = (size_t)B * L, esz = e->esz;
    // the phone-level outputs live in the engine's persistent arena (decode does not touch it): copied out BEHIND the decode
    // launches - three hipMemcpyAsync cost the host ~15 us each, which the GPU would otherwise spend idle at the seam
    const PersistBufs& ps = e->ps;
    auto phone_outputs = [&]() -> int {
        if (out->duration_prediction) FS2_HIP(e, hipMemcpyAsync(out->duration_prediction, ps.dur_pred, ML * 4, hipMemcpyDeviceToDevice, st));
        if (out->duration_rounded) FS2_HIP(e, hipMemcpyAsync(out->duration_rounded, ps.d_dur, ML * 4, hipMemcpyDeviceToDevice, st));
        if (out->src_mask) FS2_HIP(e, hipMemcpyAsync(out->src_mask, ps.src_mask, ML, hipMemcpyDeviceToDevice, st));
        for (int v = 0; v < c.n_variances; ++v) {  // phone-level variances: (B, L) outputs, produced by the encode phase
            if (!c.var_level[v]) continue;
            if (out->variances[v]) FS2_HIP(e, hipMemcpyAsync(out->variances[v], ps.pv_pred[v], ML * 4, hipMemcpyDeviceToDevice, st));
            if (c.var_cwt[v] && out->var_spectrogram[v]) FS2_HIP(e, hipMemcpyAsync(out->var_spectrogram[v], ps.pv_spec[v], ML * 10 * 4, hipMemcpyDeviceToDevice, st));
            if (c.var_cwt[v] && out->var_mean_std[v]) FS2_HIP(e, hipMemcpyAsync(out->var_mean_std[v], ps.pv_ms[v], (size_t)B * 8, hipMemcpyDeviceToDevice, st));
        }
        return FS2_OK;
    };
    if (T == 0) { e->encoded = false; e->mid_forward = false; return phone_outputs(); }

    FS2_TRY(ensure_arena(e, e->scratch, decode_scratch_need(e, B, T), "scratch"));  // too small: the caller may retry with more
    e->mid_forward = false;  // from here on the encoder state is consumed by this call
    DecodeScratch ds;
    if (!layout_decode_scratch(e, e->scratch, B, T, out, &ds)) return e->fail(FS2_ERR_NOMEM, "scratch arena too small");
    void *yA = ds.yA, *yB = ds.yB;  // swapped below: locals (run_phase's rule for a body)
    uint8_t* const tmask = ds.tmask;
    const LayerScratch& sc = ds.sc;
    if (e->debug) {
        const size_t need_d = 3 * al(MT * H * 4) + (size_t)c.n_variances * al(MT * 4) + 4096;
        if (need_d > e->dbg.cap) FS2_HIP(e, hipDeviceSynchronize());
        if (e->dbg.reserve(need_d) != FS2_OK) return e->fail(FS2_ERR_NOMEM, "debug arena");
    }

    {   // length regulator                                                  model.py:311,349-370
        Bracket br(e, FS2_K_ROWOPS, st, 0, 2.0 * MT * H * esz);
        RegulateArgs ra{ps.xA, ps.d_cum, ps.d_totals, yA, tmask, B, L, T, (int)H};
        if (launch_regulate(ra, e->fdt, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "regulate launch failed");
        MaskBitsArgs mb{tmask, sc.bits, B, T, sc.nw64};
        if (launch_mask_bits(mb, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "mask_bits launch failed");
    }
    if (e->debug) FS2_TRY(tap_store(e, st, "regulated", yA, MT * H, e->fdt));
    // frame-level variance encoders, sequential                            model.py:315-333
    const bool fuse_pe = !e->debug;
    for (int v = 0; v < c.n_variances; ++v) {
        if (c.var_level[v]) continue;  // phone level: done by the encode phase
        const CwtOut cwo{ds.cw_spec, out->var_mean_std[v] ? out->var_mean_std[v] : ds.cw_ms, out->var_spectrogram[v]};
        FS2_TRY(variance_stage(e, st, v, yA, yB, B, T, tmask, ds.vpred[v], sc, c.var_cwt[v] ? &cwo : nullptr, v == ds.last_frame_v && fuse_pe, e->dbg));
    }
    if (e->debug) FS2_TRY(tap_store(e, st, "adaptor_out", yA, MT * H, e->fdt));
    if (!fuse_pe || ds.last_frame_v < 0) {  // y = (x + pe) + spk            fastspeech2.py:705-718
        BucketArgs ba{yA, nullptr, nullptr, nullptr, 0, 0.f, 0.f, e->pe, ps.spk, yA, nullptr, B, T, (int)H, nullptr};
        if (launch_bucket_embed(ba, e->fdt, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "pe/spk add launch failed");
    }
    if (e->fdt != e->bdt) {  // FS2_MIXED: the decoder's input, rounded once to the back dtype (yB is free until layer 0 writes it)
        ConvertArgs ca{yA, yB, MT * H};
        if (launch_convert(ca, e->fdt, e->bdt, st) != FS2_OK) return e->fail(FS2_ERR_HIP, "front -> back conversion failed");
        std::swap(yA, yB);
    }
    // (the mel head takes the last block's norm2 folded in where it can: nothing else reads the decoder's normalised output)
    bool dec_pre = false;
    FS2_TRY(run_stack(e, st, e->dec, yA, yB, B, T, c.dec_heads, sc, true, e->mel_fold && out->mel && !e->debug, &dec_pre));  // fastspeech2.py:719-721
    if (e->debug) FS2_TRY(tap_store(e, st, "decoder_out", yA, MT * H, e->bdt));
    if (out->mel && dec_pre) {                                               // fastspeech2.py:723
        const RowScale rs{sc.rsf, e->mel_wg};
        FS2_TRY(gemm(e, st, e->mel_f, yA, out->mel, (int)MT, (int)MT, false, FS2_F32, {.zero_rows = e->zero_pad_mel ? tmask : nullptr, .rowscale = &rs}));
    } else if (out->mel) {
        FS2_TRY(gemm(e, st, e->mel, yA, out->mel, (int)MT, (int)MT, false, FS2_F32, {.zero_rows = e->zero_pad_mel ? tmask : nullptr}));
    }
    for (int v = 0; v < FS2_MAX_VARIANCES; ++v) e->forced_idx[v] = nullptr, e->forced_tgt[v] = nullptr;  // one-shot
    return phone_outputs();
}

// A phase of the forward (encode: embedding .. durations + the totals' copy to pinned memory; decode: length regulator .. mel head:
// ~100 / ~50 launches on one stream, no host decision inside) as a hipGraph.  A signature = shape + every buffer address a launch
// sees (the caller's tensors, the arenas).  First sight of a signature: plain launches (lazy initialisation happens there); second
// sight: the same code path runs under stream capture on an engine-owned non-blocking stream, is instantiated and launched; from
// then on one hipGraphLaunch.  The caller's stream (the legacy null stream included, which cannot be captured itself) is ordered
// around it with two events.  Anything a capture cannot hold (debug taps, per-class profiling events, one-shot forced buckets or
// priors) takes the plain path.
// Rule for a body: a replay runs its launches, not its host code.  So nothing that fs2_decode or the next fs2_encode reads may be
// host state that the body changes (an engine pointer swapped, a buffer chosen by parity): such a change happens at capture only
// and is missing on every replay.  Ping-pong choices live in the body's locals.
static int run_phase(fs2_engine* e, std::vector<fs2_engine::GraphEntry>& cache, const std::vector<uint64_t>& key, bool plain,
                     hipStream_t st, const std::function<int(hipStream_t)>& body) {
    static const bool gdbg = getenv("FS2_GRAPH_DEBUG") != nullptr;
    plain = plain || !e->use_graph || e->debug;
    for (int k = 0; k < FS2_K_COUNT && !plain; ++k) plain = e->prof[k].enabled;
    if (plain) return body(st);
    fs2_engine::GraphEntry* g = nullptr;
    for (auto& c : cache) if (c.key == key) { g = &c; break; }
    if (!g) {  // first sight: remember it, run plainly
        if (cache.size() >= 8) {
            size_t old = 0;
            for (size_t i = 1; i < cache.size(); ++i) if (cache[i].stamp < cache[old].stamp) old = i;
            if (cache[old].exec) (void)hipGraphExecDestroy(cache[old].exec);
            cache.erase(cache.begin() + old);
        }
        cache.emplace_back();
        cache.back().key = key;
        cache.back().stamp = ++e->gclock;
        if (gdbg) fprintf(stderr, "fs2 graph: new signature (%zu cached)\n", cache.size());
        return body(st);
    }
    g->stamp = ++e->gclock;
    if (g->bad) { if (gdbg) fprintf(stderr, "fs2 graph: signature marked bad\n"); return body(st); }
    if (!e->gstream) {
        if (hipStreamCreateWithFlags(&e->gstream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e->gev_in, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e->gev_out, hipEventDisableTiming) != hipSuccess) {
            e->use_graph = false;
            return body(st);
        }
    }
    if (!g->exec) {  // second sight: capture the same code path
        if (hipStreamBeginCapture(e->gstream, hipStreamCaptureModeThreadLocal) != hipSuccess) { g->bad = true; return body(st); }
        const bool enc = e->encoded, mid = e->mid_forward;
        const int r = body(e->gstream);
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(e->gstream, &graph);
        hipError_t ie = hipSuccess;
        if (r != FS2_OK || ce != hipSuccess || !graph || (ie = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0)) != hipSuccess) {
            if (gdbg) fprintf(stderr, "fs2 graph: capture failed (body %d, end %d %s, instantiate %d)\n", r, (int)ce, hipGetErrorString(ce), (int)ie);
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            g->exec = nullptr;
            g->bad = true;
            e->encoded = enc; e->mid_forward = mid;
            return body(st);  // nothing was executed during the capture
        }
        (void)hipGraphDestroy(graph);
    }
    FS2_HIP(e, hipEventRecord(e->gev_in, st));
    FS2_HIP(e, hipStreamWaitEvent(e->gstream, e->gev_in, 0));
    FS2_HIP(e, hipGraphLaunch(g->exec, e->gstream));
    FS2_HIP(e, hipEventRecord(e->gev_out, e->gstream));
    FS2_HIP(e, hipStreamWaitEvent(st, e->gev_out, 0));
    e->graph_replays++;
    return FS2_OK;
}

int fs2_decode(fs2_engine* e, const fs2_outputs* out, void* stream) {
    if (!e || !out) return FS2_ERR_ARG;
    if (!e->encoded) return e->fail(FS2_ERR_STATE, "fs2_decode without a preceding successful fs2_encode");
    hipStream_t st = (hipStream_t)stream;
    bool plain = !e->use_graph || e->debug || e->T == 0;
    for (int v = 0; v < FS2_MAX_VARIANCES && !plain; ++v) plain = e->forced_idx[v] || e->forced_tgt[v];
    if (plain) return decode_body(e, out, st);
    // the arena may grow (device sync + hipMalloc) only outside a capture; the body's own call is then a no-op
    const char* base0 = e->scratch.base;
    FS2_TRY(ensure_arena(e, e->scratch, decode_scratch_need(e, e->B, e->T), "scratch"));
    if (e->scratch.base != base0) drop_graphs(e);
    std::vector<uint64_t> key = {(uint64_t)e->B, (uint64_t)e->L, (uint64_t)e->T, (uint64_t)e->scratch.base, (uint64_t)e->persist.base,
                                 (uint64_t)e->ps.xA, (uint64_t)e->ps.d_cum, (uint64_t)e->ps.spk,(uint64_t)e->zero_pad_mel, (uint64_t)e->fuse_predictor, (uint64_t)e->tune.gen,
                                 (uint64_t)e->defer_ln, (uint64_t)e->front_split, (uint64_t)e->fold_ln, (uint64_t)out->mel, (uint64_t)out->tgt_mask,
                                 (uint64_t)out->duration_prediction, (uint64_t)out->duration_rounded, (uint64_t)out->src_mask};
    for (int v = 0; v < FS2_MAX_VARIANCES; ++v) {
        key.push_back((uint64_t)out->variances[v]);
        key.push_back((uint64_t)out->var_mean_std[v]);
        key.push_back((uint64_t)out->var_spectrogram[v]);
    }
    const int r = run_phase(e, e->dgraphs, key, false, st, [&](hipStream_t s2) { return decode_body(e, out, s2); });
    if (r == FS2_OK) e->mid_forward = false;
    return r;
}

int fs2_set_graphs(fs2_engine* e, int32_t on) {
    if (!e) return FS2_ERR_ARG;
    e->use_graph = on != 0;
    if (!on) drop_graphs(e);
    return FS2_OK;
}

int64_t fs2_graph_replays(const fs2_engine* e) { return e ? e->graph_replays : -1; }

int fs2_force_buckets(fs2_engine* e, int32_t variance_index, const int32_t* idx) {
    if (!e || variance_index < 0 || variance_index >= e->cfg.n_variances) return FS2_ERR_ARG;
    e->forced_idx[variance_index] = idx;
    return FS2_OK;
}

int fs2_force_variance_targets(fs2_engine* e, int32_t variance_index, const float* tgt) {
    if (!e || variance_index < 0 || variance_index >= e->cfg.n_variances) return FS2_ERR_ARG;
    e->forced_tgt[variance_index] = tgt;
    return FS2_OK;
}

int fs2_debug_copy(fs2_engine* e, const char* what, void* dst, void* stream) {
    if (!e || !what || !dst) return FS2_ERR_ARG;
    auto it = e->taps.find(what);
    if (it == e->taps.end()) return e->fail(FS2_ERR_STATE, "no debug tap '%s' (fs2_set_debug before encode?)", what);
    FS2_HIP(e, hipMemcpyAsync(dst, it->second.first, it->second.second, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FS2_OK;
}

int fs2_profile_enable(fs2_engine* e, int32_t cls, int32_t enable) {
    if (!e || cls < 0 || cls >= FS2_K_COUNT) return FS2_ERR_ARG;
    ProfSlot& s = e->prof[cls];
    s.enabled = enable != 0;
    s.used = 0;
    s.flops = s.bytes = 0;
    return FS2_OK;
}

// Create the event pairs of `pairs` bracketed launches now, so that a timed region with profiling on records into existing
// events only (hipEventCreate is an ioctl that was seen to take tens of microseconds on hosts whose other GPUs are busy - 160
// of them inside bench.py's timed region turned 2.4 ms forwards into 4.5 ms ones).
int fs2_profile_reserve(fs2_engine* e, int32_t cls, int32_t pairs) {
    if (!e || cls < 0 || cls >= FS2_K_COUNT || pairs < 0) return FS2_ERR_ARG;
    ProfSlot& s = e->prof[cls];
    while ((int)s.ev.size() < pairs) {
        hipEvent_t a, b;
        FS2_HIP(e, hipEventCreate(&a));
        if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return e->fail(FS2_ERR_HIP, "hipEventCreate failed"); }
        s.ev.emplace_back(a, b);
    }
    return FS2_OK;
}

int fs2_profile_read(fs2_engine* e, int32_t cls, double* total_ms, int64_t* launches, double* flops, double* bytes) {
    if (!e || cls < 0 || cls >= FS2_K_COUNT) return FS2_ERR_ARG;
    ProfSlot& s = e->prof[cls];
    double ms = 0;
    for (size_t i = 0; i < s.used; ++i) {
        FS2_HIP(e, hipEventSynchronize(s.ev[i].second));
        float t = 0;
        FS2_HIP(e, hipEventElapsedTime(&t, s.ev[i].first, s.ev[i].second));
        ms += t;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = (int64_t)s.used;
    if (flops) *flops = s.flops;
    if (bytes) *bytes = s.bytes;
    s.used = 0;
    s.flops = s.bytes = 0;
    return FS2_OK;
}

}  // extern "C"
