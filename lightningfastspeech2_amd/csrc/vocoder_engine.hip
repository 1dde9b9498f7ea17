// HiFi-GAN generator engine behind the fs2_voc_* C ABI (include/fs2.h).
// Reference: litfass/third_party/hifigan/models.py:112-165 (Generator), :20-110 (ResBlock "1"),
// called by Synthesiser.__call__ (litfass/third_party/hifigan/__init__.py:37-43) from
// SpeechGenerator.generate_samples (litfass/synthesis/generator.py:163-170).
//
//   x = conv_pre(mel)                                              models.py:147
//   for each stage i:  x = ups[i](lrelu(x, 0.1))                   :149-150
//                      x = mean_j resblock[i, j](x)                :151-157
//       resblock: for (c1, c2): x = c2(lrelu(c1(lrelu(x)))) + x    :98-104
//   wav = tanh(conv_post(lrelu(x, 0.01)))                          :158-160  (F.leaky_relu default slope)
//
// Every conv is one launch of vocoder_conv_kernel; the LeakyReLU in front of a conv is applied
// while that conv stages its operand, the residual / the 1/3 mean over the resblocks in the epilogue
// of the conv that produces them.  ConvTranspose1d(k, stride s, padding p) with k - 2p = s:
//   y[q*s + f] = sum_m x[q - m] . Wt[:, :, m*s + f + p]   (0 <= m*s + f + p < k)
// is a plain conv of x to s*Cout channels (phase-major), whose (T, s*Cout) row-major output is the
// (T*s, Cout) tensor the next layer reads - no scatter, no zero insertion.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fs2_host.h"

using namespace fs2;

namespace {

struct VocLayer {     // one conv in kernel form
    void* w = nullptr;
    float* b = nullptr;
    int cin = 0, cin_pad = 0, n = 0, taps = 1, dil = 1, pad = 0, wn = 1;
    int shift_from = 0;  // VocConvArgs::shift_from
};

}  // namespace

struct fs2_vocoder : ErrorBase {
    fs2_voc_config cfg;
    int dt = FS2_BF16;
    size_t esz = 2;
    bool finalized = false;
    WeightStore w;
    DevAllocs allocs;
    VocLayer pre, post;
    std::vector<VocLayer> ups;
    std::vector<VocLayer> c1, c2;  // [(stage * n_kernels + j) * 3 + m]
    struct FusedRb { void* w = nullptr; float* b = nullptr; size_t conv_bytes = 0; };
    std::vector<FusedRb> rb;       // [stage * n_kernels + j]: six convs back to back (narrow stages)
    std::vector<int> chan, upf;    // channels / cumulative upsampling after stage i (index 0 = conv_pre)
    Arena ws;                      // one output per stage + 4 scratch tensors of the largest stage, laid out per synthesize
    std::vector<void*> stage_out;  // x after conv_pre and after each stage
    int lastB = 0, lastT = 0;
    std::vector<int32_t> launches;  // fs2_voc_last_launches: one code per kernel launch of the last synthesize
};

namespace {

// fp32 host values -> the generator's storage dtype (weights) or fp32 (biases) on the device
int vupload(fs2_vocoder* v, const std::vector<float>& h, int dt, void** out) {
    return upload_as(*v, v->allocs, h.data(), h.size(), dt, out, FS2_ERR_HIP);
}

int next_pow2(int x) {
    int p = 32;
    while (p < x) p <<= 1;
    return p;
}

// wave columns of a conv to n channels (n a multiple of 32; conv_post: one column)
int wave_cols(int n, bool post) {
    const int n32 = post ? 1 : n / 32;
    return (n32 % 8 == 0) ? 8 : (n32 % 4 == 0) ? 4 : (n32 % 2 == 0) ? 2 : 1;
}

// W (n, cin, taps) fp32 host (conv form: out[t] = sum_tap x[t - pad + tap*dil] . W[:, :, tap]) ->
// fragment order [n-tile][step][wn][2][64] x 16 B as fp32 staging
void frag_order(int dt, const std::vector<float>& W, int n, int cin, int cin_pad, int taps, int wn_cols, bool post,
                std::vector<float>* stage) {
    const int KE = is_16bit(dt) ? 32 : 16, e16 = 16 / (int)elem_bytes(dt);
    const int nkc = cin_pad / KE, nsteps4 = voc_steps_padded(taps, cin_pad, dt);
    const int ntiles = post ? 1 : n / (wn_cols * 32);
    const size_t nfrag = (size_t)ntiles * nsteps4 * wn_cols * 2 * 64;
    stage->assign(nfrag * e16, 0.f);
    for (int nt = 0; nt < ntiles; ++nt)
        for (int g = 0; g < taps * nkc; ++g) {
            const int tap = g / nkc, kc = g % nkc;
            for (int wn = 0; wn < wn_cols; ++wn)
                for (int ni = 0; ni < 2; ++ni)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int fr = lane & 15, fg = lane >> 4;
                        const int ch = nt * wn_cols * 32 + wn * 32 + (fr >> 2) * 8 + ni * 4 + (fr & 3);
                        if (ch >= n) continue;
                        float* dst = &(*stage)[((((size_t)nt * nsteps4 + g) * wn_cols + wn) * 2 + ni) * 64 * e16 + (size_t)lane * e16];
                        for (int e = 0; e < e16; ++e) {
                            const int c = kc * KE + fg * e16 + e;
                            if (c < cin) dst[e] = W[((size_t)ch * cin + c) * taps + tap];
                        }
                    }
        }
}

int pack_layer(fs2_vocoder* v, const std::vector<float>& W, const std::vector<float>& bias, int n, int cin, int taps,
               int dil, int pad, bool post, VocLayer* L) {
    L->cin = cin;
    L->cin_pad = next_pow2(cin);
    L->n = n;
    L->taps = taps;
    L->dil = dil;
    L->pad = pad;
    if (!post && n % 32) return v->fail(FS2_ERR_SHAPE, "channel count %d is not a multiple of 32", n);
    L->wn = wave_cols(n, post);
    std::vector<float> stage;
    frag_order(v->dt, W, n, cin, L->cin_pad, taps, L->wn, post, &stage);
    FS2_TRY(vupload(v, stage, v->dt, &L->w));
    std::vector<float> bp(post ? 32 : n, 0.f);
    for (size_t i = 0; i < bias.size() && i < bp.size(); ++i) bp[i] = bias[i];
    return vupload(v, bp, FS2_F32, (void**)&L->b);
}

int conv_layer(fs2_vocoder* v, const std::string& name, int n, int cin, int k, int dil, bool post, VocLayer* L) {
    const auto& w = v->w.at(name + ".weight");
    const auto& b = v->w.at(name + ".bias");
    return pack_layer(v, w.data, b.data, n, cin, k, dil, (k - 1) / 2 * dil, post, L);
}

// ConvTranspose1d weight (cin, cout, k), stride s, padding p  ->  conv form (s*cout, cin, K)
int up_layer(fs2_vocoder* v, const std::string& name, int cin, int cout, int k, int s, VocLayer* L) {
    const auto& w = v->w.at(name + ".weight");
    const auto& b = v->w.at(name + ".bias");
    const int p = (k - s) / 2;
    if (k - 2 * p != s) return v->fail(FS2_ERR_SHAPE, "%s: kernel %d / stride %d: kernel - 2*padding must equal the stride", name.c_str(), k, s);
    int m_lo = 1 << 30, m_hi = -(1 << 30);
    for (int f = 0; f < s; ++f)
        for (int m = -k; m <= k; ++m) {
            const int kk = m * s + f + p;
            if (kk >= 0 && kk < k) { m_lo = m < m_lo ? m : m_lo; m_hi = m > m_hi ? m : m_hi; }
        }
    const int K = m_hi - m_lo + 1, pad = m_hi;  // tap j reads x[q - pad + j]  <->  m = pad - j
    // A phase f only has the taps with 0 <= (pad - j)*s + f + p < k.  With k = 2s (every HiFi-GAN config) that is two of
    // the K = 3: j in {0, 1} for f < s/2, {1, 2} above - the kernel runs K - 1 taps and reads one row further on for
    // the channels from shift_from upwards (a wave column is 32 channels, cout a multiple of 32) instead of
    // multiplying a third of its steps by zeros.
    std::vector<int> jlo(s, K), jhi(s, -1);
    for (int f = 0; f < s; ++f)
        for (int j = 0; j < K; ++j) {
            const int kk = (pad - j) * s + f + p;
            if (kk >= 0 && kk < k) { jlo[f] = j < jlo[f] ? j : jlo[f]; jhi[f] = j > jhi[f] ? j : jhi[f]; }
        }
    int fshift = s;  // first phase whose window starts at tap 1
    bool two = K >= 2;
    for (int f = 0; f < s && two; ++f) {
        if (jlo[f] > 1 || jhi[f] - (jlo[f] >= 1 ? 1 : 0) > K - 2) two = false;
        if (jlo[f] >= 1 && fshift == s) fshift = f;
        if (jlo[f] < 1 && fshift != s) two = false;  // one switch point only
    }
    const int K2 = two ? K - 1 : K;
    std::vector<float> W((size_t)s * cout * cin * K2, 0.f), bias((size_t)s * cout);
    for (int f = 0; f < s; ++f)
        for (int co = 0; co < cout; ++co) {
            bias[(size_t)f * cout + co] = b.data[co];
            for (int j2 = 0; j2 < K2; ++j2) {
                const int j = j2 + (two && f >= fshift ? 1 : 0);
                const int kk = (pad - j) * s + f + p;
                if (kk < 0 || kk >= k) continue;
                for (int ci = 0; ci < cin; ++ci)
                    W[(((size_t)f * cout + co) * cin + ci) * K2 + j2] = w.data[((size_t)ci * cout + co) * k + kk];
            }
        }
    FS2_TRY(pack_layer(v, W, bias, s * cout, cin, K2, 1, pad, false, L));
    L->shift_from = two && fshift < s ? fshift * cout : 0;
    return FS2_OK;
}

int run_conv(fs2_vocoder* v, hipStream_t st, const VocLayer& L, const void* x, void* out, const void* res,
             const int32_t* lengths, int len_scale, int B, int S, float in_slope, float scale, bool accumulate,
             bool in_fp32 = false, bool post = false, float out_slope = 1.f) {
    VocConvArgs a;
    a.tune = &op_tuning();  // the calling thread's A/B switches (fs2_op_set_vocoder_*)
    a.out_slope = out_slope;
    a.x = x; a.w = L.w; a.bias = L.b; a.res = res; a.out = out; a.lengths = lengths; a.len_scale = len_scale;
    a.B = B; a.S = S; a.cin = L.cin; a.cin_pad = L.cin_pad; a.n = L.n; a.taps = L.taps; a.dil = L.dil; a.pad = L.pad;
    a.wn = L.wn; a.in_slope = in_slope; a.scale = scale; a.accumulate = accumulate ? 1 : 0;
    a.in_fp32 = in_fp32 ? 1 : 0; a.post = post ? 1 : 0;
    a.shift_from = L.shift_from;
    int32_t code = -1;
    const int r = launch_vocoder_conv(a, v->dt, st, &code);
    if (code >= 0) v->launches.push_back(code);
    if (r != FS2_OK) return v->fail(r, "vocoder conv launch failed (cin=%d n=%d k=%d dil=%d S=%d)", L.cin, L.n, L.taps, L.dil, S);
    return FS2_OK;
}

// The resident launch of resblock j of stage i: the whole block (m < 0) or its pair m.  The last pair, and so the whole block, adds
// (xt + x) / n_kernels into the stage output; an earlier pair hands x on as it is.  With the defaults: the shape alone, which is
// all voc_resblock_mi16 reads.
VocResblockArgs rb_args(const fs2_vocoder* v, int i, int j, int m, const int32_t* lengths = nullptr, int B = 0, int T = 0,
                        const void* x = nullptr, void* out = nullptr, bool x_act = false, bool out_act = false) {
    const fs2_voc_config& c = v->cfg;
    const fs2_vocoder::FusedRb& f = v->rb[(size_t)i * c.n_kernels + j];
    const int first = m < 0 ? 0 : m;
    const bool last = m < 0 || m == 2;
    VocResblockArgs a{};
    a.tune = &op_tuning();  // the calling thread's A/B switches
    a.x = x; a.out = out; a.lengths = lengths; a.len_scale = v->upf[i + 1];
    a.B = B; a.S = T * v->upf[i + 1]; a.C = v->chan[i + 1]; a.taps = c.rb_kernels[j]; a.wn = a.C / 32; a.npairs = m < 0 ? 3 : 1;
    a.w = (const char*)f.w + f.conv_bytes * 2 * first;
    a.bias = f.b + (size_t)2 * first * a.C;
    for (int q = 0; q < 3; ++q) a.dil[q] = c.rb_dilations[j][q];
    a.dil[0] = c.rb_dilations[j][first];
    a.slope = 0.1f; a.scale = last ? 1.0f / (float)c.n_kernels : 1.f; a.accumulate = last && j > 0 ? 1 : 0;
    a.x_act = x_act ? 1 : 0; a.out_act = out_act ? 1 : 0;
    return a;
}

int run_resblock(fs2_vocoder* v, hipStream_t st, const VocResblockArgs& a) {
    int32_t code = -1;
    const int r = launch_vocoder_resblock(a, v->dt, st, &code);
    if (code >= 0) v->launches.push_back(code);
    if (r != FS2_OK) return v->fail(r, "fused %s launch failed (C=%d k=%d)", a.npairs == 3 ? "resblock" : "conv pair", a.C, a.taps);
    return FS2_OK;
}

// How a resblock runs: in one resident launch (`whole`), else pair by pair, pair m on an LDS-resident tile where it fits and pays
// (`pair[m]`) and as two plain convs otherwise.  Each entry is a form of voc_resblock_mi16 (408 / 808 / 804) or 0.
struct BlockForm {
    int whole = 0, pair[3] = {0, 0, 0};
    bool resident() const { return whole || (pair[0] && pair[1] && pair[2]); }
};

// ... of resblock j of stage i, for the calling thread's knobs.  A block that fs2_voc_finalize did not pack (a wide stage) has no
// resident form; the pairs are asked only when the whole block is refused.
BlockForm block_form(const fs2_vocoder* v, int i, int j) {
    BlockForm f;
    if (!v->rb[(size_t)i * v->cfg.n_kernels + j].w) return f;
    f.whole = voc_resblock_mi16(rb_args(v, i, j, -1), v->dt);
    for (int m = 0; m < 3 && !f.whole; ++m) f.pair[m] = voc_resblock_mi16(rb_args(v, i, j, m), v->dt);
    return f;
}

}  // namespace

extern "C" {

int fs2_voc_create(const fs2_voc_config* cfg, fs2_vocoder** out) {
    if (!cfg || !out) return FS2_ERR_ARG;
    *out = nullptr;
    if (cfg->abi_version != FS2_ABI_VERSION) return FS2_ERR_ARG;
    if (cfg->n_stages < 1 || cfg->n_stages > FS2_VOC_MAX_STAGES || cfg->n_kernels < 1 || cfg->n_kernels > FS2_VOC_MAX_KERNELS)
        return FS2_ERR_SHAPE;
    if (cfg->n_mels < 4 || cfg->n_mels % 4 || (cfg->initial_channel >> cfg->n_stages) % 32) return FS2_ERR_SHAPE;
    if (!is_storage_dtype(cfg->dtype)) return FS2_ERR_ARG;  // FS2_F32, FS2_BF16 or FS2_F16: the engine modes are not storage types
    std::unique_ptr<fs2_vocoder> v(new fs2_vocoder());
    v->cfg = *cfg;
    v->dt = cfg->dtype;
    v->esz = elem_bytes(cfg->dtype);
    const int C0 = cfg->initial_channel;
    v->w.expect("conv_pre.weight", {C0, cfg->n_mels, 7});
    v->w.expect("conv_pre.bias", {C0});
    v->chan.push_back(C0);
    v->upf.push_back(1);
    for (int i = 0; i < cfg->n_stages; ++i) {
        const int cin = C0 >> i, cout = C0 >> (i + 1);
        if (cfg->up_rates[i] < 1 || cfg->up_kernels[i] < cfg->up_rates[i]) return FS2_ERR_SHAPE;
        const std::string u = "ups." + std::to_string(i);
        v->w.expect(u + ".weight", {cin, cout, cfg->up_kernels[i]});
        v->w.expect(u + ".bias", {cout});
        v->chan.push_back(cout);
        v->upf.push_back(v->upf.back() * cfg->up_rates[i]);
        for (int j = 0; j < cfg->n_kernels; ++j) {
            const int k = cfg->rb_kernels[j];
            if (k < 1 || !(k & 1)) return FS2_ERR_SHAPE;
            const std::string r = "resblocks." + std::to_string(i * cfg->n_kernels + j);
            for (int m = 0; m < 3; ++m) {
                v->w.expect(r + ".convs1." + std::to_string(m) + ".weight", {cout, cout, k});
                v->w.expect(r + ".convs1." + std::to_string(m) + ".bias", {cout});
                v->w.expect(r + ".convs2." + std::to_string(m) + ".weight", {cout, cout, k});
                v->w.expect(r + ".convs2." + std::to_string(m) + ".bias", {cout});
            }
        }
    }
    v->w.expect("conv_post.weight", {1, v->chan.back(), 7});
    v->w.expect("conv_post.bias", {1});
    *out = v.release();
    return FS2_OK;
}

void fs2_voc_destroy(fs2_vocoder* v) {
    if (!v) return;
    v->ws.release();
    delete v;
}

const char* fs2_voc_last_error(const fs2_vocoder* v) { return v ? v->err : "null vocoder"; }

int fs2_voc_load_weight(fs2_vocoder* v, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!v || !name || !data || !shape) return v ? v->fail(FS2_ERR_ARG, "bad load_weight argument") : FS2_ERR_ARG;
    if (v->finalized) return v->fail(FS2_ERR_STATE, "weights are frozen after fs2_voc_finalize");
    return v->w.load(*v, name, data, shape, ndim);
}

int fs2_voc_finalize(fs2_vocoder* v) {
    if (!v) return FS2_ERR_ARG;
    if (v->finalized) return FS2_OK;
    if (const char* missing = v->w.first_missing()) return v->fail(FS2_ERR_WEIGHT, "missing weight '%s'", missing);
    const fs2_voc_config& c = v->cfg;
    FS2_TRY(conv_layer(v, "conv_pre", c.initial_channel, c.n_mels, 7, 1, false, &v->pre));
    v->ups.resize(c.n_stages);
    v->c1.resize((size_t)c.n_stages * c.n_kernels * 3);
    v->c2.resize(v->c1.size());
    for (int i = 0; i < c.n_stages; ++i) {
        const int cin = v->chan[i], cout = v->chan[i + 1];
        FS2_TRY(up_layer(v, "ups." + std::to_string(i), cin, cout, c.up_kernels[i], c.up_rates[i], &v->ups[i]));
        for (int j = 0; j < c.n_kernels; ++j) {
            const std::string r = "resblocks." + std::to_string(i * c.n_kernels + j);
            for (int m = 0; m < 3; ++m) {
                const size_t idx = ((size_t)i * c.n_kernels + j) * 3 + m;
                FS2_TRY(conv_layer(v, r + ".convs1." + std::to_string(m), cout, cout, c.rb_kernels[j], c.rb_dilations[j][m], false, &v->c1[idx]));
                FS2_TRY(conv_layer(v, r + ".convs2." + std::to_string(m), cout, cout, c.rb_kernels[j], 1, false, &v->c2[idx]));
            }
        }
    }
    FS2_TRY(conv_layer(v, "conv_post", 1, v->chan.back(), 7, 1, true, &v->post));
    // narrow stages: the six convs of a resblock back to back for the LDS-resident kernel
    v->rb.resize((size_t)c.n_stages * c.n_kernels);
    for (int i = 0; i < c.n_stages; ++i) {
        const int C = v->chan[i + 1];
        if (C != 32 && C != 64 && C != 128) continue;
        for (int j = 0; j < c.n_kernels; ++j) {
            const std::string r = "resblocks." + std::to_string(i * c.n_kernels + j);
            std::vector<float> all, bias;
            for (int m = 0; m < 3; ++m)
                for (const char* grp : {".convs1.", ".convs2."}) {
                    const auto& w = v->w.at(r + grp + std::to_string(m) + ".weight");
                    const auto& b = v->w.at(r + grp + std::to_string(m) + ".bias");
                    std::vector<float> st;
                    frag_order(v->dt, w.data, C, C, C, c.rb_kernels[j], C / 32, false, &st);
                    all.insert(all.end(), st.begin(), st.end());
                    bias.insert(bias.end(), b.data.begin(), b.data.end());
                }
            fs2_vocoder::FusedRb& f = v->rb[(size_t)i * c.n_kernels + j];
            f.conv_bytes = all.size() / 6 * v->esz;
            FS2_TRY(vupload(v, all, v->dt, &f.w));
            FS2_TRY(vupload(v, bias, FS2_F32, (void**)&f.b));
        }
    }
    v->w.drop();
    v->finalized = true;
    return FS2_OK;
}

int32_t fs2_voc_hop(const fs2_vocoder* v) { return v ? v->upf.back() : 0; }

int fs2_voc_synthesize(fs2_vocoder* v, const float* mel, const int32_t* lengths, int32_t B, int32_t T, float* wav,
                       void* stream) {
    if (!v || !mel || !wav || B <= 0 || T <= 0) return v ? v->fail(FS2_ERR_ARG, "bad synthesize argument") : FS2_ERR_ARG;
    if (!v->finalized) return v->fail(FS2_ERR_STATE, "fs2_voc_finalize not called");
    hipStream_t st = (hipStream_t)stream;
    const fs2_voc_config& c = v->cfg;
    const int ns = c.n_stages;
    // workspace: one output per stage (kept for the parity taps) + 4 scratch tensors of the largest stage
    size_t need = 0, big = 0;
    std::vector<size_t> sb(ns + 1);
    for (int i = 0; i <= ns; ++i) {
        sb[i] = al((size_t)B * T * v->upf[i] * v->chan[i] * v->esz);
        need += sb[i];
        if (i > 0 && sb[i] > big) big = sb[i];
    }
    need += 4 * big;
    if ((size_t)T * v->upf.back() > (size_t)0x7fffffff / 4) return v->fail(FS2_ERR_SHAPE, "T too large");
    if (need > v->ws.cap) FS2_HIP(v, hipStreamSynchronize(st));  // it grows: the last pass may still use the block about to be freed
    if (v->ws.reserve(need) != FS2_OK) return v->fail(FS2_ERR_NOMEM, "workspace of %zu bytes", need);
    v->stage_out.assign(ns + 1, nullptr);
    for (int i = 0; i <= ns; ++i) v->stage_out[i] = v->ws.take(sb[i]);
    void* u = v->ws.take(big);
    void* a = v->ws.take(big);
    void* r1 = v->ws.take(big);
    void* r2 = v->ws.take(big);
    v->lastB = B;
    v->lastT = T;
    v->launches.clear();

    FS2_TRY(run_conv(v, st, v->pre, mel, v->stage_out[0], nullptr, lengths, 1, B, T, 1.f, 1.f, false, /*in_fp32=*/true));
    const float inv = 1.0f / (float)c.n_kernels;
    // a stream between two resident launches travels as lrelu(x) (x_act / out_act below); knob 9 keeps every stream raw
    const bool act = op_tuning().voc_fused_resblock != 9;
    for (int i = 0; i < ns; ++i) {
        const int S = T * v->upf[i + 1], sc = v->upf[i + 1];
        // when every resblock of this stage runs on LDS-resident tiles, the upsampled stream travels as lrelu(x):
        // all its consumers then fill their slabs by plain LDS-DMA (x_act, vocoder_resblock.hip)
        BlockForm form[FS2_VOC_MAX_KERNELS];
        bool stage_act = act;
        for (int j = 0; j < c.n_kernels; ++j) {
            form[j] = block_form(v, i, j);
            stage_act = stage_act && form[j].resident();
        }
        // transposed conv, at the INPUT resolution, to up_rate * Cout phase-major channels
        FS2_TRY(run_conv(v, st, v->ups[i], v->stage_out[i], u, nullptr, lengths, v->upf[i], B, T * v->upf[i], 0.1f, 1.f, false, false,
                      false, stage_act ? 0.1f : 1.f));
        for (int j = 0; j < c.n_kernels; ++j) {
            const BlockForm& f = form[j];
            if (f.whole) {  // the whole block in one launch
                FS2_TRY(run_resblock(v, st, rb_args(v, i, j, -1, lengths, B, T, u, v->stage_out[i + 1], stage_act)));
                continue;
            }
            // else pair by pair: a (c1, c2) pair on an LDS-resident tile where it fits and pays, two plain convs otherwise
            // (always, in a stage too wide to be packed)
            const void* rin = u;
            bool x_act = stage_act;
            for (int m = 0; m < 3; ++m) {
                void* o = m == 0 ? r1 : (m == 1 ? r2 : v->stage_out[i + 1]);
                // between two resident pairs the residual stream travels as lrelu(x): the consumer's slab fill is
                // then a plain LDS-DMA copy and it recovers x by the inverse map it applies anyway
                const bool out_act = act && m < 2 && f.pair[m] && f.pair[m + 1];
                if (f.pair[m]) {
                    FS2_TRY(run_resblock(v, st, rb_args(v, i, j, m, lengths, B, T, rin, o, x_act, out_act)));
                } else {
                    const size_t idx = ((size_t)i * c.n_kernels + j) * 3 + m;
                    // c1 stores lrelu(out): c2 then stages it untouched (LDS-DMA fill in vocoder_conv.hip)
                    FS2_TRY(run_conv(v, st, v->c1[idx], rin, a, nullptr, lengths, sc, B, S, 0.1f, 1.f, false, false, false, 0.1f));
                    // last pair of the block: (xt + x) / n_kernels summed into the stage output
                    FS2_TRY(run_conv(v, st, v->c2[idx], a, o, rin, lengths, sc, B, S, 1.f, m < 2 ? 1.f : inv, m == 2 && j > 0));
                }
                rin = o;
                x_act = out_act;
            }
        }
    }
    FS2_TRY(run_conv(v, st, v->post, v->stage_out[ns], wav, nullptr, lengths, v->upf[ns], B, T * v->upf[ns], 0.01f, 1.f, false,
                  false, /*post=*/true));
    return FS2_OK;
}

int fs2_voc_debug_copy(fs2_vocoder* v, int32_t stage, float* dst, void* stream) {
    if (!v || !dst) return FS2_ERR_ARG;
    if (stage < 0 || stage > v->cfg.n_stages || v->stage_out.empty()) return v->fail(FS2_ERR_STATE, "no such stage output");
    const size_t n = (size_t)v->lastB * v->lastT * v->upf[stage] * v->chan[stage];
    ConvertArgs a{v->stage_out[stage], dst, n};
    const int r = launch_convert(a, v->dt, FS2_F32, (hipStream_t)stream);
    if (r != FS2_OK) return v->fail(r, "convert failed");
    return FS2_OK;
}

int32_t fs2_voc_last_launches(const fs2_vocoder* v, int32_t* codes, int32_t cap) {
    if (!v || cap < 0 || (cap > 0 && !codes)) return -FS2_ERR_ARG;
    const size_t n = v->launches.size();
    for (size_t i = 0; i < n && i < (size_t)cap; ++i) codes[i] = v->launches[i];
    return (int32_t)n;
}

int32_t fs2_op_vocoder_resblock_form(int32_t dtype, int32_t channels, int32_t taps, const int32_t* dilations, int32_t npairs) {
    if (!is_storage_dtype(dtype) || !dilations || (npairs != 1 && npairs != 3) || channels <= 0 || taps <= 0) return -FS2_ERR_ARG;
    VocResblockArgs a{};
    a.C = channels; a.taps = taps; a.wn = channels / 32; a.npairs = npairs;
    for (int m = 0; m < npairs; ++m) {
        if (dilations[m] < 1) return -FS2_ERR_ARG;
        a.dil[m] = dilations[m];
    }
    a.tune = &op_tuning();
    return voc_resblock_mi16(a, dtype);
}

int32_t fs2_op_vocoder_conv_tile(int32_t dtype, int32_t n, int32_t cin, int32_t taps, int32_t dil, int32_t shift, int32_t post,
                                 int32_t* cin_pad) {
    if (!is_storage_dtype(dtype) || n <= 0 || cin <= 0 || taps <= 0 || dil <= 0 || (!post && n % 32)) return -FS2_ERR_ARG;
    VocConvArgs a{};
    a.cin = cin; a.cin_pad = next_pow2(cin); a.n = n; a.taps = taps; a.dil = dil;
    a.wn = wave_cols(n, post != 0); a.post = post ? 1 : 0; a.shift_from = shift ? 32 : 0;
    a.tune = &op_tuning();
    if (cin_pad) *cin_pad = a.cin_pad;
    size_t smem = 0;
    return voc_pick_mi16(a, (int)elem_bytes(dtype), &smem);
}

}  // extern "C"
