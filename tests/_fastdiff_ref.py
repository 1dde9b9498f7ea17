"""CPU restatement of FastDiff at inference, written from the definition (litfass/third_party/fastdiff/FastDiff.py:120-135,
149-195; module/modules.py:127-138, 190-253, 320-343; module/util.py:187-231, 318-343) for ONE utterance, in the dtype asked for:
float64 is the truth the device is judged against, float32 the equal-precision yardstick.

``rnd``: an optional storage-rounding hook applied exactly where the engine's bf16 mode stores a value (csrc/fastdiff.hip):
the packed MFMA conv weights (everything but first_audio_conv, final_conv and the fc_t* linears), the conditioning mel + offset,
every MFMA conv's operand after its input LeakyReLU, every stream a launch writes (conv outputs after bias / adds / output LeakyReLU,
the predicted kernels and biases, x after each LVC layer's gate, residual and the next layer's audio_down add).  The gate, the
diffusion state, eps and the sampler stay in the working dtype."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

RESIDUAL_IDX = (1, 3, 6, 8, 11, 13)
RATIOS = (8, 8, 4)
HOPS = (8, 64, 256)
DOWN = (4, 8, 8)
_UNROUNDED = ("first_audio_conv.", "final_conv.", "fc_t1.", "fc_t2.")


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


class FastDiffRef:
    def __init__(self, sd, dtype=torch.float64, rnd=None):
        self.dtype, self.rnd = dtype, (rnd or (lambda t: t))
        self.w = {}
        for k, v in sd.items():
            t = torch.as_tensor(np.asarray(v)).to(dtype)
            if rnd is not None and k.endswith(".weight") and not k.startswith(_UNROUNDED) and ".fc_t." not in k:
                t = rnd(t)
            self.w[k] = t

    # ---- pieces ----
    def conv(self, x, name, dil=1, in_slope=None, out_slope=None, add1=None, add2=None):
        """x (C, S) -> (N, S): Conv1d with 'same' zero padding; operand and result rounded where the engine stores"""
        w, b = self.w[name + ".weight"], self.w[name + ".bias"]
        if in_slope is not None:
            x = self.rnd(lrelu(x, in_slope))
        y = F.conv1d(x[None], w, b, padding=dil * (w.shape[2] - 1) // 2, dilation=dil)[0]
        if add1 is not None:
            y = y + add1
        if out_slope is not None:
            y = lrelu(y, out_slope)
        if add2 is not None:
            y = y + add2
        return self.rnd(y)

    def step_offsets(self, step):
        """fc_t(swish(fc_t2(swish(fc_t1(emb(step)))))) per LVC block: three (80,) vectors"""
        w = self.w
        f = torch.exp(torch.arange(64).to(self.dtype) * -(np.log(10000) / 63))
        e = torch.as_tensor(float(step)).to(self.dtype) * f
        emb = torch.cat((torch.sin(e), torch.cos(e)))
        h = F.linear(emb, w["fc_t1.weight"], w["fc_t1.bias"])
        h = h * torch.sigmoid(h)
        h = F.linear(h, w["fc_t2.weight"], w["fc_t2.bias"])
        h = h * torch.sigmoid(h)
        return [F.linear(h, w[f"lvc_blocks.{n}.fc_t.weight"], w[f"lvc_blocks.{n}.fc_t.bias"]) for n in range(3)]

    def dblock(self, n, x):
        """DiffusionDBlock n: x (32, S) -> (32, S / f); nearest-neighbour down-sampling of a multiple of f = every f-th sample"""
        f, p = DOWN[n], f"downsample.{n}"
        res = self.conv(x, p + ".residual_dense")[:, ::f]
        h = x[:, ::f]
        h = self.conv(h, p + ".conv.0", 1, in_slope=0.2)
        h = self.conv(h, p + ".conv.1", 2, in_slope=0.2)
        return self.conv(h, p + ".conv.2", 4, in_slope=0.2, add1=res)

    def predict(self, n, cond):
        """cond (80, T) -> kernels (4, 32, 64, 3, T) and bias (4, 64, T) in the reference's order"""
        p = f"lvc_blocks.{n}.kernel_predictor"
        c = self.conv(self.rnd(cond), p + ".input_conv.0", out_slope=0.1)
        h = c
        for j, i in enumerate(RESIDUAL_IDX):
            h = self.conv(h, p + f".residual_conv.{i}", out_slope=0.1, add2=c if j == 5 else None)
        T = cond.shape[1]
        return self.conv(h, p + ".kernel_conv").view(4, 32, 64, 3, T), self.conv(h, p + ".bias_conv").view(4, 64, T)

    @staticmethod
    def lvc(y, k, b, hop):
        """y (32, S), k (32, 64, 3, T), b (64, T) -> o (64, S): o[:, t] = b[:, l] + sum_{c, j} y[c, t + j - 1] k[c, :, j, l], l = t // hop;
        neighbours across a frame border are the real samples, zero only outside the utterance"""
        C, S = y.shape
        T = S // hop
        yp = F.pad(y, (1, 1))
        o = b[:, :, None].expand(64, T, hop).clone()
        for j in range(3):
            o = o + torch.einsum("clh,col->olh", yp[:, j:j + S].reshape(C, T, hop), k[:, :, j, :])
        return o.reshape(64, S)

    def lvc_block(self, n, x, audio_down, cond):
        p = f"lvc_blocks.{n}"
        r = RATIOS[n]
        kernels, bias = self.predict(n, cond)
        xin = self.rnd(lrelu(x, 0.2))
        x = F.conv_transpose1d(xin[None], self.w[p + ".upsample.weight"], self.w[p + ".upsample.bias"], stride=r, padding=r // 2)[0]
        x = self.rnd(x + audio_down)  # `x += audio_down` of layer 0
        for i in range(4):
            y = self.conv(x, p + f".convs.{i}", 3 ** i, in_slope=0.2, out_slope=0.2)
            o = self.lvc(y, kernels[i], bias[i], HOPS[n])
            x = x + torch.sigmoid(o[:32]) * torch.tanh(o[32:])
            if i < 3:
                x = x + audio_down  # the next layer's `x += audio_down`
            x = self.rnd(x)
        return x

    # ---- the network and the sampler ----
    def eps(self, x, mel, step):
        """x (S,), mel (T, 80), step -> eps (S,)"""
        x = x.to(self.dtype)
        mel_c = mel.to(self.dtype).t().contiguous()
        offs = self.step_offsets(step)
        w = self.w
        h = self.rnd(F.conv1d(x[None, None], w["first_audio_conv.weight"], w["first_audio_conv.bias"], padding=3)[0])
        saved = []
        for n in range(3):
            saved.append(h)
            h = self.dblock(n, h)
        for n in range(3):
            h = self.lvc_block(n, h, saved[2 - n], mel_c + offs[n][:, None])
        return F.conv1d(h[None], w["final_conv.0.weight"], w["final_conv.0.bias"], padding=3)[0, 0]

    def inference(self, mel, noise, schedule):
        """mel (T, 80); noise: [x_T, z of step N-1, ..., z of step 1], each (S,); schedule: beta / alpha / sigma / steps of
        lightningfastspeech2_amd.fastdiff.inference_schedule (float32 values) -> the peak-normalised waveform (S,)"""
        beta, alpha, sigma, steps = (schedule[k].to(self.dtype) for k in ("beta", "alpha", "sigma", "steps"))
        N = len(beta)
        x = noise[0].to(self.dtype).clone()
        for n in range(N - 1, -1, -1):
            e = self.eps(x, mel, float(schedule["steps"][n]))
            x = x - beta[n] / torch.sqrt(1 - alpha[n] ** 2.) * e
            x = x / torch.sqrt(1 - beta[n])
            if n > 0:
                x = x + sigma[n] * noise[N - n].to(self.dtype)
        return x / x.abs().max()


def lvc_op_inputs(hop, lengths, T, seed=None, bf16=False):
    """y, x, add (B, T*hop, 32), K (B, T, 4, 32, 64, 3) in the reference's order and bias (B, T, 4, 64) of the fs2_op_lvc tests,
    float32; ``bf16``: rounded to bf16 values, so that they are exact in float32, float64 and on the device alike"""
    rs = np.random.RandomState(hop if seed is None else seed)
    B, S = len(lengths), T * hop
    y, x, add = (rs.standard_normal((B, S, 32)) for _ in range(3))
    K = rs.standard_normal((B, T, 4, 32, 64, 3)) * (1 / 96) ** 0.5
    bias = rs.standard_normal((B, T, 4, 64)) * 0.3
    arrs = [a.astype(np.float32) for a in (y, x, add, K, bias)]
    return [bf16_round(torch.as_tensor(a)).numpy() for a in arrs] if bf16 else arrs


def lvc_op_ref(inputs, b, frames, hop, layer, dtype):
    """utterance b of the fs2_op_lvc launch in ``dtype``: x + sigmoid(o[:32]) * tanh(o[32:]) without and with ``add``, each
    (frames * hop, 32) in ``dtype`` (the caller casts: a float32 result is the yardstick AND what a bf16 store would round)"""
    y, x, add, K, bias = inputs
    n = frames * hop
    t = lambda a: torch.as_tensor(a).to(dtype)
    o = FastDiffRef.lvc(t(y[b, :n].T), t(K[b, :frames, layer]).permute(1, 2, 3, 0), t(bias[b, :frames, layer].T), hop)
    v = t(x[b, :n].T) + torch.sigmoid(o[:32]) * torch.tanh(o[32:])
    return v.T.contiguous(), (v + t(add[b, :n].T)).T.contiguous()


def bf16_elementwise_excess(got, truth, yard, margin):
    """The elementwise rule for ONE round-to-nearest bf16 store of a float32 evaluation:
    |got - truth| <= 2^-8 |truth| + margin * max(yard, 2^-23 max|truth|), 2^-8 = bf16's unit roundoff (8 significand bits), yard = the
    float32 restatement's own max error.  Returns max over elements of (error - bound): <= 0 passes."""
    truth = np.asarray(truth, np.float64)
    bound = 2.0 ** -8 * np.abs(truth) + margin * max(yard, 2.0 ** -23 * float(np.abs(truth).max()))
    return float((np.abs(np.asarray(got, np.float64) - truth) - bound).max())


def fixture_mels(seed, frames):
    """The synthetic mels of the fixtures: standard normal, (frames_i, 80) float32 each, numpy RandomState"""
    rs = np.random.RandomState(seed)
    return [rs.standard_normal((f, 80)).astype(np.float32) for f in frames]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fastdiff")


@functools.lru_cache(maxsize=None)
def fixture(name):
    """tests/golden/fastdiff/fastdiff_<name>.npz (tools/gen_golden_fastdiff.py) as a dict, ``meta`` decoded"""
    z = np.load(os.path.join(GOLDEN, f"fastdiff_{name}.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


@functools.lru_cache(maxsize=None)
def weights(seed=0):
    """the fixtures' weights, regenerated from the seed (about a second), shared by every test"""
    from lightningfastspeech2_amd.fastdiff import FastDiffConfig, synth_state_dict
    return synth_state_dict(FastDiffConfig(), seed)


def schedule(fx, N):
    return {k: torch.as_tensor(fx[f"sched{N}_{k}"]) for k in ("beta", "alpha", "sigma", "steps")}
