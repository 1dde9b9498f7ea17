"""duration_stochastic=True end to end on the device: FastSpeech2.__call__(batch, inference=True) of a model whose duration predictor
is the spline-flow predictor (dense_small at its own width, hidden 64, with duration_filter_size 256 and two flows), against
tests/golden/sdp/e2e_dense_small.npz - what the unmodified reference forward returned under
torch.manual_seed (tools/gen_golden_sdp.py).

Bars: duration_rounded and the masks equal (the generator refuses near-integer exp(logw)); duration_prediction within 4 e_ref of the
float64 run, e_ref = the reference's own float32 error on this fixture (tests/test_gpu_sdp.py); mel <= 1e-3 over all entries, the
project's standing fp32 bar.  bf16 / mixed3 are held to their existing bars under the fp32 engine's decisions."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _sdp_ref as R
from _golden import Golden
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.model import FastSpeech2
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdp")
MEL_TOL_FP32 = 1e-3
BF16_MEL_MAX, BF16_MEL_MEAN = 0.06, 0.008  # tests/test_gpu_forward.py: the 16-bit decoder's bars under fixed decisions
FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "e2e_dense_small.npz"))
    cfg = Fs2Config.from_json(str(z["config_json"]))
    sd = synth_state_dict(cfg, **json.loads(str(z["synth_json"])))
    assert R.digest({k: v for k, v in sd.items() if not k.endswith((".pe", ".bins"))}) == str(z["sha256"]), "recipe drifted"
    return cfg, sd, json.loads(str(z["recipe_json"])), {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def model(precision="fp32"):
    cfg, sd, _, _ = fixture()
    return FastSpeech2(cfg, sd, precision=precision, device="cuda:0")


def batch_of(z, **extra):
    return {"phones": torch.from_numpy(z["phones"]), "speaker": torch.from_numpy(z["speaker"]), **extra}


def cpu(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


def check_against_fixture(out, z):
    for k in ("duration_rounded", "src_mask", "tgt_mask"):
        assert np.array_equal(out[k], z[k]), k
    e_ref = float(np.abs(z["duration_prediction"] - z["logw64"]).max())
    err = float(np.abs(out["duration_prediction"] - z["logw64"]).max())
    mel = float(np.abs(out["mel"] - z["mel"]).max())
    print(f"sdp e2e: duration_prediction error {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}; mel max-abs {mel:.3e}")
    assert err <= FACTOR * e_ref
    assert out["mel"].shape == z["mel"].shape and mel <= MEL_TOL_FP32


def test_fp32_matches_the_reference_under_its_seed():
    cfg, sd, rc, z = fixture()
    m = model()
    assert m.hparams.duration_stochastic is True and m.duration_noise_scale == 1.0
    torch.manual_seed(rc["torch_seed"])
    out = cpu(m(batch_of(z), inference=True))
    check_against_fixture(out, z)
    torch.manual_seed(rc["torch_seed"])
    again = cpu(m(batch_of(z), inference=True))  # one draw per call, after nothing else has drawn
    assert all(np.array_equal(out[k], again[k]) for k in out)


def test_fp32_with_the_noise_handed_in():
    cfg, sd, rc, z = fixture()
    m = model()
    torch.manual_seed(12345)  # must not matter
    out = cpu(m(batch_of(z, duration_noise=torch.from_numpy(z["noise"])), inference=True))
    check_against_fixture(out, z)
    dev = cpu(m(batch_of(z, duration_noise=torch.from_numpy(z["noise"]).cuda()), inference=True))
    assert all(np.array_equal(out[k], dev[k]) for k in out)
    # the scale applies to the model's own draw: sigma = 0 leaves the affine of a zero noise, equal for every seed
    m.duration_noise_scale = 0.0
    try:
        a, b = cpu(m(batch_of(z), inference=True)), cpu(m(batch_of(z), inference=True))
    finally:
        m.duration_noise_scale = 1.0
    assert np.array_equal(a["duration_prediction"], b["duration_prediction"])
    with pytest.raises(ValueError, match="duration_noise"):
        m(batch_of(z, duration_noise=torch.zeros(3, 2, 5)), inference=True)


def test_forced_durations_keep_the_prediction():
    cfg, sd, rc, z = fixture()
    m = model()
    noise = torch.from_numpy(z["noise"])
    free = cpu(m(batch_of(z, duration_noise=noise), inference=True))
    forced = np.where(z["src_mask"], 0, 2).astype(np.int32)
    out = cpu(m.forward(batch_of(z, duration_noise=noise), force_durations=torch.from_numpy(forced)))
    assert np.array_equal(out["duration_prediction"], free["duration_prediction"])  # the predictor still fills it
    assert np.array_equal(out["duration_rounded"], forced) and out["mel"].shape[1] == int(forced.sum(1).max())
    with pytest.raises(NotImplementedError, match="NLL"):
        m(batch_of(z, duration=torch.from_numpy(forced)))  # the teacher-forced call would need the training forward


@pytest.mark.parametrize("precision", ["bf16", "mixed3"])
def test_other_precisions_run_and_hold_their_bars_under_fixed_decisions(precision):
    cfg, sd, rc, z = fixture()
    ref_model = model()
    ref_model.engine.set_debug(True)
    try:
        ref_model(batch_of(z, duration_noise=torch.from_numpy(z["noise"])), inference=True)
        buckets = {v: ref_model.engine.debug_tensor(f"bucket_{v}").clone() for v in cfg.variances}
    finally:
        ref_model.engine.set_debug(False)
    m = model(precision)
    noise = torch.from_numpy(z["noise"])
    free = cpu(m(batch_of(z, duration_noise=noise), inference=True))
    assert np.isfinite(free["duration_prediction"]).all() and np.isfinite(free["mel"]).all()
    assert (free["duration_prediction"][z["src_mask"]] == 0).all()
    out = cpu(m.forward(batch_of(z, duration_noise=noise), force_durations=torch.from_numpy(z["duration_rounded"]),
                        force_buckets=buckets))
    err = np.abs(out["mel"] - z["mel"])
    print(f"sdp e2e {precision}: mel max-abs {err.max():.3e}, mean-abs {err.mean():.3e}")
    assert err.max() <= BF16_MEL_MAX and err.mean() <= BF16_MEL_MEAN


def test_state_errors():
    cfg, sd, rc, z = fixture()
    m = model()
    phones = torch.from_numpy(z["phones"]).cuda()
    speaker = torch.from_numpy(z["speaker"]).cuda()
    with pytest.raises(RuntimeError, match=r"\(5\).*fs2_set_duration_noise"):
        m.engine.encode(phones, speaker)  # no noise: FS2_ERR_STATE, nothing launched
    wrong = torch.zeros(3, 2, 7, device="cuda:0")
    assert m.engine.lib.fs2_set_duration_noise(m.engine.handle, wrong, 3, 7) == 0
    with pytest.raises(RuntimeError, match=r"\(5\)"):
        m.engine.encode(phones, speaker)  # noise announced for another shape does not count
    assert m.engine.lib.fs2_set_stochastic_duration(m.engine.handle, 1) == _lib.FS2_ERR_STATE  # weights are loaded
    out = cpu(m(batch_of(z, duration_noise=torch.from_numpy(z["noise"])), inference=True))      # and the engine still works
    assert np.array_equal(out["duration_rounded"], z["duration_rounded"])


def test_clone_graphs_and_pipeline_give_the_same_bits():
    cfg, sd, rc, z = fixture()
    m = model()
    noise = torch.from_numpy(z["noise"])
    want = cpu(m(batch_of(z, duration_noise=noise), inference=True))
    twin = m.replicate()
    got = cpu(twin(batch_of(z, duration_noise=noise), inference=True))
    assert all(np.array_equal(want[k], got[k]) for k in want)
    twin.engine.set_graphs(True)  # encode takes the plain path (the noise is a one-shot pointer), decode may replay
    dev_batch = {k: v.cuda() for k, v in batch_of(z, duration_noise=noise).items()}
    for i in range(3):
        got = cpu(twin(dev_batch, inference=True))
        assert all(np.array_equal(want[k], got[k]) for k in want), i
    # four batches through two forwards in flight against four plain calls under the same seed
    batches = []
    for i in range(4):
        inp = synth_inputs(cfg, 3, 11, seed=50 + i, lengths=[11, 9 - i, 4 + i])
        batches.append({"phones": torch.from_numpy(inp["phones"]), "speaker": torch.from_numpy(inp["speaker"])})
    torch.manual_seed(7)
    plain = [cpu(m(b, inference=True)) for b in batches]
    pipe = m.pipeline(2)
    try:
        torch.manual_seed(7)
        outs = []
        for b in batches:
            outs += pipe.submit(b)
        outs += pipe.drain()
    finally:
        pipe.close()
    assert len(outs) == 4
    for i, (a, b) in enumerate(zip(plain, outs)):
        b = cpu(b)
        assert all(np.array_equal(a[k], b[k]) for k in a), i
    assert len({p["duration_prediction"].tobytes() for p in plain}) == 4  # four different draws


def test_deterministic_model_is_untouched():
    """A model without the switch runs the conv + LayerNorm predictor and the round(exp(p) - 1) rule as before: dense_small against
    its golden at the existing bars, and the noise entry point refuses the engine."""
    g = Golden("dense_small")
    m = FastSpeech2(g.cfg, g.state_dict(), precision="fp32", device="cuda:0")
    assert m.hparams.duration_stochastic is False
    out = cpu(m({"phones": torch.from_numpy(g.phones), "speaker": torch.from_numpy(g.speaker)}, inference=True))
    for k in ("duration_rounded", "src_mask", "tgt_mask"):
        assert np.array_equal(out[k], g.out[k]), k
    assert np.abs(out["mel"] - g.out["mel"]).max() <= MEL_TOL_FP32
    assert np.abs(out["duration_prediction"] - g.out["duration_prediction"]).max() <= MEL_TOL_FP32
    z = torch.zeros(3, 2, 11, device="cuda:0")
    assert m.engine.lib.fs2_set_duration_noise(m.engine.handle, z, 3, 11) == _lib.FS2_ERR_STATE
