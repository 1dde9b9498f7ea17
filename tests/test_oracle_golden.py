"""The CPU oracle against (a) the committed golden vectors captured from the real reference and
(b) what the live reference import returned on randomised hparams (tests/golden/random_reference.npz)."""
import os

import numpy as np
import pytest
import torch

from _golden import GOLDEN_DIR, Golden, golden_names, lookup, sd_digest
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict
from oracle import oracle_cpu

ORACLE_TOL = 2e-5  # fp32 restatement vs the reference's own fp32 forward (observed ~1e-6)


def test_fixtures_present():
    names = golden_names()
    for want in ("dense_small", "dw_small", "mixed_small", "guard_small", "clip_small", "priors_small", "teacher_small",
                 "mid_dense_d128", "mid_dw_d64", "cwt_small", "cwt_teacher_small", "phone_small", "phone_teacher_small", "phone_cwt_small"):
        assert want in names


@pytest.mark.parametrize("name", golden_names())
def test_oracle_matches_reference_golden(name):
    g = Golden(name)
    out = oracle_cpu.forward(g.state_dict(), g.cfg, g.phones, g.speaker, return_intermediates=True, priors=g.priors,
                             teacher_targets=g.teacher)
    assert out["mel"].shape == g.out["mel"].shape
    for k in ("duration_rounded", "src_mask", "tgt_mask"):
        assert np.array_equal(out[k].numpy(), g.out[k]), k
    assert out["duration_rounded"].dtype == (torch.int32 if g.teacher is None else torch.int64)
    for k, ref in g.out.items():
        if ref.dtype.kind == "f":
            err = float(np.abs(lookup(out, k).numpy() - ref).max())
            assert err <= ORACLE_TOL, (k, err)
    for k, ref in g.mid.items():
        err = float(np.abs(out["_intermediates"][k].numpy() - ref).max())
        assert err <= ORACLE_TOL, (k, err)
    assert len(out["_zero_duration_guard"]) == g.n_guard


def test_guard_and_clip_fixtures_hit_their_branches():
    g = Golden("guard_small")
    assert 0 < g.n_guard < g.phones.shape[0]
    c = Golden("clip_small")
    totals = c.out["duration_rounded"].sum(1)
    assert totals.max() > c.cfg.max_frames == c.out["mel"].shape[1]
    # model.py:354-361: the mask uses the UNtruncated lengths -> a clipped utterance has no pad
    assert not c.out["tgt_mask"][int(totals.argmax())].any()


def _random_cfg(rs):
    H = int(rs.choice([32, 64]))
    heads = int(rs.choice([1, 2, 4]))
    dw = [bool(rs.randint(2)) for _ in range(4)]
    nl_e, nl_d = int(rs.randint(1, 3)), int(rs.randint(1, 3))
    odd = lambda: int(rs.choice([1, 3, 5, 7, 9]))
    variances = list(rs.permutation(["pitch", "energy", "snr"])[: rs.randint(1, 4)])
    nv = len(variances)
    return Fs2Config(
        n_phones=int(rs.randint(5, 50)), encoder_hidden=H, decoder_hidden=H, encoder_head=heads, decoder_head=heads,
        encoder_layers=nl_e, decoder_layers=nl_d, encoder_kernel_sizes=[odd() for _ in range(nl_e)],
        decoder_kernel_sizes=[odd() for _ in range(nl_d)], encoder_depthwise_conv=dw[0], decoder_depthwise_conv=dw[1],
        encoder_conv_filter_size=H * int(rs.choice([1, 2, 4])), decoder_conv_filter_size=H * int(rs.choice([1, 2, 4])),
        variances=variances, variance_levels=[str(rs.choice(["frame", "frame", "phone"])) for _ in range(nv)], variance_transforms=["none"] * nv,
        variance_nlayers=[int(rs.randint(1, 4)) for _ in range(nv)], variance_kernel_size=[odd() for _ in range(nv)],
        variance_filter_size=H, variance_nbins=int(rs.choice([8, 33, 256])), variance_depthwise_conv=dw[2],
        duration_nlayers=int(rs.randint(1, 3)), duration_kernel_size=odd(), duration_filter_size=H,
        duration_depthwise_conv=dw[3], n_mels=int(rs.choice([5, 80])),
        stats={v: {"min": float(-1 - rs.rand()), "max": float(1 + 2 * rs.rand()), "mean": float(rs.randn() * .3),
                   "std": float(.5 + rs.rand())} for v in variances})


N_RANDOM_CASES = 10
RANDOM_REFERENCE = os.path.join(GOLDEN_DIR, "random_reference.npz")


def random_case(seed):
    """(cfg, state_dict, inputs) of randomised-hparams case `seed`"""
    rs = np.random.RandomState(100 + seed)
    cfg = _random_cfg(rs)
    B, L = int(rs.randint(1, 5)), int(rs.randint(3, 15))
    lengths = [L] + [int(rs.randint(1, L + 1)) for _ in range(B - 1)]
    sd = synth_state_dict(cfg, seed, randomize_norm=True, duration_bias=float(rs.uniform(0.2, 1.6)))
    inp = synth_inputs(cfg, B, L, seed=seed, lengths=lengths)
    return cfg, sd, inp


@pytest.mark.parametrize("seed", range(N_RANDOM_CASES))
def test_oracle_matches_live_reference(seed):
    """The oracle against what the live reference import returned for randomised hparams (tests/golden/random_reference.npz,
    tools/gen_golden_random.py); the case is rebuilt here and must be the one the reference ran."""
    cfg, sd, inp = random_case(seed)
    z = np.load(RANDOM_REFERENCE)
    assert str(z[f"s{seed}_config_json"]) == cfg.to_json(), "randomised config drifted from the fixture"
    assert str(z[f"s{seed}_sd_sha256"]) == sd_digest(sd), "synthetic weight recipe drifted from the fixture"
    assert np.array_equal(z[f"s{seed}_phones"], inp["phones"])
    ref = {k[len(f"s{seed}_out_"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"s{seed}_out_")}
    out = oracle_cpu.forward(sd, cfg, inp["phones"], inp["speaker"], return_intermediates=True)
    # decisions may legitimately flip only if the reference sat within float noise of a threshold;
    # with 1e-6 agreement that is vanishingly rare at these sizes
    assert torch.equal(ref["duration_rounded"], out["duration_rounded"])
    assert torch.equal(ref["tgt_mask"], out["tgt_mask"]) and torch.equal(ref["src_mask"], out["src_mask"])
    for k in ["mel", "duration_prediction"] + [f"variances_{v}" for v in cfg.variances]:
        assert float((ref[k] - out[k]).abs().max()) <= ORACLE_TOL, k
