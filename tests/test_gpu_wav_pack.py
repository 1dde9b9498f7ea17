"""fs2_op_wav_pack on its own (no generator): the float32 -> int16 cast and the int16 -> float32 rescale bit for bit against numpy (what
Synthesiser.__call__ and int16_samples_to_float32 do on the host), the offsets and the packed layout of ragged batches on the wide
(16 B) and the narrow path, writes behind the packed total, argument errors."""

import numpy as np
import pytest
import torch

from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.hifigan import wav_pack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"int16": (_lib.FS2_WAV_I16, torch.int16, np.int16), "float32": (_lib.FS2_WAV_F32, torch.float32, np.float32)}
CANARY = {"int16": 12345, "float32": 777.0}
SLACK = 64  # canary elements behind the capacity the operator asks for


def pack(wav, lengths, hop, dtype, capacity=None):
    """-> status, out (whole buffer, canaries included), offsets; straight through the C ABI."""
    kind, tdt, _ = KINDS[dtype]
    B, S = wav.shape
    w = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(DEV)
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    cap = B * S if capacity is None else capacity
    out = torch.full((cap + SLACK,), CANARY[dtype], dtype=tdt, device=DEV)
    off = torch.full((B + 2,), -7, dtype=torch.int64, device=DEV)
    st = _lib.load().fs2_op_wav_pack(w, ld, B, S // hop, hop, kind, out, cap, off, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), off.cpu().numpy()


def host_i16(x):
    """Synthesiser.__call__ (third_party/hifigan/__init__.py:39-43)"""
    return (x * 32768.0).astype("int16")


def host_f32(q):
    """int16_samples_to_float32 (synthesis/generator.py:24-33)"""
    return q.astype(np.float32) / float(np.iinfo(np.int16).max)


def through(x, dtype, misalign):
    """Push a flat array of samples through one launch; `misalign` puts them behind a 3-sample utterance (hop 1), so that neither an
    int16 nor a float32 destination is 16 B aligned: the narrow path.  Otherwise one full row, hop 8: the wide path for every full chunk."""
    n = x.size
    S = -(-n // 2048) * 2048 + 2048 - 8  # whole chunks and a partial one
    row = np.zeros(S, np.float32)
    row[:n] = x
    if misalign:
        st, out, off = pack(np.stack([np.zeros(S, np.float32), row]), [3, S], 1, dtype)
        assert st == 0 and off[:3].tolist() == [0, 3, 3 + S]
        return out[3:3 + n]
    st, out, off = pack(row[None], None, 8, dtype)
    assert st == 0 and off[:2].tolist() == [0, S]
    return out[:n]


@pytest.mark.parametrize("misalign", [False, True])
def test_float_conversion_exhaustive(misalign):
    """All 65536 int16 values: x = q / 32768 is exact in float32 and quantises back to q; the float32 kind must give
    q.astype(float32) / 32767.0 bit for bit (a correctly rounded fp32 division)."""
    q = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    x = (q.astype(np.float64) / 32768.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 32768.0, q.astype(np.float64))
    got = through(x, "float32", misalign)
    want = host_f32(q)
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(through(x, "int16", misalign), q)


@pytest.mark.parametrize("misalign", [False, True])
def test_quantiser_matches_numpy_cast(misalign):
    """~4k integers k over the int16 range: k / 32768 and its two float32 neighbours (the truncation's edges on both sides of zero), zeros,
    tiny values, the largest magnitudes below one and -1.0, against numpy's own cast.  +1.0 (tanh saturated) is out of int16's range:
    the operator wraps it to -32768 as the host recipe does on the hosts this was written on - asserted as a literal."""
    ks = np.unique(np.concatenate([np.linspace(-32768, 32767, 4001).round().astype(np.int64), np.arange(-3, 4),
                                   [-32768, -32767, 32766, 32767]]))
    c = (ks.astype(np.float64) / 32768.0).astype(np.float32)
    x = np.concatenate([c, np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-2)),
                        np.array([-0.0, 0.0, 1e-8, -1e-8, 0.99999994, -0.99999994, -1.0], np.float32)]).astype(np.float32)
    assert not (x == 1.0).any() and x.min() >= np.nextafter(np.float32(-1), np.float32(-2))
    x = np.concatenate([x, np.array([1.0], np.float32)])
    got = through(x, "int16", misalign)
    assert np.array_equal(got[:-1], host_i16(x[:-1]))
    assert int(got[-1]) == -32768
    gotf = through(x, "float32", misalign)
    assert np.array_equal(gotf[:-1].view(np.uint32), host_f32(host_i16(x[:-1])).view(np.uint32))
    assert gotf[-1] == np.float32(-32768.0) / np.float32(32767.0)


RAGGED = [
    (5, 7, 8, [7, 0, 1, 6, 7]),          # the int16 rows start 16 B aligned, the float32 ones too
    (5, 7, 4, [7, 0, 1, 6, 7]),          # hop 4: int16 offsets 28, 28, 32, 56 elements - aligned and misaligned utterances in one launch
    (5, 7, 256, None),                   # full rows
    (4, 6, 3, [6, 5, 0, 2]),             # an odd hop: source rows misaligned as well
    (3, 5, 8, [9, -2, 3]),               # counts clamped to [0, T]
    (3, 41, 256, [41, 17, 40]),          # several workgroups per utterance, partial last chunks, workgroups past an utterance's end
    (64, 36, 2048, "random"),            # 36 chunks per row on a grid of 32: the strided rounds
]


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("B,T,hop,lengths", RAGGED)
def test_ragged_packing(B, T, hop, lengths, dtype):
    rs = np.random.RandomState(B * 1000 + T * 10 + hop)
    if isinstance(lengths, str):
        lengths = rs.randint(0, T + 1, size=B).tolist()
        lengths[3], lengths[-1] = T, T
    wav = rs.uniform(-1, 1, size=(B, T * hop)).astype(np.float32)
    wav[0, :4] = [1.0, -1.0, 0.99999994, -0.0]
    lens = [T] * B if lengths is None else [min(max(n, 0), T) for n in lengths]
    fed = wav.copy()
    for b, n in enumerate(lens):
        fed[b, n * hop:] = np.nan  # pads are not read; whatever they hold must not show
    st, out, off = pack(fed, lengths, hop, dtype)
    assert st == 0
    want_off = np.concatenate([[0], np.cumsum(np.array(lens, np.int64) * hop)])
    assert np.array_equal(off[:B + 1], want_off) and off[B + 1] == -7
    q = host_i16(wav)
    q[0, 0] = -32768  # +1.0: see test_quantiser_matches_numpy_cast
    ref = q if dtype == "int16" else host_f32(q)
    want = np.concatenate([ref[b, :n * hop] for b, n in enumerate(lens)])
    total = int(want_off[-1])
    got = out[:total]
    assert got.dtype == KINDS[dtype][2]
    assert np.array_equal(got.view(np.uint16 if dtype == "int16" else np.uint32), want.view(np.uint16 if dtype == "int16" else np.uint32))
    assert (out[total:] == KINDS[dtype][2](CANARY[dtype])).all(), "written behind offsets[B]"


def test_python_binding_and_out_buffer():
    rs = np.random.RandomState(0)
    wav = torch.from_numpy(rs.uniform(-1, 1, size=(3, 40)).astype(np.float32)).to(DEV)
    lens = torch.tensor([5, 2, 4], dtype=torch.int32, device=DEV)
    packed, off = wav_pack(wav, lens, 8, "int16")
    assert packed.dtype == torch.int16 and packed.shape == (120,) and off.tolist() == [0, 40, 56, 88]
    q = host_i16(wav.cpu().numpy())
    assert np.array_equal(packed[:88].cpu().numpy(), np.concatenate([q[0, :40], q[1, :16], q[2, :32]]))
    mine = torch.zeros(200, dtype=torch.float32, device=DEV)
    packed, off = wav_pack(wav, None, 8, "float32", out=mine)
    assert packed.data_ptr() == mine.data_ptr() and off.tolist() == [0, 40, 80, 120]
    assert np.array_equal(mine[:120].cpu().numpy(), host_f32(q).reshape(-1)) and float(mine[120:].abs().sum()) == 0.0
    with pytest.raises(RuntimeError):
        wav_pack(wav, lens, 8, "float32", out=torch.zeros(119, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        wav_pack(wav, lens, 8, "float64")
    with pytest.raises(ValueError):
        wav_pack(wav, lens, 7, "int16")


def test_errors():
    wav = np.zeros((2, 24), np.float32)
    for dtype in KINDS:
        st, out, off = pack(wav, [3, 3], 8, dtype, capacity=47)  # one short of B * T * hop, whatever the lengths say
        assert st == _lib.FS2_ERR_ARG
        assert (out == KINDS[dtype][2](CANARY[dtype])).all() and (off == -7).all()  # nothing was launched
    lib = _lib.load()
    w = torch.zeros(2, 24, device=DEV)
    out = torch.zeros(48, dtype=torch.int16, device=DEV)
    off = torch.zeros(3, dtype=torch.int64, device=DEV)
    args = lambda **k: [k.get("wav", w), None, k.get("B", 2), k.get("T", 3), k.get("hop", 8), k.get("kind", 0), k.get("out", out),
                        48, k.get("off", off), None]
    assert lib.fs2_op_wav_pack(*args()) == 0
    for bad in (dict(wav=None), dict(out=None), dict(off=None), dict(kind=2), dict(B=0), dict(T=0), dict(hop=0)):
        assert lib.fs2_op_wav_pack(*args(**bad)) == _lib.FS2_ERR_ARG, bad
    torch.cuda.synchronize()
