"""CPU checks of the sample-rate converter (csrc/glowk_resample.h, audiosourcesep_amd/audio.py): the kernel's table and output
length against the fp64 restatement of tests/resample_ref.py, the filter design itself (tone SNR and alias rejection, measured on
the restatement), the wav I/O of load_audio / save_audio without resampling, and the argument validation of the C entry points
(no GPU: every call here is refused before any device call)."""
import ctypes
import struct
import wave

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, audio
from tests import resample_ref as R

# the six rate pairs of the design check; half-second tones, 2000 samples trimmed at each end
DESIGN_PAIRS = [(44100, 16000), (48000, 16000), (32000, 16000), (22050, 16000), (8000, 16000), (16000, 44100)]


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def _err(lib):
    return lib.glowk_last_error().decode()


def test_kernel_table_against_the_restatement(lib):
    T = np.empty(R.ZP + 1, dtype=np.float64)
    assert lib.glowk_resample_filter(T.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    ref = R.table()
    print("kernel table vs scipy restatement: max |d| %.2e" % np.abs(T - ref).max())
    assert np.abs(T - ref).max() <= 1e-14
    from scipy.special import i0
    assert abs(T[0] - R.ROLLOFF) <= 1e-15 and abs(T[-1]) <= 1.0 / (np.pi * R.Z * i0(R.BETA))   # |rho sinc(rho Z)| <= 1 / (pi Z), window end 1 / I0
    assert lib.glowk_resample_filter(None) != 0 and "null" in _err(lib)


def test_output_length_against_the_integer_formula(lib):
    rates = [(44100, 16000), (48000, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (96000, 16000), (16000, 44100),
             (16000, 48000), (44101, 16000), (16000, 16000), (1000, 64000), (768000, 12000), (767999, 768000)]
    for sr_in, sr_out in rates:
        for n in (0, 1, 2, 127, 128, 129, 1000, 32640, 195840, 52920000, 1 << 32):
            assert lib.glowk_resample_length(n, sr_in, sr_out) == -((-n * sr_out) // sr_in) == R.length(n, sr_in, sr_out)
    for n, sr_in, sr_out in [(-1, 44100, 16000), ((1 << 32) + 1, 44100, 16000), (10, 999, 16000), (10, 16000, 768001),
                             (10, 1000, 64001), (10, 64001, 1000), (10, 0, 16000), (10, 16000, -5)]:
        assert lib.glowk_resample_length(n, sr_in, sr_out) == -1


def _tone_case(sr_in, sr_out, f):
    n = sr_in // 2
    x = np.sin(2.0 * np.pi * f * np.arange(n) / sr_in)
    y = R.resample(x, sr_in, sr_out)
    assert len(y) == R.length(n, sr_in, sr_out)
    return y[2000:-2000], np.sin(2.0 * np.pi * f * np.arange(len(y)) / sr_out)[2000:-2000]


@pytest.mark.parametrize("sr_in,sr_out", DESIGN_PAIRS)
def test_design_passes_tones_and_rejects_aliases(sr_in, sr_out):
    """Conditions on the design (measured on the restatement: SNR >= 112.9 dB, aliases <= -119.7 dB), not kernel tolerances."""
    narrow = min(sr_in, sr_out) / 2.0
    for f in (440.0, 3000.0, 6500.0):
        if f > 0.8125 * narrow:
            continue
        y, ideal = _tone_case(sr_in, sr_out, f)
        snr = 10.0 * np.log10(np.sum(ideal ** 2) / np.sum((y - ideal) ** 2))
        print("%d -> %d Hz, tone %6.0f Hz: SNR %.1f dB" % (sr_in, sr_out, f, snr))
        assert snr >= 100.0
    if sr_out < sr_in:                                   # a tone above the new Nyquist must vanish, not fold back
        for k in (1.0, 1.06, 1.15, 1.5):
            f = k * sr_out / 2.0
            if f >= sr_in / 2.0:
                continue
            y, _ = _tone_case(sr_in, sr_out, f)
            level = 10.0 * np.log10(np.mean(y ** 2) / 0.5)
            print("%d -> %d Hz, tone at %.2f x the new Nyquist: %.1f dB re its input level" % (sr_in, sr_out, k, level))
            assert level <= -100.0


def test_restatement_subset_equals_the_full_run():
    x = np.random.default_rng(2).standard_normal(3000)
    y = R.resample(x, 44100, 16000)
    idx = np.array([0, 1, 17, 500, len(y) - 1])
    np.testing.assert_allclose(R.resample(x, 44100, 16000, idx=idx), y[idx], rtol=0, atol=1e-13)     # fp64 sums of other row counts


def _write_pcm(path, values, width, ch, rate):
    """values [n, ch] integers -> a PCM wav of `width` bytes per sample (8-bit is unsigned, offset 128)."""
    v = np.asarray(values, dtype=np.int64).reshape(-1)
    if width == 1:
        raw = (v + 128).astype(np.uint8).tobytes()
    elif width == 3:
        u = (v & 0xFFFFFF).astype(np.uint32)
        raw = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    else:
        raw = v.astype("<i2" if width == 2 else "<i4").tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ch); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(raw)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("ch", [1, 2])
def test_load_audio_reads_every_pcm_width_exactly(tmp_path, width, ch):
    bits = 8 * width
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rng = np.random.default_rng(width * 10 + ch)
    v = rng.integers(lo, hi + 1, size=(500, ch))
    v[0], v[1], v[2] = lo, hi, 0
    p = tmp_path / "a.wav"
    _write_pcm(p, v, width, ch, 44100)
    y, rate = audio.load_audio(p, sr=None, mono=False)
    assert rate == 44100 and torch.is_tensor(y) and y.dtype == torch.float32 and not y.is_cuda and tuple(y.shape) == (ch, 500)
    want = (v.T.astype(np.float64) / float(1 << (bits - 1)))
    np.testing.assert_array_equal(y.numpy(), want.astype(np.float32))
    m, _ = audio.load_audio(p, sr=None)                               # mono=True: librosa.to_mono
    assert tuple(m.shape) == (500,)
    np.testing.assert_array_equal(m.numpy(), want.mean(axis=0).astype(np.float32))
    same, _ = audio.load_audio(p, sr=44100)                           # the file's own rate: no resampling, no GPU
    assert torch.equal(same, m)


def test_save_audio_round_trips_through_load_audio(tmp_path):
    rng = np.random.default_rng(4)
    y = rng.uniform(-1.2, 1.2, (2, 3000)).astype(np.float32)
    p = tmp_path / "st.wav"
    audio.save_audio(p, y, 48000)
    with wave.open(str(p), "rb") as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (48000, 2, 2, 3000)
    z, rate = audio.load_audio(p, sr=None, mono=False)
    q = np.rint(np.clip(y.astype(np.float64), -1.0, 1.0) * 32767.0)    # write_wav's rounding and clipping
    assert rate == 48000
    np.testing.assert_array_equal(z.numpy(), (q / 32768.0).astype(np.float32))
    audio.save_audio(tmp_path / "m.wav", torch.from_numpy(y[0]), 22050)
    z, rate = audio.load_audio(tmp_path / "m.wav", sr=None)
    assert rate == 22050
    np.testing.assert_array_equal(z.numpy(), (q[0] / 32768.0).astype(np.float32))
    for bad in (999, 768001, 44100.0, True, None):
        with pytest.raises(ValueError, match="sr"):
            audio.save_audio(tmp_path / "x.wav", y, bad)
    with pytest.raises(ValueError, match="y:"):
        audio.save_audio(tmp_path / "x.wav", np.zeros((2, 3, 4), np.float32), 16000)


def _write_tagged(path, tag, bits, extensible=False):
    """A RIFF/WAVE file of 8 mono frames whose fmt chunk carries format tag `tag`."""
    data = b"\0" * (8 * bits // 8)
    fmt = struct.pack("<HHIIHH", tag, 1, 16000, 16000 * bits // 8, bits // 8, bits)
    if extensible:                                                   # cbSize 22: valid bits, channel mask, the PCM sub-format GUID
        fmt += struct.pack("<HHI", 22, bits, 4) + struct.pack("<H", 1) + bytes.fromhex("000000001000800000aa00389b71")
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_load_audio_refuses_float_and_extensible_wavs(tmp_path):
    f = tmp_path / "float.wav"
    _write_tagged(f, 3, 32)
    with pytest.raises(ValueError, match="IEEE float"):
        audio.load_audio(f, sr=None)
    e = tmp_path / "ext.wav"
    _write_tagged(e, 0xFFFE, 16, extensible=True)
    with pytest.raises(ValueError, match="EXTENSIBLE"):
        audio.load_audio(e, sr=None)
    junk = tmp_path / "junk.wav"
    junk.write_bytes(b"not a wav file at all")
    with pytest.raises(ValueError, match="RIFF"):
        audio.load_audio(junk, sr=None)
    ok = tmp_path / "ok.wav"
    _write_tagged(ok, 1, 16)
    y, rate = audio.load_audio(ok, sr=None)
    assert rate == 16000 and tuple(y.shape) == (8,)
    with pytest.raises(ValueError, match="sr"):
        audio.load_audio(ok, sr=500)


def test_read_wav_still_refuses_other_rates(tmp_path):
    p = tmp_path / "b.wav"
    _write_pcm(p, np.zeros((10, 1)), 2, 1, 44100)
    with pytest.raises(ValueError, match="44100"):
        audio.read_wav(p)
    y, rate = audio.load_audio(p, sr=None)
    assert rate == 44100 and tuple(y.shape) == (10,)


def test_resample_python_checks_come_before_any_device_call():
    x = np.zeros(100, np.float32)
    for bad in (999, 768001, 44100.0, "44100", True, None):
        with pytest.raises(ValueError, match="orig_sr"):
            audio.resample(x, bad, 16000)
        with pytest.raises(ValueError, match="target_sr"):
            audio.resample(x, 16000, bad)
    with pytest.raises(ValueError, match="factor 64"):
        audio.resample(x, 1000, 64001)
    with pytest.raises(ValueError, match="y:"):
        audio.resample(np.float32(1.0), 44100, 16000)
    with pytest.raises(ValueError, match="real"):
        audio.resample(np.zeros(4, np.complex64), 44100, 16000)
    same = audio.resample(x.astype(np.float64), 16000, 16000)         # equal rates: the input, as float32, no launch
    assert same.dtype == torch.float32 and not same.is_cuda and tuple(same.shape) == (100,)
    with pytest.raises(ValueError, match="out_rate"):
        audio.separate_wav("nothing.wav", None, None, [1.0], out_rate="native")
    with pytest.raises(ValueError, match="out_rate"):
        audio.separate_wav("nothing.wav", None, None, [1.0], out_rate=10)


def test_resample_entry_point_validates_before_any_device_call(lib):
    d = ctypes.c_void_p(16)                           # never dereferenced: every call below fails validation or returns first
    z = ctypes.c_void_p(0)
    for sr_in, sr_out in [(999, 16000), (768001, 16000), (16000, 999), (16000, 768001), (0, 16000), (16000, -1)]:
        assert lib.glowk_resample(d, 1, 100, sr_in, sr_out, d, z) == _lib.ERR and "[1000, 768000]" in _err(lib)
    assert lib.glowk_resample(d, 1, 100, 1000, 64001, d, z) == _lib.ERR and "1/64" in _err(lib)
    assert lib.glowk_resample(d, 1, 100, 64001, 1000, d, z) == _lib.ERR and "1/64" in _err(lib)
    assert lib.glowk_resample(d, 1, -1, 44100, 16000, d, z) == _lib.ERR and "n_in" in _err(lib)
    assert lib.glowk_resample(d, 1, (1 << 32) + 1, 44100, 16000, d, z) == _lib.ERR and "n_in" in _err(lib)
    assert lib.glowk_resample(d, -1, 100, 44100, 16000, d, z) == _lib.ERR and "nsig" in _err(lib)
    assert lib.glowk_resample(d, (1 << 20) + 1, 100, 44100, 16000, d, z) == _lib.ERR and "nsig" in _err(lib)
    assert lib.glowk_resample(z, 1, 100, 44100, 16000, d, z) == _lib.ERR and "null" in _err(lib)
    assert lib.glowk_resample(d, 1, 100, 44100, 16000, z, z) == _lib.ERR and "null" in _err(lib)
    assert lib.glowk_resample(d, 1 << 20, 1 << 32, 16000, 44100, d, z) == _lib.ERR and "one launch" in _err(lib)
    assert lib.glowk_resample(z, 0, 100, 44100, 16000, z, z) == 0      # no signals, no samples: successful no-ops
    assert lib.glowk_resample(z, 3, 0, 44100, 16000, z, z) == 0
    assert lib.glowk_resample(z, 0, 100, 999, 16000, z, z) == _lib.ERR  # ... of valid arguments only
