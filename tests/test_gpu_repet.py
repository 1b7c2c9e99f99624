"""REPET-SIM on the GPU (csrc/glowk_repet.h through ``audiosourcesep_amd.repet``) against the fp64 restatement of
tests/repet_ref.py.

Bars.  Neighbours: tie-tolerant validity with tol = 4 rows 2^-24, the worst-case fp32 bound of one dot product and two norms over
``rows`` terms (numpy's own fp32 evaluation: 1.4e-6 at rows = 1025 against 2.4e-4, 3.4e-7 at rows = 96); exact where the input
leaves no doubt (one row: every cosine is 1 or 0; the planted input: the gap is thousands of tol).  Filter: bitwise -- the median
is a selection, and at an even count one fp32 (a + b) * 0.5.  Masks: 1e-6 absolute against the fp64 restatement fed the device's
own filter output, the bar of tests/test_gpu_hpss.py, whose kernel this is.  Audio: 1e-5 of the mixture's peak over every sample,
the bar of the HPSS stems, whose inversion this is."""
import ctypes
import functools
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio, repet
from tests import audio_ref as A
from tests import repet_ref as R
from tests.footprint import Guarded

pytestmark = pytest.mark.gpu

# (nsig, rows, F, k, width).  A workgroup owns 32 query frames and walks the candidates in tiles of 256 (k <= 160) or 128 frames;
# the Gram loop takes 16 row pairs per step, then single pairs, then an odd row; the median takes 64, 32 or 16 rows per workgroup
# by k (<= 192, <= 384, above).
NEIGHBOUR_CASES = [
    (1, 1, 40, 3, 1),                       # one row: every cosine is 1 or 0, everything ties (held exactly, below)
    (1, 33, 63, 4, 5), (1, 33, 64, 4, 5), (1, 33, 65, 5, 5), (3, 33, 129, 8, 3),   # either side of tile edges; rows off the MFMA K; batch
    (1, 96, 64, 1, 1),                      # k = 1
    (1, 7, 7, 16, 3),                       # k above the candidate count; edge frames have more candidates than middle ones
    (1, 9, 10, 4, 10), (1, 9, 10, 4, 1000),                                       # no candidates at all
    (1, 5, 600, 512, 1),                    # k at its cap: the 128-frame candidate tiles, five of them
    (2, 1025, 70, 9, 4),                    # the real row count
    (1, 4096, 66, 6, 2),                    # the row cap
    (1, 39, 300, 6, 2),                     # 16 row pairs, 3 single pairs and an odd row; two 256-frame candidate tiles
    (1, 5, 200, 160, 1), (1, 5, 200, 161, 1),                                     # either side of the two list capacities
    (2, 70, 300, 200, 2),                   # the median's 32-row workgroups, the last with 6 rows
]
MEDIAN_CASES = NEIGHBOUR_CASES


def quantised(rng, shape):
    """|N(0, 1)| quantised to 8 levels (multiples of 1/2, so a margin of 2 or 10 multiplies them exactly), 30 % exact zeros."""
    x = np.minimum(np.floor(np.abs(rng.standard_normal(shape)) * 2.0), 7.0) / 2.0
    x[rng.random(shape) < 0.3] = 0.0
    return x.astype(np.float32)


def continuous(rng, shape):
    """|N(0, 1)|^2 with about 5 % all-zero frames."""
    x = (np.abs(rng.standard_normal(shape)) ** 2).astype(np.float32)
    silent = rng.random(shape[-1]) < 0.05
    if shape[-1] >= 8:
        silent[shape[-1] // 2] = True                                               # at least one, whatever the draw
    x[..., silent] = 0.0
    return x


def spectra(case, maker=continuous):
    nsig, rows, F, k, width = case
    return maker(np.random.default_rng(1000 * rows + 10 * F + k), (nsig, rows, F))


@pytest.mark.parametrize("case", NEIGHBOUR_CASES, ids=lambda c: "-".join(map(str, c)))
def test_neighbours_are_valid_against_fp64(case):
    nsig, rows, F, k, width = case
    S = spectra(case)
    assert F < 8 or (S == 0).all(axis=(0, 1)).any()                                # a silent frame is among them
    tol = 4 * rows * 2.0 ** -24
    idx, sim = repet.neighbors(S, k, width, return_similarity=True)
    assert idx.is_cuda and idx.dtype == torch.int32 and sim.dtype == torch.float32 and tuple(idx.shape) == tuple(sim.shape) == (nsig, F, k)
    idx, sim = idx.cpu().numpy(), sim.cpu().numpy()
    j = np.arange(F)
    worst_sel, worst_sim = 0.0, 0.0
    for n in range(nsig):
        sim64 = R.similarity(S[n])
        _, _, kth = R.select(sim64, k, width)
        for i in range(F):
            k_i = min(k, int((np.abs(j - i) >= width).sum()))
            got = idx[n, i, :k_i]
            assert (idx[n, i, k_i:] == -1).all() and (sim[n, i, k_i:] == 0).all(), (n, i)
            assert ((got >= 0) & (got < F)).all() and (np.abs(got - i) >= width).all() and len(set(got.tolist())) == k_i, (n, i)
            if k_i:
                worst_sel = max(worst_sel, float((kth[i] - sim64[i, got]).max()))
                worst_sim = max(worst_sim, float(np.abs(sim[n, i, :k_i] - sim64[i, got]).max()))
        assert (np.diff(sim[n], axis=1) <= 0).all()                                # non-increasing along k, the zeros of the -1 included
    print("neighbours %s: selected at most %.3e below the k-th fp64 similarity, sim at most %.3e off fp64; tol %.3e"
          % (case, worst_sel, worst_sim, tol))
    assert worst_sel <= tol and worst_sim <= tol
    if rows == 1:                                                                   # cosines of one row: exactly 1 or 0, all ties
        live = (S[0, 0] != 0).astype(np.float64)
        want_idx, want_sim, _ = R.select(np.outer(live, live), k, width)
        assert np.array_equal(idx[0], want_idx) and np.array_equal(sim[0], want_sim.astype(np.float32))
    again = repet.neighbors(torch.from_numpy(S).cuda(), k, width)                   # a second run, from the device, without sim
    assert np.array_equal(again.cpu().numpy(), idx)
    if nsig > 1:                                                                    # a batch gives what its signals give alone
        for n in range(nsig):
            assert np.array_equal(repet.neighbors(S[n], k, width).cpu().numpy(), idx[n])


@pytest.mark.parametrize("rows,P,k,width", [(33, 12, 4, 5), (1025, 70, 3, 62)])
def test_unambiguous_neighbour_sets_equal_the_restatements(rows, P, k, width):
    S = R.planted(np.random.default_rng(rows + P), rows, P, k + 1)
    F = S.shape[1]
    tol = 4 * rows * 2.0 ** -24
    sim64 = R.similarity(S)
    want, _, kth = R.select(sim64, k, width)
    j = np.arange(F)
    gap = min(kth[i] - np.sort(sim64[i, np.abs(j - i) >= width])[::-1][k] for i in range(F))
    print("planted %s: the fp64 gap between candidates k and k + 1 is at least %.3e; 10 tol = %.3e" % ((rows, P, k, width), gap, 10 * tol))
    assert gap > 10 * tol                                                           # the input's property, not the code's
    got = repet.neighbors(S, k, width).cpu().numpy()
    copies = R.copies_of(F, P)
    for i in range(F):
        assert set(got[i].tolist()) == set(want[i].tolist()) == copies[i], i


@pytest.mark.parametrize("maker", [quantised, continuous], ids=["quantised", "continuous"])
@pytest.mark.parametrize("case", MEDIAN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_nn_filter_bitwise(case, maker):
    nsig, rows, F, k, width = case
    S = spectra(case, maker)
    got, idx = repet.nn_filter(S, k, width, return_neighbors=True)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == S.shape and tuple(idx.shape) == (nsig, F, k)
    want = R.gather_median(S, idx.cpu().numpy())                                    # the device's own neighbours
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    counts = (idx.cpu().numpy() >= 0).sum(-1)
    if case == (1, 7, 7, 16, 3):
        assert set(counts.ravel().tolist()) == {2, 3, 4}                            # odd and even counts in one call
    if width >= F:
        assert (counts == 0).all() and np.array_equal(got.cpu().numpy(), S)         # no candidates: the filter returns S
    again = repet.nn_filter(torch.from_numpy(S).cuda(), k, width)                   # a second run, from the device
    assert torch.equal(got, again)
    if nsig > 1:
        for n in range(nsig):                                                       # a batch gives what its signals give alone
            assert torch.equal(repet.nn_filter(S[n], k, width), got[n])


def test_nn_filter_defaults_and_empty_batches():
    S = spectra((1, 33, 65, 0, 1))[0]
    out, idx = repet.nn_filter(S, return_neighbors=True)                            # k = default_k(65, 1) = 16
    assert tuple(idx.shape) == (65, 16) and tuple(out.shape) == (33, 65)
    assert torch.equal(out, repet.nn_filter(S, k=16, width=1))
    assert tuple(repet.nn_filter(np.zeros((0, 5, 7), np.float32), 3, 1).shape) == (0, 5, 7)
    assert tuple(repet.neighbors(np.zeros((0, 5, 7), np.float32), 3, 1).shape) == (0, 7, 3)


# ---- repet_sim -----------------------------------------------------------------------------------------------------------------------
def test_the_workspace_query_is_whole_words_and_both_calls_stay_inside_it():
    """(1, 2, 31): 31 norms and 62 copied values are 93 floats, an odd count; glowk_nn_workspace_bytes rounds them up to 8-byte words, as
    every other size query does.  Through the C ABI with canaries around the workspace and the outputs: nothing outside is written and the
    results are the wrapper's."""
    nsig, rows, F, k, width = 1, 2, 31, 16, 1
    lib = _lib.load()
    nbytes = lib.glowk_nn_workspace_bytes(nsig, rows, F, k)
    assert nbytes == 376 and nbytes % 8 == 0
    S = torch.from_numpy(spectra((nsig, rows, F, k, width))).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    work = Guarded((nbytes // 4,), torch.float32, float("nan"))
    idx, sim = Guarded((nsig, F, k), torch.int32, -9, canary=77), Guarded((nsig, F, k), torch.float32, float("nan"))
    out = Guarded((nsig, rows, F), torch.float32, float("nan"))
    assert lib.glowk_nn_neighbors(p(S), nsig, rows, F, k, width, idx.ptr(), sim.ptr(), work.ptr(), nbytes, None) == 0
    assert lib.glowk_nn_median(p(S), idx.ptr(), nsig, rows, F, k, out.ptr(), work.ptr(), nbytes, None) == 0
    torch.cuda.synchronize()
    assert work.intact() and idx.intact() and sim.intact() and out.intact()
    want_out, want_idx = repet.nn_filter(S, k, width, return_neighbors=True)
    assert torch.equal(idx.t, want_idx) and torch.equal(out.t, want_out) and not bool(torch.isnan(sim.t).any())


POWERS = [1.0, 2.0, float("inf")]
MARGINS = [(1.0, 1.0), (2.0, 10.0)]


@functools.lru_cache(maxsize=None)
def filtered(kind):
    """A [2, 40, 70] spectrum (quantised: multiples of 1/2, so rep, res and their margin multiples are exact in fp32 and the hard
    mask has no doubtful comparison) and the device's own filter output (k = 6, width = 3).  Never modified."""
    S = (quantised if kind == "quantised" else continuous)(np.random.default_rng(11), (2, 40, 70))
    filt = repet.nn_filter(S, 6, 3).cpu().numpy()
    for a in (S, filt):
        a.setflags(write=False)
    return S, filt


# the hard mask compares exactly: the quantised input is its case
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("kind,power", [("quantised", p) for p in POWERS] + [("continuous", p) for p in POWERS[:2]])
def test_masks_against_the_restatement(kind, power, margin):
    S, filt = filtered(kind)
    mb, mf = (m.cpu().numpy() for m in repet.repet_sim(S.copy(), k=6, width=3, power=power, margin=margin, mask=True))
    wb, wf = R.masks(S, filt, power, margin)
    err = max(float(np.abs(mb - wb).max()), float(np.abs(mf - wf).max()))
    print("masks (%s) power = %g, margins %s: max abs error %.3e" % (kind, power, margin, err))
    assert err <= 1e-6
    assert mb.min() >= 0.0 and mb.max() <= 1.0 and mf.min() >= 0.0 and mf.max() <= 1.0
    b, f = (c.cpu().numpy() for c in repet.repet_sim(S.copy(), k=6, width=3, power=power, margin=margin))
    for c, m in ((b, mb), (f, mf)):                                                 # the components are the masked spectrum: 1 ulp
        want = S.astype(np.float64) * m.astype(np.float64)
        assert c.dtype == np.float32 and (np.abs(c - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    if margin == (1.0, 1.0) and not np.isinf(power):
        # unit margins: the masks sum to one within two roundings of 2^-25 each (a / (a + b) + b / (b + a)), and each component is
        # one rounded product -- 1 ulp per term
        bound = 2.0 ** -22 * S.astype(np.float64) + np.spacing(b) + np.spacing(f)
        assert (np.abs(b.astype(np.float64) + f - S) <= bound).all()


def test_repet_sim_of_complex_spectra_keeps_the_phase():
    rng = np.random.default_rng(21)
    S = continuous(rng, (2, 33, 65))
    phi = rng.uniform(-np.pi, np.pi, S.shape)
    Sc = (S * np.exp(1j * phi)).astype(np.complex64)
    Bc, Fc = repet.repet_sim(Sc, k=5, width=2)
    mag = np.abs(Sc)
    Br, Fr = repet.repet_sim(mag, k=5, width=2)
    # exp(i angle(S)) in fp32: the angle within an ulp of pi (2.4e-7), its cosine and sine within an ulp (6e-8), the product's
    # rounding (6e-8) -- below 4e-7 together; the bar is 1e-6 (tests/test_gpu_hpss.py)
    for c, r in ((Bc, Br), (Fc, Fr)):
        assert c.dtype == torch.complex64 and tuple(c.shape) == S.shape
        c, r = c.cpu().numpy(), r.cpu().numpy()
        live = r > 0
        assert live.any() and np.abs(c[live] / np.abs(c[live]) - Sc[live] / mag[live]).max() <= 1e-6
        assert np.abs(np.abs(c) - r).max() <= 1e-6 * r.max() and not c[~live].any()
    assert torch.equal(repet.repet_sim(mag[0], k=5, width=2)[0], Br[0])            # [rows, F] is the batch of one
    one, pair = repet.repet_sim(mag, k=5, width=2, margin=3.0), repet.repet_sim(mag, k=5, width=2, margin=(3.0, 3.0))
    assert torch.equal(one[0], pair[0]) and torch.equal(one[1], pair[1])           # a scalar margin is the pair of it


# ---- audio ---------------------------------------------------------------------------------------------------------------------------
N_AUDIO = 48000
WIDTH_SEC = 0.4
AUDIO_BAR = 1e-5


@functools.lru_cache(maxsize=None)
def mixture():
    """(pattern, chirp, y) as float32, y their sum: 3 s at 16 kHz of a repeated 0.5 s phrase and a chirp.  Never modified."""
    pattern, chirp = (c.astype(np.float32) for c in R.pattern_and_chirp(N_AUDIO))
    out = (pattern, chirp, pattern + chirp)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("margin", [(2.0, 10.0), (1.0, 1.0)])
def test_repet_sim_audio_against_the_restatement(margin):
    pattern, chirp, y = mixture()
    peak = float(np.abs(y).max())
    width = max(1, int(WIDTH_SEC * audio.SR / audio.HOP))
    b, f = repet.repet_sim_audio(y.copy(), width_sec=WIDTH_SEC, margin=margin)
    assert b.is_cuda and tuple(b.shape) == tuple(f.shape) == (N_AUDIO,) and b.dtype == torch.float32
    b, f = b.cpu().numpy(), f.cpu().numpy()
    # the restatement's path: fp64 masks on the device's STFT and neighbours, the same inverse STFT
    _, X = audio.mel_frames(np.stack([y, chirp]), return_stft=True)
    mag = X[0].abs()
    k = R.default_k(mag.shape[1], width)
    assert (width, k) == (12, 18)
    idx = repet.neighbors(mag, k, width).cpu().numpy()
    mag = mag.cpu().numpy()
    wb, wf = R.masks(mag, R.gather_median(mag, idx), 2.0, margin)
    X0 = X[0].cpu().numpy().astype(np.complex128)
    want_b, want_f = (A.istft(X0 * m)[:N_AUDIO] for m in (wb, wf))
    e_b, e_f = float(np.abs(b - want_b).max() / peak), float(np.abs(f - want_f).max() / peak)
    e_sum = float(np.abs(b.astype(np.float64) + f - y).max() / peak)
    print("repet_sim_audio margins %s: background %.2e, foreground %.2e, background + foreground - y %.2e of the peak"
          % (margin, e_b, e_f, e_sum))
    assert e_b <= AUDIO_BAR and e_f <= AUDIO_BAR
    if margin == (1.0, 1.0):
        assert e_sum <= AUDIO_BAR                                                  # unit margins: the stems sum to the mixture
    # the device's foreground mask of the mixture on the chirp's own STFT: what does not repeat is foreground
    _, mask_f = repet.repet_sim(X[0].abs(), width=width, margin=margin, mask=True)
    in_f = float(((mask_f * X[1].abs()) ** 2).sum() / (X[1].abs() ** 2).sum())
    print("margins %s: %.4f of the chirp's energy in the foreground stem" % (margin, in_f))
    assert in_f > 0.5


def test_repet_sim_audio_channels_and_residual():
    y = mixture()[2]
    two = np.stack([y, 0.5 * y[::-1]]).astype(np.float32)
    b2, f2 = repet.repet_sim_audio(two, width_sec=WIDTH_SEC)
    assert tuple(b2.shape) == tuple(f2.shape) == (2, N_AUDIO)
    for c in range(2):                                                             # a channel's stems depend on that channel alone
        b, f = repet.repet_sim_audio(two[c], width_sec=WIDTH_SEC)
        assert torch.equal(b2[c], b) and torch.equal(f2[c], f)
    yt = torch.from_numpy(y.copy()).cuda()
    b, f, r = repet.repet_sim_audio(yt, k=10, width_sec=WIDTH_SEC, residual=True)
    assert tuple(r.shape) == (N_AUDIO,) and torch.equal(r, yt - b - f) and float(r.abs().max()) > 1e-3   # margins above 1 leave a residual


def test_separate_wav_repet_returns_the_files_rate_and_length(tmp_path):
    rate = 22050
    pattern, chirp = R.pattern_and_chirp(N_AUDIO, rate)
    y = pattern + chirp
    q = np.rint(np.clip(np.stack([y, 0.5 * y]), -1.0, 1.0) * 32767.0).astype("<i2")
    mono, stereo = tmp_path / "mono.wav", tmp_path / "stereo.wav"
    for path, data in ((mono, q[:1]), (stereo, q)):
        with wave.open(str(path), "wb") as w:
            w.setnchannels(data.shape[0])
            w.setsampwidth(2)
            w.setframerate(rate)
            w.writeframes(np.ascontiguousarray(data.T).tobytes())
    stems, out_rate = repet.separate_wav_repet(str(mono), width_sec=WIDTH_SEC)
    assert out_rate == rate and tuple(stems.shape) == (2, N_AUDIO) and bool(torch.isfinite(stems).all()) and float(stems.abs().max()) > 0.1
    n16 = -(-N_AUDIO * 16000 // rate)
    stems, out_rate = repet.separate_wav_repet(str(mono), out_rate=None, width_sec=WIDTH_SEC, residual=True)
    assert out_rate == 16000 and tuple(stems.shape) == (3, n16)
    stems, out_rate = repet.separate_wav_repet(str(stereo), width_sec=WIDTH_SEC, k=8)
    assert out_rate == rate and tuple(stems.shape) == (2, 2, N_AUDIO) and bool(torch.isfinite(stems).all())
    stems, out_rate = repet.separate_wav_repet(str(stereo), out_rate=8000, mono=True, width_sec=WIDTH_SEC)
    assert out_rate == 8000 and tuple(stems.shape) == (2, -(-n16 * 8000 // 16000))
