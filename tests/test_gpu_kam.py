"""Kernel additive modelling on the GPU (audiosourcesep_amd/kam.py, csrc/glowk_kam.h) against the restatement of tests/kam_ref.py: the
sparse-kernel median bit for bit (it selects), and against ``hpss.median_filter`` where no neighbour leaves the plane; the back-fitting
step inside bars derived from its operations; the loop bit for bit against its staged rounds, each stage against the restatement on the
device's own inputs; where the wrappers write (tests/footprint.py); and audio end to end."""
import functools
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, hpss, kam, repet
from tests import kam_ref as R
from tests import repet_ref
from tests import test_gpu_footprint as FP

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                                         # half an ulp of 1 in float32


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def plane_kinds(shape, seed):
    """Continuous values; tied values (multiples of 1/2, many equal); zeros; -0 and +0 mixed among a few values."""
    rng = np.random.default_rng(seed)
    return {"continuous": rng.standard_normal(shape).astype(np.float32),
            "tied": (np.round(np.abs(rng.standard_normal(shape)) * 4.0) / 2.0).astype(np.float32),
            "zeros": np.zeros(shape, np.float32),
            "signed zeros": rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0], np.float32), shape)}


def random_table(n, max_row, max_frame, seed):
    """n offsets with duplicates: drawn from fewer than n distinct pairs."""
    rng = np.random.default_rng(seed)
    pool = np.stack([rng.integers(-max_row, max_row + 1, max(1, n // 2 + 1)), rng.integers(-max_frame, max_frame + 1, max(1, n // 2 + 1))], 1)
    return pool[rng.integers(0, len(pool), n)].astype(np.int32)


def spectra(shape, seed):
    """|N(0, 1)|^2 float32 with about 10 % exact zeros."""
    rng = np.random.default_rng(seed)
    x = (np.abs(rng.standard_normal(shape)) ** 2).astype(np.float32)
    x[rng.random(shape) < 0.1] = 0.0
    return x


def bits(a):
    return (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).view(np.uint32)


# ---- the median --------------------------------------------------------------------------------------------------------------------------------
MEDIAN_CASES = [
    ((1, 1, 1), "one offset out of range", np.array([[1, 0]], np.int32)),
    ((1, 3, 5), "n = 2", np.array([[0, 1], [1, -2]], np.int32)),
    ((2, 33, 65), "harmonic(31)", R.harmonic(31)),
    ((2, 33, 65), "percussive(31)", R.percussive(31)),
    ((2, 33, 65), "cross(9, 9)", R.cross(9, 9)),
    ((1, 65, 130), "n = 127 random with duplicates", random_table(127, 10, 20, 127)),
    ((3, 17, 64), "n = 8", random_table(8, 3, 5, 8)),
    ((1, 257, 97), "periodic(24, 8)", R.periodic(24, 8)),
    ((1, 4096, 3), "n = 5", random_table(5, 2, 2, 5)),
    ((1, 2, 4500), "n = 31", random_table(31, 1, 70, 31)),
]


@pytest.mark.parametrize("shape,name,table", MEDIAN_CASES, ids=["%s-%s" % ("x".join(map(str, c[0])), c[1]) for c in MEDIAN_CASES])
def test_median_bitwise(shape, name, table):
    """Compares select, and the even case is one exact fp32 add and a halving: no tolerance."""
    for kind, S in plane_kinds(shape, 1000 * shape[1] + shape[2] + len(table)).items():
        got = kam.median(S, table)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == shape
        np.testing.assert_array_equal(bits(got), bits(R.median(S, table)), err_msg=kind)
        if name == "one offset out of range":
            np.testing.assert_array_equal(bits(got), bits(S))


def test_the_neighbour_counts_of_the_cases_cover_none_odd_and_even():
    counts = set()
    for shape, name, table in MEDIAN_CASES:
        counts |= set(R.gather(np.zeros(shape[1:], np.float32), table)[1].sum(0).reshape(-1).tolist())
    assert {0, 1, 2, 17, 31, 127} <= counts and any(c % 2 == 0 and c > 2 for c in counts)


def test_median_equals_the_contiguous_filters_away_from_the_edges():
    """Where no neighbour leaves the plane, skipping and reflecting agree: the new filter is tied to the one pinned to scipy."""
    for kind, S in plane_kinds((2, 65, 130), 65130).items():
        x = torch.from_numpy(S).cuda()
        h, p = kam.median(x, kam.harmonic(31)), kam.median(x, kam.percussive(31))
        assert torch.equal(h[:, :, 15:-15].view(torch.int32), hpss.median_filter(x, 31, "frames")[:, :, 15:-15].view(torch.int32)), kind
        assert torch.equal(p[:, 15:-15].view(torch.int32), hpss.median_filter(x, 31, "rows")[:, 15:-15].view(torch.int32)), kind


def test_median_of_a_batch_a_rerun_and_a_device_tensor():
    S = plane_kinds((3, 17, 64), 3)["tied"]
    table = kam.cross(5, 7)
    whole = kam.median(S, table)
    assert torch.equal(whole.view(torch.int32), kam.median(torch.from_numpy(S).cuda(), table).view(torch.int32))
    assert torch.equal(whole.view(torch.int32), kam.median(S, table.tolist()).view(torch.int32))
    for i in range(3):
        assert torch.equal(whole[i].view(torch.int32), kam.median(S[i], table).view(torch.int32))
    assert tuple(kam.median(np.zeros((0, 3, 5), np.float32), table).shape) == (0, 3, 5)             # nsig = 0: a successful no-op


# ---- the back-fit ------------------------------------------------------------------------------------------------------------------------------
def backfit_inputs(J, seed=0):
    """(V [2, 33, 65], A [2, J, 33, 65]) with exact zeros in A, whole cells of zeros (the 1 / J rule) and one cell of subnormals."""
    A = spectra((2, J, 33, 65), 100 * J + seed)
    V = spectra((2, 33, 65), 100 * J + seed + 1) + np.float32(0.25)
    A[:, :, 5:9, 20:30] = 0.0
    A[0, :, 0, 0] = np.float32(1e-39)
    return V, A


def check_backfit(V, A, P, M, power, mask_bar):
    """The device's P and masks against the fp64 restatement of the same A and V."""
    J = A.shape[-3]
    wp, wm = R.backfit(V, A, power)
    bad = A.max(axis=-3) < R.TINY
    e_m = np.abs(M.astype(np.float64) - wm).max()
    e_p = np.abs(P.astype(np.float64) - wp) - (mask_bar * (1 + EPS) * V[..., None, :, :].astype(np.float64) + EPS * np.abs(wp))
    e_s = np.abs(M.astype(np.float64).sum(-3) - 1.0).max()
    print("backfit J = %d power %g: mask error %.3e (bar %.3e), sum of masks off 1 by %.3e" % (J, power, e_m, mask_bar, e_s))
    assert e_m <= mask_bar and e_p.max() <= 0 and e_s <= 4 * J * EPS
    assert bad.any() and (M.transpose(1, 0, 2, 3)[:, bad] == np.float32(1.0) / np.float32(J)).all()
    return e_m


@pytest.mark.parametrize("J", [1, 2, 3, 8])
@pytest.mark.parametrize("power", [1.0, 2.0])
def test_backfit_within_the_derived_bar(J, power):
    """Per mask: one quotient a / Z, one optional square, J - 1 additions and one quotient, each rounding once a value at most 1 (the
    sum at most J, relative to which the last quotient is taken): an absolute error of at most (J + 4) 2^-24.  P is that times v, plus
    the product's own rounding."""
    V, A = backfit_inputs(J)
    P, M = kam.backfit(V, A, power, return_masks=True)
    assert P.is_cuda and tuple(P.shape) == tuple(M.shape) == A.shape
    check_backfit(V, A, P.cpu().numpy(), M.cpu().numpy(), power, (J + 4) * EPS)
    assert torch.equal(kam.backfit(V, A, power).view(torch.int32), P.view(torch.int32))            # without the masks: the same P
    assert torch.equal(kam.backfit(V[1], A[1], power).view(torch.int32), P[1].view(torch.int32))   # a batch is its signals


# powf's device error cannot be derived: the largest deviation of the masks from the fp64 restatement on these inputs, measured on the
# MI355X (profiles/kam_accuracy.json), times four -- and no looser than the 1e-6 of tests/test_gpu_hpss.py.
POWF_MEASURED = {0.5: 1.0324e-07, 10.0: 1.8771e-07}
POWF_BAR = {p: min(4.0 * m, 1e-6) for p, m in POWF_MEASURED.items()}           # 4.13e-07 and 7.51e-07


@pytest.mark.parametrize("J", [1, 2, 3, 8])
@pytest.mark.parametrize("power", [0.5, 10.0])
def test_backfit_with_powf(J, power):
    V, A = backfit_inputs(J)
    P, M = kam.backfit(V, A, power, return_masks=True)
    check_backfit(V, A, P.cpu().numpy(), M.cpu().numpy(), power, POWF_BAR[power])


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
def staged(V, models, n_iter, power):
    """The rounds one call at a time -> (P, masks, [(P_in, A) of every round])."""
    v = torch.from_numpy(V).cuda() if not torch.is_tensor(V) else V
    P = torch.stack([v] * len(models), dim=-3)
    rounds, M = [], None
    for _ in range(n_iter):
        A = torch.stack([repet._median(P.select(-3, j).contiguous(), m) if torch.is_tensor(m) else kam.median(P.select(-3, j), m)
                         for j, m in enumerate(models)], dim=-3)
        rounds.append((P, A))
        P, M = kam.backfit(v, A, power, return_masks=True)
    return P, M, rounds


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def loop_case(mixed):
    V = spectra((2, 33, 97), 97 + mixed)                                                         # never modified
    if mixed:
        idx = repet.period_neighbors(torch.tensor([12, 7], dtype=torch.int32), 97, 5)              # [2, 97, 5]
        return V, (kam.harmonic(9), idx, kam.percussive(9)), 2, 1.0
    return V, (kam.harmonic(31), kam.percussive(31), kam.cross(9, 9)), 3, 2.0


@pytest.mark.parametrize("mixed", [0, 1], ids=["offset models", "with an index model"])
def test_fit_is_its_staged_rounds_bit_for_bit(mixed):
    V, models, n_iter, power = loop_case(mixed)
    P, M = kam.fit(V, models, n_iter, power, return_masks=True)
    assert P.is_cuda and tuple(P.shape) == tuple(M.shape) == (2, len(models), 33, 97) and P.dtype == torch.float32
    wp, wm, rounds = staged(V, models, n_iter, power)
    assert same_bits(P, wp) and same_bits(M, wm)
    for n in range(1, n_iter):
        assert same_bits(kam.fit(V, models, n, power), rounds[n][0])                                 # every shorter loop too
    # a second run, a run from a device tensor, without the masks, and a batch against its signals alone
    P2, M2 = kam.fit(torch.from_numpy(V.copy()).cuda(), models, n_iter, power, return_masks=True)
    assert same_bits(P, P2) and same_bits(M, M2) and same_bits(P, kam.fit(V, models, n_iter, power))
    for i in range(2):
        alone = tuple(m[i] if torch.is_tensor(m) else m for m in models)
        Pi, Mi = kam.fit(V[i], alone, n_iter, power, return_masks=True)
        assert same_bits(P[i], Pi) and same_bits(M[i], Mi)
    assert tuple(kam.fit(np.zeros((0, 33, 97), np.float32), tuple(m[:0] if torch.is_tensor(m) else m for m in models)).shape) == (0, len(models), 33, 97)


@pytest.mark.parametrize("mixed", [0, 1], ids=["offset models", "with an index model"])
def test_every_stage_of_the_loop_against_the_restatement(mixed):
    """One stage at a time on the device's own inputs, never the composed chain: the medians bit for bit, the back-fit inside its bar."""
    V, models, n_iter, power = loop_case(mixed)
    P, M, rounds = staged(V, models, n_iter, power)
    J = len(models)
    for k, (P_in, A) in enumerate(rounds):
        p_in, a = P_in.cpu().numpy(), A.cpu().numpy()
        if k == 0:
            assert all(np.array_equal(bits(p_in[:, j]), bits(V)) for j in range(J))                   # P_j = V to begin with
        for j, m in enumerate(models):
            want = repet_ref.gather_median(p_in[:, j], m.cpu().numpy()) if torch.is_tensor(m) else R.median(p_in[:, j], m)
            np.testing.assert_array_equal(bits(a[:, j]), bits(want), err_msg="round %d source %d" % (k, j))
        P_out = rounds[k + 1][0] if k + 1 < n_iter else P
        wp, wm = R.backfit(V, a, power)
        assert (np.abs(P_out.cpu().numpy() - wp) <= (J + 4) * EPS * (1 + EPS) * V[:, None] + EPS * np.abs(wp)).all()
    assert np.abs(M.cpu().numpy() - R.backfit(V, rounds[-1][1].cpu().numpy(), power)[1]).max() <= (J + 4) * EPS


def test_two_kernels_and_one_iteration_are_hpss():
    """(harmonic(31), percussive(31)), n_iter = 1, power 2: at the interior cells the filtered spectra are ``hpss``'s bit for bit, and both
    masks are fp32 evaluations of the same formula from them: the back-fit's derived bar, (J + 4) 2^-24 = 6 x 2^-24."""
    V = spectra((2, 65, 130), 65130)
    P, M = kam.fit(V, (kam.harmonic(31), kam.percussive(31)), n_iter=1, power=2.0, return_masks=True)
    mh, mp = hpss.hpss(V, kernel_size=31, power=2.0, mask=True)
    inner = (slice(None), slice(15, 65 - 15), slice(15, 130 - 15))
    e = max(float((M[:, 0][inner] - mh[inner]).abs().max()), float((M[:, 1][inner] - mp[inner]).abs().max()))
    print("KAM against hpss at the interior cells: masks %.3e apart (bar %.3e)" % (e, 6 * EPS))
    assert e <= 6 * EPS
    assert same_bits(kam.kam(V, (kam.harmonic(31), kam.percussive(31)), n_iter=1), P)
    assert same_bits(kam.kam(V, (kam.harmonic(31), kam.percussive(31)), n_iter=1, mask=True), M)
    X = (V * np.exp(1j * np.random.default_rng(1).uniform(-np.pi, np.pi, V.shape))).astype(np.complex64)
    Y = kam.kam(X, (kam.harmonic(31), kam.percussive(31)), n_iter=1)
    assert Y.dtype == torch.complex64 and tuple(Y.shape) == (2, 2, 65, 130)
    assert float((Y.sum(1) - torch.from_numpy(X).cuda()).abs().max()) <= 8 * EPS * float(V.max())     # the components add up to S


# ---- where the wrappers write --------------------------------------------------------------------------------------------------------------------
FOOT_SHAPES = [(1, 1, 1), (1, 3, 5), (2, 33, 65), (3, 17, 64), (1, 257, 97)]


@pytest.mark.parametrize("shape", FOOT_SHAPES, ids=["x".join(map(str, s)) for s in FOOT_SHAPES])
@pytest.mark.parametrize("name", ["median", "median_127", "backfit", "fit", "fit_index", "kam_mask"])
def test_footprint(name, shape):
    """Plain, poison 0xFF, poison 0x00: the guards stay untouched, the results are bitwise equal, the inputs are unmodified and the size
    query's bytes are an allocation of the call (tests/test_gpu_footprint.py's four assertions)."""
    nsig, rows, F = shape
    S = FP.spectra(shape, "kam")
    lib = _lib.load()
    models = (kam.harmonic(31), kam.percussive(5), kam.cross(3, 3))
    zero3 = np.zeros(3, np.int32)
    if name == "median":
        case = FP.Case(lambda: kam.median(S, kam.periodic(24, 8)), [S])
    elif name == "median_127":
        table = random_table(127, 10, 20, 1)
        case = FP.Case(lambda: kam.median(S, table), [S])
    elif name == "backfit":
        A = FP.spectra((nsig, 3, rows, F), "kam A")
        case = FP.Case(lambda: kam.backfit(S, A, 2.0, return_masks=True), [S, A])
    elif name == "fit":
        case = FP.Case(lambda: kam.fit(S, models, 2, 2.0, return_masks=True), [S], [lib.glowk_kam_work_bytes(nsig, rows, F, 3, kam._host(zero3))])
    elif name == "fit_index":
        idx = repet.period_neighbors(torch.full((nsig,), 3, dtype=torch.int32), F, 4)
        ks = np.array([0, 4, 0], np.int32)
        case = FP.Case(lambda: kam.fit(S, (models[0], idx, models[2]), 2, 1.0), [S, idx], [lib.glowk_kam_work_bytes(nsig, rows, F, 3, kam._host(ks))])
    else:
        case = FP.Case(lambda: kam.kam(S, models, 1, mask=True), [S], [lib.glowk_kam_work_bytes(nsig, rows, F, 3, kam._host(zero3))])
    for w in case.work:
        assert w > 0 and w % 8 == 0
        print("footprint %s %s: glowk_kam_work_bytes = %d" % (name, shape, w))
    FP.check_footprint("kam/%s" % name, case)


# ---- audio end to end ------------------------------------------------------------------------------------------------------------------------------
AUDIO_BAR = 1e-5                                         # of the peak: the whole-file inversion's bar (tests/test_gpu_hpss.py)
SOURCES = ("harmonic", "percussive", R.periodic(8, 4))
AUDIO_ARGS = dict(n_iter=3, power=2.0, kernel_size=9)


@functools.lru_cache(maxsize=None)
def scene():
    """(components [3, n] float32, y float32, the fp64 pipeline's stems of y, its fractions).  Never modified."""
    comps = np.stack(R.scene()).astype(np.float32)
    y = comps.sum(0)
    want = R.kam_audio(y.astype(np.float64), SOURCES, **AUDIO_ARGS)
    out = (comps, y, want, R.fractions(want, comps))
    for a in out:
        a.setflags(write=False)
    return out


def test_kam_audio_against_the_restatement_and_every_component_in_its_own_stem():
    comps, y, want, want_frac = scene()
    peak = float(np.abs(y).max())
    stems = kam.kam_audio(y.copy(), SOURCES, **AUDIO_ARGS)
    assert len(stems) == 3 and all(s.is_cuda and s.dtype == torch.float32 and tuple(s.shape) == y.shape for s in stems)
    got = np.stack([s.cpu().numpy() for s in stems])
    e_sum = float(np.abs(got.astype(np.float64).sum(0) - y).max() / peak)
    e_ref = float(np.abs(got - want).max() / peak)
    frac = R.fractions(got, comps)
    print("kam_audio: stems - restatement %.2e, sum of stems - y %.2e of the peak" % (e_ref, e_sum))
    print("fractions (component x stem), device:\n%s\nfp64 pipeline:\n%s" % (np.round(frac, 4), np.round(want_frac, 4)))
    assert e_sum <= AUDIO_BAR and e_ref <= AUDIO_BAR
    # each component mostly in its own stem: the threshold is the fp64 pipeline's own share on this input, less 0.05 for fp32
    assert (np.diag(want_frac) > 0.5).all() and (want_frac.argmax(1) == np.arange(3)).all()
    assert (np.diag(frac) >= np.diag(want_frac) - 0.05).all() and (frac.argmax(1) == np.arange(3)).all()


def test_kam_audio_channels_and_named_sources():
    y = scene()[1]
    two = np.stack([y, 0.5 * y[::-1]]).astype(np.float32)
    both = kam.kam_audio(two, SOURCES, **AUDIO_ARGS)
    assert len(both) == 3 and all(tuple(s.shape) == two.shape for s in both)
    for c in range(2):                                                             # a channel's stems depend on that channel alone
        alone = kam.kam_audio(two[c], SOURCES, **AUDIO_ARGS)
        assert all(torch.equal(both[j][c], alone[j]) for j in range(3))
    named = kam.kam_audio(torch.from_numpy(y.copy()).cuda(), ("harmonic", "percussive", "repeating", "similar"), n_iter=2, kernel_size=9,
                          period_sec=(0.2, 1.0), width_sec=0.1)
    assert len(named) == 4 and all(tuple(s.shape) == y.shape and bool(torch.isfinite(s).all()) for s in named)
    assert float((sum(named).cpu() - torch.from_numpy(y.copy())).abs().max()) <= AUDIO_BAR * float(np.abs(y).max())


def test_separate_wav_kam_returns_the_files_rate_and_length(tmp_path):
    rate, n = 22050, 30000
    y = sum(R.scene(n, rate))
    q = np.rint(np.clip(np.stack([y, 0.5 * y]) * 0.7, -1.0, 1.0) * 32767.0).astype("<i2")
    mono, stereo = tmp_path / "mono.wav", tmp_path / "stereo.wav"
    for path, data in ((mono, q[:1]), (stereo, q)):
        with wave.open(str(path), "wb") as w:
            w.setnchannels(data.shape[0])
            w.setsampwidth(2)
            w.setframerate(rate)
            w.writeframes(np.ascontiguousarray(data.T).tobytes())
    stems, out_rate = kam.separate_wav_kam(str(mono), sources=SOURCES, kernel_size=9)
    assert out_rate == rate and tuple(stems.shape) == (3, n) and bool(torch.isfinite(stems).all()) and float(stems.abs().max()) > 0.1
    stems, out_rate = kam.separate_wav_kam(str(stereo), out_rate=None)
    n16 = -(-n * 16000 // rate)
    assert out_rate == 16000 and tuple(stems.shape) == (2, 2, n16)
    stems, out_rate = kam.separate_wav_kam(str(stereo), out_rate=8000, mono=True, n_iter=1)
    assert out_rate == 8000 and tuple(stems.shape) == (2, -(-n16 * 8000 // 16000))
