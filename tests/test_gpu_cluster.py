"""Clustering on the GPU against the restatement of tests/cluster_ref.py: the statistics and the start inside the a-priori bound of
include/glowk.h (against the longdouble restatement), the update, the posteriors, labels, bitwise reproducibility (runs, batches, staged
calls against the fused loop, symmetric covariances), the status paths, 30 iterations against the restatement's own sensitivity to the
order of its sums, the spatial features, the input forms, the two scenes and the wav paths.

Fractions of the allowed error measured on an MI355X are in profiles/cluster_accuracy.json and DESIGN section 27."""
import functools
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import cluster
from tests import cluster_ref as R

pytestmark = pytest.mark.gpu
SHAPES = R.GPU_SHAPES
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
KEYS = ("weights", "means", "covariances", "origin", "total")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dtype=dtype) if dtype is not None else t.cuda()


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(i):
    """(F, w, states): the inputs of shape i and one valid state per signal; computed once, never modified."""
    N, D, J, rows, frames = SHAPES[i]
    F, w = R.inputs(SHAPES[i])
    return F, w, [R.random_state(F[n], w[n], J) for n in range(N)]


def stack_state(states):
    return {k: np.stack([np.asarray(s[k], np.float64) for s in states]) for k in KEYS}


def signal_state(st, n):
    return {k: host(st[k])[n] for k in KEYS}


def report(name, frac):
    print("%s: worst fraction of the allowed error %.3g" % (name, frac))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_stats_lie_inside_the_bound(i):
    N, D, J, rows, frames = SHAPES[i]
    F, w, states = case(i)
    S = host(cluster.stats(F, w, stack_state(states)))
    assert S.shape == (N, R.stat_size(D, J))
    worst = 0.0
    for n in range(N):
        ref, b = R.stats_longdouble(F[n], w[n], states[n]), R.stats_bound(F[n], w[n], states[n])
        frac = np.abs((S[n] - ref).astype(np.float64)) / b
        worst = max(worst, float(frac.max()))
        assert (frac <= 1.0).all(), (n, frac.max())
    report("stats %s" % IDS[i], worst)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_init_matches_the_restatement(i):
    """origin and total are statistics of one cluster with r = 1: inside the bound with e = 0 (chain + 4 roundings per term).  The start is
    64 power-iteration steps away from them: 1e-9 of each parameter's scale."""
    N, D, J, rows, frames = SHAPES[i]
    F, w, _ = case(i)
    st = cluster.init(F, w, J)
    worst = 0.0
    for n in range(N):
        ref = R.init(F[n], w[n], J)
        x, ww = F[n].astype(np.float64).reshape(D, -1), w[n].astype(np.float64).reshape(-1)
        bound = R.EPS * (R.chain(rows, frames) + 4)
        W = host(st["total"])[n]
        assert abs(W - ref["total"]) <= bound * ww.sum()
        num_bound = bound * (ww[None] * np.abs(x)).sum(axis=1)
        o_bound = (num_bound + np.abs(ref["origin"]) * (bound * ww.sum() + R.EPS * W)) / W * 1.01
        frac = np.abs(host(st["origin"])[n] - ref["origin"]) / o_bound
        worst = max(worst, float(frac.max()))
        assert (frac <= 1.0).all()
        scale = np.sqrt(np.abs(ref["covariances"]).max())
        assert np.abs(host(st["means"])[n] - ref["means"]).max() <= 1e-9 * max(scale, np.abs(ref["means"]).max())
        assert np.abs(host(st["covariances"])[n] - ref["covariances"]).max() <= 1e-9 * scale * scale
        assert np.array_equal(host(st["weights"])[n], ref["weights"]) and host(st["status"])[n] == 0
    report("init origin %s" % IDS[i], worst)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_update_from_given_statistics(i):
    """Per element 2^-53 64 D^2 (1 + cond(Sigma_j)) of the element's scale (include/glowk.h)."""
    N, D, J, rows, frames = SHAPES[i]
    F, w, states = case(i)
    S = np.stack([R.stats(F[n], w[n], states[n]) for n in range(N)])
    new = cluster.update(S, stack_state(states), 1e-6)
    worst = 0.0
    for n in range(N):
        ref, ll = R.update(S[n], states[n], 1e-6)
        tol = R.update_tolerance(ref, D)
        sig_scale = np.abs(ref["covariances"]).reshape(J, -1).max(axis=1)
        mu_scale = np.maximum(np.abs(ref["means"]).max(axis=1), np.sqrt(sig_scale))
        got = signal_state(new, n)
        fr = [np.abs(got["weights"] - ref["weights"]) / tol,
              np.abs(got["means"] - ref["means"]).max(axis=1) / (tol * mu_scale),
              np.abs(got["covariances"] - ref["covariances"]).reshape(J, -1).max(axis=1) / (tol * sig_scale)]
        worst = max(worst, max(float(f.max()) for f in fr))
        assert all((f <= 1.0).all() for f in fr), fr
        assert abs(host(new["log_likelihood"])[n] - ll) <= 4 * R.EPS * abs(ll) and host(new["status"])[n] == ref["status"]
        assert np.array_equal(got["covariances"], got["covariances"].transpose(0, 2, 1))
    report("update %s" % IDS[i], worst)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_posteriors_masks_and_spectra(i):
    N, D, J, rows, frames = SHAPES[i]
    F, w, states = case(i)
    rng = np.random.default_rng(i)
    X = (rng.normal(size=(N, 2, rows, frames)) + 1j * rng.normal(size=(N, 2, rows, frames))).astype(np.complex64)
    st = stack_state(states)
    m = host(cluster.posteriors(F, st))
    Y = host(cluster.posteriors(F, st, X))
    assert m.dtype == np.float32 and m.shape == (N, J, rows, frames) and Y.dtype == np.complex64 and Y.shape == (N, J, 2, rows, frames)
    worst = 0.0
    for n in range(N):
        r, b = R.posteriors(F[n], states[n]), R.posterior_bound(F[n], states[n])
        frac = np.abs(m[n].astype(np.float64) - r) / (2.0 ** -24 + b)
        worst = max(worst, float(frac.max()))
        assert (frac <= 1.0).all()
    assert np.abs(m.astype(np.float64).sum(axis=1) - 1.0).max() <= J * 2.0 ** -23
    want = m[:, :, None] * X[:, None]                                                    # one float32 rounding per component
    assert np.array_equal(Y.real, m[:, :, None] * X.real[:, None]) and np.array_equal(Y.imag, m[:, :, None] * X.imag[:, None]), np.abs(Y - want).max()
    report("posteriors %s" % IDS[i], worst)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_labels(i):
    N, D, J, rows, frames = SHAPES[i]
    F, w, states = case(i)
    lab = host(cluster.labels(F, stack_state(states)))
    assert lab.shape == (N, J, rows, frames) and np.array_equal(lab.sum(axis=1), np.ones((N, rows, frames), np.float32))
    for n in range(N):
        assert R.label_ties(F[n], states[n]) == 0                                        # the premise (also checked on the CPU)
        differ = (lab[n] != R.labels(F[n], states[n])).any(axis=0)
        assert differ.sum() == 0


@pytest.mark.parametrize("i", [1, 2, 4], ids=[IDS[1], IDS[2], IDS[4]])
def test_runs_batches_and_staged_calls_agree_bit_for_bit(i):
    N, D, J, rows, frames = SHAPES[i]
    F, w, states = case(i)
    Fd, wd = dev(F), dev(w)
    n_iter = 3
    a = cluster.fit(Fd, wd, J, n_iter=n_iter, tol=0.0)
    b = cluster.fit(Fd, wd, J, n_iter=n_iter, tol=0.0)
    keys = KEYS + ("log_likelihood", "iterations", "status")
    for k in keys:
        assert torch.equal(a[k], b[k]), k                                                # a repeated run
    last = N - 1
    alone = cluster.fit(Fd[last], wd[last], J, n_iter=n_iter, tol=0.0)
    for k in keys:
        assert torch.equal(alone[k], a[k][last]), k                                      # a signal alone against the batch
    st = cluster.init(Fd, wd, J)
    lls = []
    for _ in range(n_iter):
        st = cluster.update(cluster.stats(Fd, wd, st), st, 1e-6)
        lls.append(st["log_likelihood"])
    for k in KEYS:
        assert torch.equal(st[k], a[k]), k                                               # staged calls against the fused loop
    assert torch.equal(torch.stack(lls, dim=-1), a["log_likelihood"])
    assert torch.equal(a["covariances"], a["covariances"].transpose(-1, -2))
    assert (a["iterations"] == n_iter).all()
    m1, m2 = cluster.posteriors(Fd, a), cluster.posteriors(Fd[last], alone)
    assert torch.equal(m1[last], m2)


def test_zero_weights_inside_a_batch():
    N, D, J, rows, frames = SHAPES[1]
    F, w, _ = case(1)
    w0 = w.copy()
    w0[1] = 0.0
    a, b = cluster.fit(F, w0, J, n_iter=4, tol=0.0), cluster.fit(F, w, J, n_iter=4, tol=0.0)
    assert host(a["status"]).tolist() == [0, R.STATUS_ZERO_WEIGHT, 0] and host(a["iterations"]).tolist() == [4, 0, 4]
    for k in KEYS:
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][2], b[k][2]), k        # the neighbours are unchanged
    m = host(cluster.posteriors(F, a))
    assert np.array_equal(m[1], np.full((J, rows, frames), np.float32(1.0 / J)))
    assert torch.equal(cluster.posteriors(F, a)[0], cluster.posteriors(F, b)[0])
    assert np.isnan(host(a["log_likelihood"])[1]).all()


def test_a_far_mean_gives_a_dead_cluster():
    N, D, J, rows, frames = SHAPES[3]
    F, w, _ = case(3)
    start = R.init(F[0], w[0], J)
    means = start["means"].copy()
    means[2] = 1e4
    got = cluster.fit(F[0], w[0], J, n_iter=3, tol=0.0, means=means)
    assert host(got["status"]) & R.STATUS_DEAD and host(got["weights"])[2] == 0.0
    assert np.array_equal(host(got["means"])[2], means[2])
    m = host(cluster.posteriors(F[0], got))
    assert (m[2] == 0.0).all() and np.abs(m.sum(axis=0) - 1.0).max() <= J * 2.0 ** -23
    ref = R.fit(F[0], w[0], J, n_iter=3, tol=0.0, means=means)
    assert ref["status"] & R.STATUS_DEAD and np.abs(host(got["means"]) - ref["means"]).max() <= 1e-9 * 1e4


def test_a_large_tol_stops_one_signal_early_and_freezes_it():
    N, D, J, rows, frames = SHAPES[3]
    F, w, _ = case(3)
    lls = [R.fit(F[n], w[n], J, n_iter=12, tol=0.0)["log_likelihood"] for n in range(N)]
    rel = [np.diff(l) / np.abs(l[1:]) for l in lls]
    stops = None
    for tol in sorted(set(np.concatenate(rel)) | {0.0})[::-1]:                            # a tol that separates the two signals' stops
        k = [int(np.argmax(r <= tol)) + 2 if (r <= tol).any() else 12 for r in rel]
        if k[0] != k[1] and min(k) < 12:
            stops, tol = k, float(tol) * (1 + 1e-9) + 1e-300
            break
    assert stops is not None
    got = cluster.fit(F, w, J, n_iter=12, tol=tol)
    assert host(got["iterations"]).tolist() == stops
    for n in range(N):
        part = cluster.fit(F[n], w[n], J, n_iter=stops[n], tol=0.0)
        for k in KEYS:
            assert torch.equal(part[k], got[k][n]), k                                    # frozen at its state at the stop
        ll = host(got["log_likelihood"])[n]
        assert np.isfinite(ll[:stops[n]]).all() and np.isnan(ll[stops[n]:]).all()


@pytest.mark.parametrize("i", [1, 2, 3], ids=[IDS[1], IDS[2], IDS[3]])
def test_fit_30_iterations_against_the_restatement(i):
    """Allowed: 32 times the difference between the restatement with its cells summed in natural and in reversed order, with a floor of
    1e-12 of the parameter's scale (the device also differs in exp and log by an ulp or two)."""
    N, D, J, rows, frames = SHAPES[i]
    F, w, _ = case(i)
    got = cluster.fit(F, w, J, n_iter=30, tol=0.0)
    worst = 0.0
    for n in range(N):
        a, b = R.fit(F[n], w[n], J, n_iter=30, tol=0.0), R.fit(F[n], w[n], J, n_iter=30, tol=0.0, reverse=True)
        mine = signal_state(got, n)
        for k, scale in (("weights", 1.0), ("means", np.abs(a["means"]).max()), ("covariances", np.abs(a["covariances"]).max())):
            allowed = np.maximum(32 * np.abs(a[k] - b[k]), 1e-12 * scale)
            frac = np.abs(mine[k] - a[k]) / allowed
            worst = max(worst, float(frac.max()))
            assert (frac <= 1.0).all(), (k, frac.max())
        assert host(got["status"])[n] == a["status"] and host(got["iterations"])[n] == 30
    report("fit 30 %s" % IDS[i], worst)


@pytest.mark.parametrize("delay,p", [(False, 1.0), (True, 2.0), (True, 0.7)])
def test_spatial_features_within_one_ulp(delay, p):
    rng = np.random.default_rng(5)
    X = (rng.normal(size=(2, 2, 17, 45)) + 1j * rng.normal(size=(2, 2, 17, 45))).astype(np.complex64)
    X[0, 0, 3, 4] = 0
    X[0, :, 5, 6] = 0
    X[1, 1, 7] = 0
    Fd, wd = cluster.spatial_features(X, delay=delay, max_delay=3.0, p=p)
    assert Fd.dtype == torch.float32 and Fd.shape == (2, 2 if delay else 1, 17, 45) and wd.shape == (2, 17, 45)
    for n in range(2):
        Fr, wr = R.spatial_features(X[n], delay, 3.0, p)
        for got, ref in ((host(Fd)[n], Fr), (host(wd)[n], wr)):
            ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
            assert (np.abs(got.astype(np.float64) - ref) <= ulp).all()
        assert (host(wd)[n][0] == 0).all() and host(wd)[0][5, 6] == 0 and (host(wd)[n][1:] >= 0).all()
    if delay:
        assert host(Fd)[0, 1, 3, 4] == 0 and np.abs(host(Fd)[:, 1]).max() <= 3.0


def test_input_forms():
    N, D, J, rows, frames = SHAPES[1]
    F, w, states = case(1)
    st = stack_state(states)
    base = cluster.stats(F, w, st)
    Fd = dev(F)
    wide = torch.zeros((N, D, rows, 2 * frames), device="cuda")
    wide[..., ::2] = Fd
    assert torch.equal(cluster.stats(wide[..., ::2], dev(w).double(), {k: dev(v) for k, v in st.items()}), base)      # non-contiguous, other dtypes
    assert torch.equal(cluster.stats(F[0], w[0], {k: v[0] for k, v in st.items()}), base[0])                          # one signal, numpy
    rng = np.random.default_rng(2)
    X = (rng.normal(size=(N, 2, rows, frames)) + 1j * rng.normal(size=(N, 2, rows, frames))).astype(np.complex64)
    m = cluster.posteriors(F, st)
    stereo = cluster.posteriors(F, st, X)
    mono = cluster.posteriors(F, st, X[:, 0])
    one = cluster.posteriors(F, st, X[:, :1])
    single = cluster.posteriors(F[0], {k: v[0] for k, v in st.items()}, X[0, 0])
    assert mono.shape == (N, J, rows, frames) and one.shape == (N, J, 1, rows, frames) and single.shape == (J, rows, frames)
    assert torch.equal(mono, stereo[:, :, 0]) and torch.equal(one[:, :, 0], mono) and torch.equal(single, mono[0])
    assert torch.equal(cluster.mask_features(m[:, 0], host(m[:, 1])), m[:, :2].contiguous())


@pytest.mark.parametrize("rows,frames,pans,density", [(33, 47, (0.3, 1.2), 0.15), (65, 120, (0.2, 0.8, 1.4), 0.1)])
def test_spatial_on_the_panned_scenes(rows, frames, pans, density):
    """The restatement's SDR gains over X / J with the principal-axis start, p = 1, 30 iterations: 8.92 / 8.92 dB and 6.71 / 3.90 / 7.64 dB."""
    X, imgs = R.spatial_scene(rows, frames, pans, density)
    J = len(pans)
    Y, model = cluster.spatial(X, J, n_iter=30, tol=0.0, return_model=True)
    assert Y.shape == (J, 2, rows, frames) and Y.dtype == torch.complex64
    means = host(model["means"])[:, 0]
    assert (np.diff(means) > 0).all()
    Yr, st = R.spatial_separate(X, J, n_iter=30)
    gain, ref = R.sdr_gains(host(Y), X, imgs), R.sdr_gains(Yr, X, imgs)
    print("spatial %dx%d: SDR gains %s dB, the restatement's %s dB" % (rows, frames, np.round(gain, 3), np.round(ref, 3)))
    assert (np.abs(gain - ref) <= 0.01).all() and (gain >= ref - 1.0).all()
    masks = cluster.spatial(X, J, n_iter=30, tol=0.0, mask=True)
    assert masks.shape == (J, rows, frames) and torch.equal(Y, masks[:, None] * dev(X)[None])


def test_ensemble_on_the_melody_scene():
    """Both stems' SDR gains are at least the median of the three primitives' own, and within 0.05 dB of the restatement fed with the
    device's primitive masks.  Measured on an MI355X, gains over the mixture (accompaniment / lead): ensemble 3.19 / 1.61 dB, the
    restatement the same; melody 8.37 / 6.79, hpss 0.81 / -0.77, repet_sim 1.63 / 0.04."""
    from audiosourcesep_amd import hpss, melody, repet
    X_lead, X_acc, X_mix = R.melody_scene()
    X_mix = X_mix.astype(np.complex64)
    mag = dev(X_mix).abs()                                                               # the magnitudes ensemble takes: torch's, on the device
    prim = {"melody": melody.melody(mag, mask=True)[0], "hpss": hpss.hpss(mag, mask=True)[1], "repet_sim": repet.repet_sim(mag, mask=True)[1]}
    base = [R.sdr(X_mix, X_acc), R.sdr(X_mix, X_lead)]                                    # gains over the mixture itself; source 0 the background
    own = np.array([[R.sdr((1 - host(m)) * X_mix, X_acc) - base[0], R.sdr(host(m) * X_mix, X_lead) - base[1]] for m in prim.values()])
    Y, model = cluster.ensemble(X_mix, primitives=("melody", "hpss", "repet_sim"), n_iter=30, tol=0.0, return_model=True)
    assert Y.shape == (2,) + X_mix.shape and Y.dtype == torch.complex64
    assert torch.equal(model["features"], torch.stack(list(prim.values())))
    gain = np.array([R.sdr(host(Y)[0], X_acc) - base[0], R.sdr(host(Y)[1], X_lead) - base[1]])
    r, st = R.ensemble_separate([host(m) for m in prim.values()], host(mag), 2, n_iter=30)
    ref = np.array([R.sdr(r[0] * X_mix, X_acc) - base[0], R.sdr(r[1] * X_mix, X_lead) - base[1]])
    print("ensemble: SDR gains (accompaniment, lead) %s dB, the restatement's %s dB, the primitives' %s" % (np.round(gain, 2), np.round(ref, 2), np.round(own, 2).tolist()))
    assert (gain >= np.median(own, axis=0)).all()
    assert (np.abs(gain - ref) <= 0.05).all()
    ready = cluster.ensemble(X_mix, primitives=(prim["melody"], ("hpss", {}), host(prim["repet_sim"])), n_iter=30, tol=0.0)
    assert torch.equal(ready, Y)
    real = cluster.ensemble(mag, primitives=list(prim.values()), n_iter=30, tol=0.0, mask=True)
    assert real.dtype == torch.float32 and torch.equal(real, cluster.posteriors(model["features"], model))


def _write_wav(path, y, rate):
    data = (np.clip(y, -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(data.shape[0])
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(data.T.tobytes())


def test_the_wav_paths_return_the_inputs_length_and_rate(tmp_path):
    rate, n = 22050, 9001
    t = np.arange(n) / rate
    rng = np.random.default_rng(0)
    a, b = 0.3 * np.sin(2 * np.pi * 440 * t), 0.3 * np.sign(np.sin(2 * np.pi * 3 * t)) * rng.normal(size=n) * 0.3
    y = np.stack([0.9 * a + 0.2 * b, 0.3 * a + 0.8 * b])
    _write_wav(tmp_path / "stereo.wav", y, rate)
    _write_wav(tmp_path / "mono.wav", y[:1], rate)
    stems, r = cluster.separate_wav_spatial(str(tmp_path / "stereo.wav"), 2, n_iter=5)
    assert r == rate and stems.shape == (2, 2, n) and torch.isfinite(stems).all()
    stems, r = cluster.separate_wav_ensemble(str(tmp_path / "mono.wav"), primitives=("hpss", "repet_sim"), n_iter=5, residual=True)
    assert r == rate and stems.shape == (3, n) and torch.isfinite(stems).all()
    stems, r = cluster.separate_wav_ensemble(str(tmp_path / "stereo.wav"), primitives=("hpss",), n_iter=2, out_rate=None)
    assert r == 16000 and stems.shape[:2] == (2, 2)
