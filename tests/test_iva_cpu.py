"""AuxIVA / ILRMA without a GPU: ``iva.py`` refuses bad arguments before the library is loaded, and the fp64 restatement
(tests/iva_ref.py) has the properties the GPU tests lean on: its costs never rise, it separates the synthetic scenes, and its images
add up to the mixture."""
import functools

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, iva
from tests import iva_ref as I

SCENES = [(2, 65, 200), (3, 33, 300), (4, 17, 400)]
ILRMA_SCENES = [(2, 65, 200), (2, 129, 257)]


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def _x(shape, dtype=np.complex64):
    return np.zeros(shape, dtype)


def test_bad_arguments_are_refused_before_the_library_loads(no_library, tmp_path):
    good, w = _x((2, 3, 5)), np.broadcast_to(np.eye(2, dtype=np.complex128), (3, 2, 2)).copy()
    for bad in (_x((1, 3, 5)), _x((5, 3, 5)), _x((2, 3, 1)), _x((3, 3, 2)), _x((2, 4097, 2)), _x((2, 1, 32769)), _x((3, 5)),
                _x((2, 3, 5), np.float32), _x((1, 2, 2, 3, 5))):
        for call in (iva.init, iva.auxiva, iva.ilrma, lambda x: iva.demix(x, w), lambda x: iva.images(x, w), lambda x: iva.source_weights(x, w),
                     lambda x: iva.covariances(x, phi=np.ones((2, 5))), lambda x: iva.power(x, w)):
            with pytest.raises(ValueError):
                call(bad)
    for bad_w in (np.eye(2), w[:2], w.real, np.zeros((3, 3, 3), np.complex128), np.zeros((1, 3, 2, 2), np.complex128)):
        for call in (iva.demix, iva.images, iva.source_weights, iva.power, lambda x, v: iva.auxiva(x, W=v), lambda x, v: iva.ilrma(x, W=v)):
            with pytest.raises(ValueError):
                call(good, bad_w)
    for kw in (dict(n_iter=-1), dict(n_iter=1.5), dict(n_iter=True), dict(n_iter=100001), dict(model="cauchy"), dict(model=0), dict(return_model=1)):
        with pytest.raises(ValueError):
            iva.auxiva(good, **kw)
    for kw in (dict(n_components=0), dict(n_components=129), dict(n_components=2.0), dict(n_iter=-1), dict(seed=-1), dict(seed=1.0), dict(return_model="yes")):
        with pytest.raises(ValueError):
            iva.ilrma(good, **kw)
    for b, a, n in ((np.ones((2, 3, 4)), np.ones((2, 5, 5)), 1), (np.ones((2, 4, 4)), np.ones((2, 4, 5)), 1), (np.ones((2, 3, 129)), np.ones((2, 129, 5)), 1),
                    (np.ones((2, 3, 4), np.complex64), np.ones((2, 4, 5)), 1), (np.ones((2, 3, 4)), np.ones((2, 4, 5)), -1), (np.ones((2, 3, 4)), np.ones((2, 4, 5)), 1.5)):
        with pytest.raises(ValueError):
            iva.ilrma_fit(good, w, b, a, n)
    with pytest.raises(ValueError):
        iva.ilrma_fit(good, w[:2], np.ones((2, 3, 4)), np.ones((2, 4, 5)))
    with pytest.raises(ValueError):
        iva.source_weights(good, w, model="student")
    for kw in (dict(), dict(phi=np.ones((2, 5)), factors=(np.ones((2, 3, 1)), np.ones((2, 1, 5)))), dict(phi=np.ones((2, 4))), dict(phi=np.ones((2, 5), np.complex64)),
               dict(factors=(np.ones((2, 3, 1)), np.ones((2, 2, 5)))), dict(factors=np.ones((2, 3, 1)))):
        with pytest.raises(ValueError):
            iva.covariances(good, **kw)
    for bad_v in (np.zeros((3, 2, 2, 2)), np.zeros((3, 2, 2), np.complex128), np.zeros((2, 2, 2, 2), np.complex128)):
        with pytest.raises(ValueError):
            iva.ip_update(w, bad_v)
    with pytest.raises(ValueError):
        iva.ip_update(np.zeros((3, 5, 5), np.complex128), np.zeros((3, 5, 5, 5), np.complex128))
    with pytest.raises(ValueError):
        iva.inverse(np.zeros((3, 2, 3), np.complex128))
    with pytest.raises(ValueError):
        iva.normalize(good, w, np.ones((2, 4, 2)))
    with pytest.raises(ValueError):
        iva.init_factors(np.ones((2, 3, 5)), 0)
    with pytest.raises(ValueError):
        iva.init_factors(-np.ones((2, 3, 5)), 2)
    audio_ok = np.zeros((2, 4000), np.float32)
    for y, kw in ((np.zeros((1, 4000), np.float32), {}), (np.zeros((5, 4000), np.float32), {}), (np.zeros(4000, np.float32), {}), (np.zeros((2, 1000), np.float32), {}),
                  (audio_ok, dict(method="duet")), (audio_ok, dict(n_iter=-1)), (audio_ok, dict(model="x")), (audio_ok, dict(n_components=0)),
                  (audio_ok.astype(np.complex64), {})):
        with pytest.raises(ValueError):
            iva.iva_audio(y, **kw)
    missing = str(tmp_path / "missing.wav")
    for kw in (dict(out_rate="file"), dict(out_rate=10), dict(num_sources=2), dict(method="nmf"), dict(n_iter=2.5)):
        with pytest.raises(ValueError):                    # refused before the file is opened: it does not exist
            iva.separate_wav_iva(missing, **kw)


@functools.lru_cache(maxsize=None)
def auxiva_chain(shape):
    X, mix, _ = I.scene(*shape)
    return X, mix, I.auxiva(X, 30)


@functools.lru_cache(maxsize=None)
def ilrma_chain(shape):
    X, mix, _ = I.scene(*shape)
    W = I.identity(X)
    b, a = I.init_factors(I.power(X, W), 4, 1)
    states = [(W, b, a)]
    for _ in range(60):
        states.append(I.ilrma_step(X, *states[-1]))
    return X, mix, states


@pytest.mark.parametrize("shape", SCENES, ids=str)
def test_auxiva_cost_never_rises_and_the_scene_separates(shape):
    X, mix, Ws = auxiva_chain(shape)
    J = np.array([float(I.cost_iva(X, W)) for W in Ws])
    step = np.diff(J)
    print("J_IVA %s: %.6f -> %.6f, largest step %.3e" % (shape, J[0], J[-1], step.max()))
    assert np.all(step <= 1e-12 * (1 + np.abs(J[:-1])))               # the evaluation's own rounding
    start, end = I.interference_db(Ws[0], mix), I.interference_db(Ws[-1], mix)
    print("interference ratio %s: %.1f dB -> %.1f dB" % (shape, start, end))
    assert start < 5.0 and end > 20.0


@pytest.mark.parametrize("shape", ILRMA_SCENES, ids=str)
def test_ilrma_cost_never_rises_and_the_scene_separates(shape):
    X, mix, states = ilrma_chain(shape)
    J = np.array([float(I.cost_ilrma(X, *s)) for s in states])
    step = np.diff(J)
    print("J_ILRMA %s: %.6f -> %.6f, largest step %.3e" % (shape, J[0], J[-1], step.max()))
    # the factors and P are rounded to float32 once per iteration: 2^-24 relative on every rho, 2 M R terms of the cost per frame
    assert np.all(step <= 2.0 ** -24 * 2 * shape[0] * shape[1] * 4)
    end = I.interference_db(states[-1][0], mix)
    print("interference ratio %s: %.1f dB" % (shape, end))
    assert end > 25.0
    lam = I.lambdas(X, states[-1][0])
    assert np.allclose(lam, 1.0, atol=1e-12)                            # step 5 leaves every source at unit mean power


@pytest.mark.parametrize("shape", SCENES, ids=str)
def test_images_add_up_to_the_mixture(shape):
    X, _, Ws = auxiva_chain(shape)
    img = I.images(X, Ws[-1])
    assert img.shape == (shape[0], shape[0]) + shape[1:]
    rel = np.abs(img.sum(axis=0) - X).max() / np.abs(X).max()
    print("images %s: %.2e" % (shape, rel))
    assert rel < 1e-13


def test_degenerate_rows_keep_their_matrix_and_singular_rows_get_zero_images():
    X = np.array(I.stft((1, 2, 4, 6))[0])
    X[:, 0] = 0                                                         # a silent row
    W0 = I.perturbed_identity((1, 2, 4, 6))[0]
    W1 = I.auxiva_step(X, W0)
    assert np.array_equal(W1[0], W0[0]) and not np.array_equal(W1[1], W0[1]) and np.isfinite(W1).all()
    Z = I.auxiva_step(np.zeros_like(X), W0)
    assert np.array_equal(Z, W0)
    W1[2] = [[1, 2], [2, 4]]
    img = I.images(X, W1)
    assert np.all(img[:, :, 2] == 0) and np.isfinite(img).all() and np.abs(img[:, :, 1].sum(axis=0) - X[:, 1]).max() < 1e-12 * np.abs(X).max()


def test_a_permuted_frame_order_stays_far_inside_the_step_bound():
    """The bound the GPU tests hold the device to, 2^-53 (T + 64 M) (1 + c_f), against the restatement itself with the frames added
    in another order."""
    for shape in [(1, 2, 33, 65), (1, 3, 5, 64), (1, 4, 17, 257)]:
        X = I.stft(shape)[0]
        W0 = I.perturbed_identity(shape)[0]
        ref, cond = I.auxiva_step(X, W0, return_cond=True)
        other = I.auxiva_step(X, W0, order=np.random.default_rng(3).permutation(shape[-1]))
        frac = (I.row_error(other, ref) / I.step_bound(shape[-1], shape[1], cond)).max()
        print("permuted frames %s: %.4f of the bound" % (shape, frac))
        assert frac < 0.05
