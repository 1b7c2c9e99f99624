"""RPCA without a GPU: the restatement of tests/rpca_ref.py (the thresholding's optimality condition, the Gram route against the SVD
route, the Jacobi loops against ``numpy.linalg.eigh``, exact recovery of the synthetic scenes), the Python argument checks of
``audiosourcesep_amd.rpca`` (ValueError with the argument's name before the library is loaded), the boundary of the C entries (declared,
exported, bound with the header's signatures; every refusal before any device call), and the host-side rules the kernels share with the
host under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, rpca
from tests import rpca_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ("glowk_rpca_gemm_workspace_bytes", "glowk_rpca_gemm", "glowk_rpca_eigh_workspace_bytes", "glowk_rpca_eigh", "glowk_rpca_shrink",
         "glowk_rpca_svt_workspace_bytes", "glowk_rpca_svt", "glowk_rpca_workspace_bytes", "glowk_rpca_fit", "glowk_rpca_binary_mask")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def _symmetric_cases():
    rng = np.random.default_rng(5)
    out = []
    for n in (1, 2, 5, 16, 17, 33):
        Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        spectra = [rng.standard_normal(n), np.repeat([2.0, -1.0, 0.0], -(-n // 3))[:n], np.zeros(n), np.r_[3.0, np.zeros(n - 1)]]
        for d in spectra:
            G = (Q * d) @ Q.T
            out.append((G + G.T) / 2)
        out.append(np.diag(rng.standard_normal(n)))
    return out


def test_svt_satisfies_the_proximal_optimality_condition():
    """L = argmin tau ||L||_* + 1/2 ||L - A||_F^2 iff (A - L) / tau = U V^T + W with U^T W = 0, W V = 0 and ||W||_2 <= 1 for the thin
    SVD L = U S V^T."""
    rng = np.random.default_rng(1)
    for rows, frames in [(5, 9), (33, 80), (48, 20)]:
        A = rng.standard_normal((rows, frames))
        s = np.linalg.svd(A, compute_uv=False)
        tau = 0.5 * (s[2] + s[3])
        for route in (R.svt_svd, R.svt_gram, lambda a, t: R.svt_gram(a, t, "jacobi")):
            L = route(A, tau)
            Ul, sl, Vlt = np.linalg.svd(L, full_matrices=False)
            r = int((sl > 1e-9 * s[0]).sum())
            assert r == 3
            Ul, Vlt = Ul[:, :r], Vlt[:r]
            W = (A - L) / tau - Ul @ Vlt
            assert np.abs(Ul.T @ W).max() < 1e-10 and np.abs(W @ Vlt.T).max() < 1e-10 and np.linalg.norm(W, 2) <= 1 + 1e-10


def test_the_gram_route_equals_the_svd_route():
    """Per element relative to ||A||_2, over a whole chain on the 33 x 80 scene: the figure the device's bar is built on."""
    Lt, St = R.scene(33, 80)
    M = Lt + St
    Y, mu, mu_bar, lam = R.start(M)
    L = np.zeros_like(M)
    worst = 0.0
    for it in range(24):
        Ln, S, Yn, mun, A, _ = R.step(M, L, Y, mu, mu_bar, lam)
        n2 = np.linalg.norm(A, 2)
        for solver in ("eigh", "jacobi"):
            worst = max(worst, np.abs(R.svt_gram(A, 1.0 / mu, solver) - Ln).max() / n2)
        L, Y, mu = Ln, Yn, mun
    print("gram route against svd route over 24 iterations at 33 x 80: %.3e ||A||_2" % worst)
    assert worst < 1e-13


def test_the_jacobi_loops_reproduce_eigh():
    for G in _symmetric_cases():
        n = G.shape[0]
        l, V, sweeps, capped = R.jacobi(G)
        scale = max(np.abs(np.linalg.eigvalsh(G)).max(), 1e-300)
        assert not capped and 1 <= sweeps < R.MAX_SWEEPS
        assert np.abs(np.sort(l) - np.linalg.eigvalsh(G)).max() <= 64 * n * U * scale
        assert np.abs(G @ V - V * l).max() <= 64 * n * U * scale and np.abs(V.T @ V - np.eye(n)).max() <= 64 * n * U
        if np.array_equal(G, np.diag(np.diag(G))):
            assert sweeps == 1 and np.array_equal(V, np.eye(n)) and np.array_equal(l, np.diag(G))
    # every pair meets exactly once per sweep, the bye of an odd n included
    for n in (2, 5, 6, 17):
        m = n + (n & 1)
        seen = [pq for r in range(m - 1) for pq in R.rr_pairs(n, r)]
        assert len(seen) == len(set(seen)) == m * (m - 1) // 2


def test_exact_recovery_on_the_scenes():
    for (rows, frames), iters in (((33, 80), 24), ((65, 200), 22)):
        Lt, St = R.scene(rows, frames)
        L, S, it = R.rpca(Lt + St)
        eL, eS = np.linalg.norm(L - Lt) / np.linalg.norm(Lt), np.linalg.norm(S - St) / np.linalg.norm(St)
        print("scene %d x %d: %d iterations, L %.2e, S %.2e" % (rows, frames, it, eL, eS))
        assert it == iters and eL <= 1e-5 and eS <= 1e-5                                # the stop at 1e-7; the device's recovery bar
    Z = np.zeros((4, 6))
    L, S, it = R.rpca(Z)
    assert it == 0 and not L.any() and not S.any()


def test_the_arguments_are_checked_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    M = np.ones((4, 6), np.float32)
    bad = [
        (lambda: rpca.rpca_fit(np.ones(4)), "M"), (lambda: rpca.rpca_fit(np.ones((2050, 3))), "M"), (lambda: rpca.rpca_fit(np.ones((1, 65536))), "M"),
        (lambda: rpca.rpca_fit(M.astype(np.complex64)), "M"), (lambda: rpca.rpca_fit(M, gain=0.0), "gain"), (lambda: rpca.rpca_fit(M, gain=True), "gain"),
        (lambda: rpca.rpca_fit(M, tol=-1.0), "tol"), (lambda: rpca.rpca_fit(M, tol=float("nan")), "tol"), (lambda: rpca.rpca_fit(M, n_iter=-1), "n_iter"),
        (lambda: rpca.rpca_fit(M, n_iter=1.5), "n_iter"), (lambda: rpca.rpca_fit(M, n_iter=100001), "n_iter"),
        (lambda: rpca.eigh(np.ones((3, 4))), "square"), (lambda: rpca.eigh(np.ones((2050, 2050), np.float32)), "G"),
        (lambda: rpca.shrink(M, -1.0), "thr"), (lambda: rpca.shrink(M.astype(np.complex64), 1.0), "T"),
        (lambda: rpca.svt(M, np.ones(3)), "tau"), (lambda: rpca.svt(M, -1.0), "tau"), (lambda: rpca.svt(np.ones(3), 1.0), "A"),
        (lambda: rpca.scaled_gram(M, np.ones(5)), "g"), (lambda: rpca.matmul(M, np.ones((5, 3))), "A"),
        (lambda: rpca.masks(M, np.ones((4, 5))), "S"), (lambda: rpca.masks(M, M, kind="hard"), "kind"), (lambda: rpca.masks(M, M, gain_mask=-1), "gain_mask"),
        (lambda: rpca.masks(M, M, power=0), "power"), (lambda: rpca.masks(M, M, margin=0.5), "margin"),
        (lambda: rpca.rpca(M, mask=1), "mask"), (lambda: rpca.rpca(M, kind=None), "kind"), (lambda: rpca.rpca(np.ones((2, 2, 2, 2))), "S"),
        (lambda: rpca.rpca_audio(np.zeros(4000, np.float32), n_iter=-3), "n_iter"), (lambda: rpca.rpca_audio(np.zeros(4000, np.float32), residual=2), "residual"),
        (lambda: rpca.separate_wav_rpca("/nonexistent.wav", out_rate="native"), "out_rate"),
        (lambda: rpca.separate_wav_rpca("/nonexistent.wav", kernel_size=5), "kernel_size"), (lambda: rpca.separate_wav_rpca("/nonexistent.wav", gain=-1), "gain"),
    ]
    for n, (call, word) in enumerate(bad):
        with pytest.raises(ValueError, match=word):
            call()
            pytest.fail("case %d was accepted" % n)


def _ctype(arg):
    if "*" in arg:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}[arg.split()[0]]


def test_the_entries_are_declared_exported_and_bound_with_the_headers_signatures(lib):
    text = open(os.path.join(REPO, "include", "glowk.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NAMES:
        m = re.search(r"\b(int|size_t) %s\(([^;]*)\);" % name, code)
        assert m, name
        res = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)]
        args = [_ctype(" ".join(a.split())) for a in m.group(2).split(",")]
        assert _lib.SYMBOLS[name] == (res, args), name
        assert getattr(lib, name) is not None
    bound = sorted(n for n in _lib.SYMBOLS if n.startswith("glowk_rpca"))
    assert bound == sorted(NAMES) and sorted(set(re.findall(r"\bglowk_rpca\w*(?=\()", code))) == bound
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 554 and "Since version 554" in text


def test_the_workspaces(lib):
    r8 = lambda n: -(-n // 8) * 8
    for nsig, rows, frames in [(1, 1, 1), (2, 16, 12), (3, 33, 80), (1, 130, 67), (1, 65, 1025), (1, 1025, 5626)]:
        parts = min(8, -(-frames // 1024))
        gemm = 0 if parts == 1 else 8 * nsig * parts * rows * rows
        assert lib.glowk_rpca_gemm_workspace_bytes(nsig, rows, rows, frames, 0) == gemm
        assert lib.glowk_rpca_gemm_workspace_bytes(nsig, rows, rows, frames, 1) == 0 and lib.glowk_rpca_gemm_workspace_bytes(nsig, rows, frames, rows, 2) == 0
        eig = 16 * nsig * -(-rows // 2) + 8 * nsig + r8(120 * nsig)
        assert lib.glowk_rpca_eigh_workspace_bytes(nsig, rows) == eig
        svt = 3 * 8 * nsig * rows * rows + 2 * 8 * nsig * rows + 2 * r8(4 * nsig) + gemm + eig
        assert lib.glowk_rpca_svt_workspace_bytes(nsig, rows, frames) == svt
        groups = min(256, -(-rows * frames // 1024))
        fit = 2 * 8 * nsig * rows * frames + 64 * nsig + 8 * nsig + 16 * nsig * groups + r8(4 * nsig * groups) + r8(4 * nsig) + svt
        assert lib.glowk_rpca_workspace_bytes(nsig, rows, frames) == fit
    for fn in (lib.glowk_rpca_svt_workspace_bytes, lib.glowk_rpca_workspace_bytes):
        for args in [(0, 4, 4), (-1, 4, 4), (65536, 1, 1), (1, 0, 4), (1, 2050, 4), (1, 4, 0), (1, 4, 65536), (16, 2049, 65535), (512, 2049, 1)]:
            assert fn(*args) == 0, args
    for args in [(0, 4), (1, 0), (1, 2050), (512, 2049), (65536, 1)]:
        assert lib.glowk_rpca_eigh_workspace_bytes(*args) == 0, args
    for args in [(1, 4, 5, 4000, 0), (1, 4, 4, 4000, 3), (0, 4, 4, 4000, 0), (1, 2050, 2050, 4000, 0), (1, 4, 4, 65536, 0)]:
        assert lib.glowk_rpca_gemm_workspace_bytes(*args) == 0, args


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z = ctypes.c_void_p(0)
    a, b, c, d, e, f = (ctypes.c_void_p(v << 28) for v in range(1, 7))                    # never dereferenced, far apart
    odd = ctypes.c_void_p((11 << 28) + 4)
    err = lambda: lib.glowk_last_error().decode()
    big = 1 << 40

    def gemm(x=a, y=b, sc=c, nsig=1, M=4, N=4, K=9, form=0, out=d, work=e, nbytes=big):
        return lib.glowk_rpca_gemm(x, y, sc, nsig, M, N, K, form, out, work, nbytes, z)

    def eig(g=a, nsig=1, n=4, l=b, v=c, sweeps=d, status=e, work=f, nbytes=big):
        return lib.glowk_rpca_eigh(g, nsig, n, l, v, sweeps, status, work, nbytes, z)

    def svt(x=a, nsig=1, rows=4, frames=9, tau=b, out=c, sweeps=d, status=e, work=f, nbytes=big):
        return lib.glowk_rpca_svt(x, nsig, rows, frames, tau, out, sweeps, status, work, nbytes, z)

    def fit(m=a, nsig=1, rows=4, frames=9, gain=1.0, tol=1e-7, n_iter=3, L=b, S=c, iters=d, status=e, work=f, nbytes=big):
        return lib.glowk_rpca_fit(m, nsig, rows, frames, gain, tol, n_iter, L, S, iters, status, work, nbytes, z)

    shape = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=2050), "rows"), (dict(frames=0), "frames"),
             (dict(frames=65536), "frames"), (dict(nsig=16, rows=2049, frames=65535), "2^31"), (dict(nsig=512, rows=2049, frames=1), "2^31")]
    last = [(dict(), "device memory")]
    for call, cases in (
            (gemm, [(dict(nsig=-1), "nsig"), (dict(M=0), "M must"), (dict(M=2050), "M must"), (dict(K=0), "K must"), (dict(N=65536, form=2), "N and K"),
                    (dict(form=3), "form"), (dict(N=5), "N == M"), (dict(form=1, N=5), "N == M"), (dict(nsig=65535, M=2049, N=2049, K=1), "2^31"),
                    (dict(x=z), "null"), (dict(form=2, y=z), "null"), (dict(form=1, sc=z), "null"), (dict(K=2000, nbytes=8), "work_bytes"),
                    (dict(K=2000, work=z), "null"), (dict(out=odd), "aligned"), (dict(out=a), "overlap"), (dict(form=2, y=d), "overlap")] + last),
            (eig, [(dict(nsig=-1), "nsig"), (dict(n=0), "n must"), (dict(n=2050), "n must"), (dict(nsig=512, n=2049), "2^31"), (dict(l=z), "null"),
                   (dict(nbytes=8), "work_bytes"), (dict(v=odd), "aligned"), (dict(v=a), "overlap"), (dict(work=b), "overlap")] + last),
            (svt, shape + [(dict(tau=z), "null"), (dict(nbytes=64), "work_bytes"), (dict(tau=odd), "aligned"), (dict(out=a), "overlap")] + last),
            (fit, shape + [(dict(gain=0.0), "gain"), (dict(gain=float("inf")), "gain"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"),
                           (dict(n_iter=-1), "n_iter"), (dict(n_iter=100001), "n_iter"), (dict(S=z), "null"), (dict(nbytes=64), "work_bytes"),
                           (dict(L=odd), "aligned"), (dict(S=b), "overlap"), (dict(work=a), "overlap")] + last)):
        for kw, word in cases:
            assert call(**kw) == _lib.ERR and word in err(), (call.__name__, kw, err())
        assert call(nsig=0) == _lib.OK
    shr = lambda t=a, n=8, thr=0.5, out=b: lib.glowk_rpca_shrink(t, n, thr, out, z)
    msk = lambda l=a, s=b, x=c, n=8, g=1.0, m=d, bg=e, fg=f: lib.glowk_rpca_binary_mask(l, s, x, n, g, m, bg, fg, z)
    for call, cases in ((shr, [(dict(n=1 << 31), "count"), (dict(thr=-1.0), "thr"), (dict(thr=float("nan")), "thr"), (dict(t=z), "null"), (dict(out=odd), "aligned"),
                               (dict(out=ctypes.c_void_p((1 << 28) + 8)), "overlap")] + last),
                        (msk, [(dict(n=1 << 31), "count"), (dict(g=-1.0), "gain_mask"), (dict(s=z), "null"), (dict(bg=z), "null"), (dict(l=odd), "aligned"),
                               (dict(m=a), "overlap"), (dict(fg=c), "overlap")] + last)):
        for kw, word in cases:
            assert call(**kw) == _lib.ERR and word in err(), (call.__name__, kw, err())
        assert call(n=0) == _lib.OK
    host = torch.ones(8, dtype=torch.float64)                                            # a host pointer is refused, not dereferenced
    assert shr(t=ctypes.c_void_p(host.data_ptr())) == _lib.ERR and "device memory" in err()


def test_the_index_rules_under_address_and_ub_sanitizers(tmp_path):
    """glowk_rpca_index.h -- the round-robin pairs, the GEMM's tiles and K split, the chunks of the sums, the workspace plans -- compiled
    without HIP into a stand-alone program with its own main (tests/rpca_index_sanitize_main.cpp) and swept against straightforward
    loops."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "rpca_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "rpca_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "RPCA_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
