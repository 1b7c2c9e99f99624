"""Kernel additive modelling without a GPU: the restatement of tests/kam_ref.py against a brute-force sort per cell, the builders'
tables, the Python argument checks of ``audiosourcesep_amd.kam`` (ValueError before the library is loaded), the boundary of the C
entries, the host-side rules the kernel shares with the host under AddressSanitizer + UBSan in a stand-alone program, and the loop
with a horizontal and a vertical kernel against tests/hpss_ref.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, kam
from tests import hpss_ref
from tests import kam_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ("glowk_kam_median", "glowk_kam_backfit", "glowk_kam_work_bytes", "glowk_kam_fit")


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def planes(rows, F, seed):
    """Random values; a plane with runs of equal values; zeros; -0 and +0 mixed among a few values."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((rows, F)).astype(np.float32)
    b = np.round(rng.standard_normal((rows, F)) * 1.5).astype(np.float32)
    c = np.zeros((rows, F), np.float32)
    d = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], np.float32), (rows, F))
    return [a, b, c, d]


KERNELS = [R.harmonic(5), R.percussive(7), R.cross(3, 5), R.rectangle(3, 3), R.periodic(4, 3),
           np.array([[9, 0]], np.int32),                                     # never in range on these planes: the identity
           np.array([[2, 4], [-2, -4]], np.int32),                          # 0, 1 or 2 neighbours in range on a 6 x 9 plane
           np.array([[1, 1], [1, 1], [0, 0], [-1, 2]], np.int32),            # a duplicate, an even count
           np.array([[0, 1], [0, -1], [1, 0], [-1, 0]], np.int32)]           # no centre


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (6, 9), (9, 4)])
def test_the_restated_median_is_a_brute_force_sort_per_cell(shape):
    for S in planes(*shape, seed=shape[0] * 100 + shape[1]):
        for k in KERNELS:
            got, want = R.median(S, k), R.median_brute(S, k)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    S = planes(6, 9, 1)[0]
    vals, ok = R.gather(S, KERNELS[6])
    assert sorted(set(ok.sum(0).reshape(-1).tolist())) == [0, 1, 2]
    np.testing.assert_array_equal(R.median(S, KERNELS[5]), S)
    both = np.array([[0.0, -0.0, 5.0]], np.float32)                           # -0 and +0 compare equal: the first in table order
    assert np.signbit(R.median(both, np.array([[0, 1], [0, 0], [0, 2]], np.int32))[0, 0])
    assert not np.signbit(R.median(both, np.array([[0, 0], [0, 1], [0, 2]], np.int32))[0, 0])


def test_the_builders_tables():
    for mine, theirs in ((kam.harmonic(31), R.harmonic(31)), (kam.percussive(5), R.percussive(5)), (kam.periodic(24, 8), R.periodic(24, 8)),
                         (kam.cross(9, 7), R.cross(9, 7)), (kam.rectangle(3, 5), R.rectangle(3, 5)), (kam.harmonic(1), [(0, 0)]),
                         (kam.periodic(7, 0), [(0, 0)])):
        assert mine.dtype == np.int32 and mine.ndim == 2 and mine.flags.c_contiguous
        np.testing.assert_array_equal(mine, np.asarray(theirs))
    assert kam.harmonic(5).tolist() == [[0, -2], [0, -1], [0, 0], [0, 1], [0, 2]]
    assert kam.percussive(3).tolist() == [[-1, 0], [0, 0], [1, 0]]
    assert kam.periodic(10, 2).tolist() == [[0, -20], [0, -10], [0, 0], [0, 10], [0, 20]]
    c = kam.cross(9, 9)
    assert len(c) == 17 and len({tuple(p) for p in c.tolist()}) == 17 and (c == 0).all(1).sum() == 1
    assert len(kam.rectangle(9, 13)) == 117 and len(kam.cross(63, 65)) == 127 and len(kam.periodic(1, 63)) == 127
    k = kam.check_kernel([[4095, -32767], [0, 0], [0, 0]])
    assert k.dtype == np.int32 and k.tolist() == [[4095, -32767], [0, 0], [0, 0]]


def test_bad_arguments_raise_before_the_library_is_loaded(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    S = np.ones((3, 4), np.float32)
    A3 = np.ones((2, 3, 4), np.float32)
    h, p = kam.harmonic(3), kam.percussive(3)
    idx = torch.zeros((4, 2), dtype=torch.int32)
    y = np.zeros(4000, np.float32)
    bad = [
        lambda: kam.harmonic(0), lambda: kam.harmonic(4), lambda: kam.harmonic(129), lambda: kam.harmonic(3.0), lambda: kam.percussive(True), lambda: kam.percussive(-3),
        lambda: kam.periodic(0, 2), lambda: kam.periodic(5, 64), lambda: kam.periodic(5, -1), lambda: kam.periodic(1000, 33), lambda: kam.periodic(2.5, 2),
        lambda: kam.cross(2, 3), lambda: kam.cross(65, 65), lambda: kam.rectangle(3, 4), lambda: kam.rectangle(11, 13),
        lambda: kam.check_kernel([]), lambda: kam.check_kernel([[0, 0, 0]]), lambda: kam.check_kernel([0, 1]), lambda: kam.check_kernel([[0.0, 1.0]]),
        lambda: kam.check_kernel([[4096, 0]]), lambda: kam.check_kernel([[0, -32768]]), lambda: kam.check_kernel(np.zeros((128, 2), np.int32)),
        lambda: kam.check_kernel(torch.zeros((3, 2), dtype=torch.int32)), lambda: kam.check_kernel([[True, False]]), lambda: kam.check_kernel("cross"),
        lambda: kam.median(S, [[0, 0, 0]]), lambda: kam.median(S[0], h), lambda: kam.median(S.astype(np.complex64), h), lambda: kam.median(np.ones((3, 0), np.float32), h),
        lambda: kam.median(np.ones((1, 2, 3, 4), np.float32), h),
        lambda: kam.backfit(S, A3, power=0.0), lambda: kam.backfit(S, A3, power=float("inf")), lambda: kam.backfit(S, A3, power="2"), lambda: kam.backfit(S, A3, return_masks=1),
        lambda: kam.backfit(S, S), lambda: kam.backfit(S, np.ones((9, 3, 4), np.float32)), lambda: kam.backfit(S, np.ones((2, 3, 5), np.float32)),
        lambda: kam.backfit(A3, A3), lambda: kam.backfit(S, A3.astype(np.complex64)), lambda: kam.backfit(S.astype(np.complex64), A3),
        lambda: kam.fit(S, ()), lambda: kam.fit(S, h), lambda: kam.fit(S, [h] * 9), lambda: kam.fit(S, (h, p), n_iter=0), lambda: kam.fit(S, (h, p), n_iter=101),
        lambda: kam.fit(S, (h, p), n_iter=2.0), lambda: kam.fit(S, (h, p), power=-1.0), lambda: kam.fit(S, (h, p), power=float("nan")), lambda: kam.fit(S, (h, p), return_masks="yes"),
        lambda: kam.fit(S, (h, [[0, 0, 1]])), lambda: kam.fit(S, (h, idx.long())), lambda: kam.fit(S, (h, idx[:3])), lambda: kam.fit(A3, (h, idx)),
        lambda: kam.fit(S, (h, torch.zeros((4, 513), dtype=torch.int32))), lambda: kam.fit(S.astype(np.complex64), (h, p)), lambda: kam.fit(S, (h, "harmonic")),
        lambda: kam.kam(S, (h, p), mask=1), lambda: kam.kam(S, None), lambda: kam.kam(S[0], (h, p)), lambda: kam.kam(S, (h, p), n_iter=True),
        lambda: kam.kam_audio(y[:100]), lambda: kam.kam_audio(y, sources=()), lambda: kam.kam_audio(y, sources="harmonic"), lambda: kam.kam_audio(y, sources=("vocal",)),
        lambda: kam.kam_audio(y, sources=("harmonic",) * 9), lambda: kam.kam_audio(y, kernel_size=30), lambda: kam.kam_audio(y, n_iter=0), lambda: kam.kam_audio(y, power=0),
        lambda: kam.kam_audio(y, sources=("harmonic", [[0, 0, 0]])), lambda: kam.kam_audio(y, sources=("harmonic", idx)), lambda: kam.kam_audio(y, period_sec=(2.0, 1.0)),
        lambda: kam.kam_audio(y, k=0), lambda: kam.kam_audio(y, width_sec=-1.0), lambda: kam.kam_audio(y, sources=("harmonic", "repeating")),
        lambda: kam.kam_audio(y.astype(np.complex64)),
        lambda: kam.separate_wav_kam("nowhere.wav", out_rate="native"), lambda: kam.separate_wav_kam("nowhere.wav", out_rate=3.5), lambda: kam.separate_wav_kam("nowhere.wav", mono=1),
        lambda: kam.separate_wav_kam("nowhere.wav", kernel_size=4), lambda: kam.separate_wav_kam("nowhere.wav", residual=True), lambda: kam.separate_wav_kam("nowhere.wav", sources=("drums",)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d raised nothing" % i)


def _ctype(decl):
    if "*" in decl:
        return ctypes.c_void_p
    base = decl.rsplit(" ", 1)[0]
    return {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}[base]


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
    bound = sorted(n for n in _lib.SYMBOLS if n.startswith("glowk_kam"))
    assert bound == sorted(NAMES) and sorted(set(re.findall(r"\bglowk_kam\w*(?=\()", code))) == bound
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 557 and "Since version 557" in text


def i32(*v):
    return np.array(v, dtype=np.int32)


def hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_the_workspace(lib):
    for nsig, rows, frames, J in [(1, 1, 1, 1), (1, 3, 5, 3), (3, 17, 45, 2), (1, 33, 65, 8), (1, 1025, 5626, 3)]:
        for ks in (np.zeros(J, np.int32), np.array([7] + [0] * (J - 1), np.int32), np.full(J, 512, np.int32)):
            want = R.work_bytes(nsig, rows, frames, J, bool(ks.any()))
            got = lib.glowk_kam_work_bytes(nsig, rows, frames, J, hp(ks))
            assert got == want and got % 8 == 0, (nsig, rows, frames, J, ks)
            if ks.any():
                assert got == R.round8(4 * nsig * J * rows * frames) + lib.glowk_nn_workspace_bytes(1, rows, frames, int(ks.max()))
    one = i32(0)
    for args in [(0, 3, 7, 1), (-1, 3, 7, 1), (65536, 1, 1, 1), (1, 0, 7, 1), (1, 4097, 7, 1), (1, 3, 0, 1), (1, 3, 32769, 1), (1, 3, 7, 0), (1, 3, 7, 9), (16, 4096, 32768, 1)]:
        assert lib.glowk_kam_work_bytes(*args, hp(np.zeros(9, np.int32))) == 0, args
    assert lib.glowk_kam_work_bytes(1, 3, 7, 1, None) == 0 and lib.glowk_kam_work_bytes(1, 3, 7, 1, hp(i32(513))) == 0
    assert lib.glowk_kam_work_bytes(1, 3, 7, 1, hp(i32(-1))) == 0 and lib.glowk_kam_work_bytes(1, 3, 7, 1, hp(one)) == 88


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z = ctypes.c_void_p(0)
    p = [ctypes.c_void_p(v << 32) for v in range(1, 10)]                                  # never dereferenced, far apart
    err = lambda: lib.glowk_last_error().decode()
    big = 1 << 40
    tab = i32(0, -1, 0, 0, 0, 1)

    def med(s=p[0], nsig=1, rows=3, frames=7, off=tab, n=3, out=p[1]):
        return lib.glowk_kam_median(s, nsig, rows, frames, z if off is None else hp(off), n, out, z)

    def back(v=p[0], a=p[1], nsig=1, J=2, n=21, power=2.0, pp=p[2], mask=p[3]):
        return lib.glowk_kam_backfit(v, a, nsig, J, n, power, pp, mask, z)

    def fit(v=p[0], nsig=1, rows=3, frames=7, J=2, mn=i32(3, 0), off=tab, mk=i32(0, 2), idx=(None, p[4]), n_iter=2, power=2.0, pp=p[2], mask=p[3], work=p[5], nbytes=big):
        ptrs = None if idx is None else (ctypes.c_void_p * len(idx))(*[None if q is None else q.value for q in idx])
        return lib.glowk_kam_fit(v, nsig, rows, frames, J, z if mn is None else hp(mn), z if off is None else hp(off), z if mk is None else hp(mk),
                                 z if ptrs is None else ctypes.cast(ptrs, ctypes.c_void_p), n_iter, power, pp, mask, work, nbytes, z)

    plane = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(frames=0), "frames"),
             (dict(frames=32769), "frames"), (dict(nsig=65535, rows=4096, frames=32768), "2^31")]
    pw = [(dict(power=0.0), "power"), (dict(power=-1.0), "power"), (dict(power=float("nan")), "power"), (dict(power=float("inf")), "power")]
    last = [(dict(), "device memory")]
    cases = (
        (med, plane + [(dict(n=0), "n, the number"), (dict(n=128), "n, the number"), (dict(off=None), "table is null"), (dict(off=i32(4096, 0), n=1), "d_row"),
                       (dict(off=i32(0, 32768), n=1), "d_frame"), (dict(off=i32(0, 0, -4096, 0), n=2), "d_row"), (dict(s=z), "null"), (dict(out=z), "null"),
                       (dict(out=p[0]), "in place")] + last),
        (back, [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(J=0), "J must"), (dict(J=9), "J must"), (dict(n=1 << 31), "2^31"), (dict(nsig=2, n=1 << 30), "2^31")] + pw +
               [(dict(v=z), "null"), (dict(a=z), "null"), (dict(pp=z), "null"), (dict(pp=p[1]), "overlap"), (dict(mask=p[2]), "overlap"), (dict(mask=p[0]), "overlap")] + last),
        (fit, plane + pw + [(dict(J=0), "J must"), (dict(J=9), "J must"), (dict(n_iter=0), "n_iter"), (dict(n_iter=101), "n_iter"), (dict(mn=None), "model_n"), (dict(mk=None), "model_n"),
                            (dict(mn=i32(3, 1)), "exactly one"), (dict(mn=i32(0, 0), mk=i32(0, 2)), "exactly one"), (dict(mn=i32(128, 0)), "n, the number"),
                            (dict(off=None), "table is null"), (dict(off=i32(0, 0, 0, 0, 9999, 0)), "d_row"), (dict(mk=i32(0, 513)), "k must"), (dict(mk=i32(0, -1)), "k must"),
                            (dict(idx=None), "idx_dev"), (dict(idx=(None, None)), "tensor is null"), (dict(v=z), "null"), (dict(pp=z), "null"), (dict(work=z), "null"),
                            (dict(nbytes=8), "work_bytes"), (dict(pp=p[0]), "overlap"), (dict(mask=p[2]), "overlap"), (dict(work=p[2]), "overlap"), (dict(idx=(None, p[2])), "overlap")] + last))
    for call, rows in cases:
        for kw, word in rows:
            assert call(**kw) == _lib.ERR and word in err(), (call.__name__, kw, err())
        assert call(nsig=0) == _lib.OK
    assert back(n=0) == _lib.OK and back(mask=z) == _lib.ERR and "device memory" in err()
    host = torch.ones(4096, dtype=torch.float32)                                          # a host pointer is refused, not dereferenced
    assert med(s=ctypes.c_void_p(host.data_ptr())) == _lib.ERR and "device memory" in err()


def test_the_index_rules_under_address_and_ub_sanitizers(tmp_path):
    """glowk_kam_index.h -- the offset table, the waves and LDS of a workgroup, the units, the neighbour test, the workspace -- compiled
    without HIP into a stand-alone program with its own main (tests/kam_index_sanitize_main.cpp) and swept against straightforward
    loops.  The same program prints the launch geometry of the GPU tests' shapes, which tests/kam_ref.py restates."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "kam_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "kam_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "KAM_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    quads = [(1, 1, 1, 1), (1, 3, 5, 2), (2, 33, 65, 31), (1, 65, 130, 127), (3, 17, 64, 8), (1, 257, 97, 17), (1, 4096, 3, 5), (1, 2, 4500, 31),
             (1, 1025, 5626, 31), (1, 1025, 5626, 64), (1, 1025, 5626, 65), (15, 4096, 32768, 127)]
    r = subprocess.run([exe, "geometry"] + [str(v) for q in quads for v in q], capture_output=True, text=True, timeout=600, env=env)
    want = [[R.waves(n), R.lds_bytes(n), R.units(nsig, rows, frames), R.blocks(nsig, rows, frames, n)] for nsig, rows, frames, n in quads]
    assert r.returncode == 0 and [[int(v) for v in line.split()] for line in r.stdout.strip().splitlines()] == want
    assert [R.waves(n) for n in (1, 64, 65, 127)] == [4, 4, 1, 1] and R.lds_bytes(64) == 65536 and R.lds_bytes(127) == 32512


def test_a_horizontal_and_a_vertical_kernel_and_one_iteration_are_hpss():
    """``kam_ref.fit`` with (harmonic(31), percussive(31)), one iteration, power 2: at cells at least 15 from every edge -- where no
    neighbour is outside the plane, so skipping and reflecting agree -- the masks are those of tests/hpss_ref.py: the same fp64
    operations in the same order, so the bar is a few roundings of a value in [0, 1]."""
    rng = np.random.default_rng(31)
    S = (np.abs(rng.standard_normal((2, 47, 53))) ** 2).astype(np.float32)
    S[rng.random(S.shape) < 0.1] = 0.0
    P, masks = R.fit(S, (R.harmonic(31), R.percussive(31)), n_iter=1, power=2.0)
    mh, mp = hpss_ref.hpss(S, kernel_size=31, power=2.0, mask=True)
    inner = (slice(None), slice(15, 47 - 15), slice(15, 53 - 15))
    assert masks[:, 0][inner].size > 0
    assert np.abs(masks[:, 0][inner] - mh[inner]).max() <= 4 * 2.0 ** -53 and np.abs(masks[:, 1][inner] - mp[inner]).max() <= 4 * 2.0 ** -53
    assert np.abs(P.sum(1) - S).max() <= 8 * 2.0 ** -53 * S.max()                     # two quotients, two products, one sum
    # away from the interior the two differ: the kernel skips what HPSS reflects
    assert np.abs(masks[:, 0] - mh).max() > 1e-3
    for a, b in ((R.median(S, R.harmonic(31)), hpss_ref.median_filter(S, 31, 0)), (R.median(S, R.percussive(31)), hpss_ref.median_filter(S, 31, 1))):
        np.testing.assert_array_equal(a[inner], b[inner])
