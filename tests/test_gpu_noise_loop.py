"""The acceptance loop of the libstdc++ noise path (afe_kernels.hip, three_accepted) keeps its bookkeeping in wave
masks: which lanes have one / two / three accepted candidates, who takes the rare exact branch, who leaves.  What that
can get wrong is per WAVE, not per lane -- a lane leaving early or late, a mask taken under a partial execution mask, the
exact branch deciding for the wrong lanes -- so the seeds here are chosen by what their wave looks like: waves that mix
ordinary seeds with seeds whose first three candidates include one the fp32 estimate cannot call, a wave of nothing but
those, a wave without any, short arrays (a partly filled last wave), and a wave whose lanes need from 3 up to 9 and more
iterations.  Every engine word after the six draws must be libstdc++'s, every normal the checker's to 4e-15 (the existing
known-answer test's bound), and the fp32 engine must stop at the same word.

The CPU tests hold the two arguments the post-loop evaluation leans on (afe_kernels.hip, canonical53): a candidate with a
coordinate word of 2147483646 is never a SURE accept, and libstdc++'s `ret >= 1.0` clamp cannot fire on a minstd_rand0
stream at all."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests.test_noise_decision_band import _canonical, _fp32_estimate

M = 2147483647            # minstd_rand0's modulus
A1, A2, A3, A4 = (pow(16807, k, M) for k in (1, 2, 3, 4))
SCAN = 4_000_000


def _mul(x, k):
    return (x * k) % M     # int64: x, k < 2^31


def _estimate(s):
    """the two high words of the candidate that starts at engine word s and its fp32 estimate, as the kernel forms it"""
    hx, hy = _mul(s, A2), _mul(s, A4)
    r2f = _fp32_estimate(hx, hy)
    sure = (r2f > np.float32(1e-5)) & (r2f < np.float32(1.0) - np.float32(1e-5))
    unsure = ~sure & (r2f <= np.float32(1.0) + np.float32(1e-5))
    return hx, hy, r2f, sure, unsure


def _exact_accept(s):
    x = 2.0 * _canonical(_mul(s, A1), _mul(s, A2)) - 1.0
    y = 2.0 * _canonical(_mul(s, A3), _mul(s, A4)) - 1.0
    r2 = x * x + y * y
    return ~((r2 > 1.0) | (r2 == 0.0))


def _scan():
    """per seed in 1 .. SCAN: which of the first three candidates is unsure (bit k), whether an unsure one is of the
    r2~ <= 1e-5 kind, and how many candidates the three accepted ones take (capped at 24)"""
    if not _scan.cache:
        s = np.arange(1, SCAN + 1, dtype=np.int64)
        unsure_at = np.zeros(SCAN, np.int8)
        small = np.zeros(SCAN, bool)
        top_word_sure = 0
        for k in range(3):
            hx, hy, r2f, sure, unsure = _estimate(s)
            unsure_at |= (unsure.astype(np.int8) << k)
            small |= unsure & (r2f <= np.float32(1e-5))
            top_word_sure += int((sure & ((hx == M - 1) | (hy == M - 1))).sum())
            s = hy
        # iterations of the loop for the first 2^18 seeds
        t = np.arange(1, (1 << 18) + 1, dtype=np.int64)
        got = np.zeros(t.size, np.int64)
        iters = np.zeros(t.size, np.int64)
        for _ in range(24):
            live = got < 3
            got += (_exact_accept(t) & live)
            iters += live
            t = np.where(live, _mul(t, A4), t)
        _scan.cache.append((unsure_at, small, top_word_sure, iters))
    return _scan.cache[0]


_scan.cache = []


def _reference(seeds):
    """libstdc++'s six normals and the engine word after them, by the checker"""
    from oracle import oracle_py
    L = oracle_py.lib()
    ref = np.empty((len(seeds), 6))
    state = np.empty(len(seeds), np.uint32)
    a, b = C.c_double(), C.c_double()
    for i, seed in enumerate(seeds):
        st = C.c_uint32(int(seed))
        for p in range(3):
            L.ora_normal_pair(C.byref(st), C.byref(a), C.byref(b))
            ref[i, 2 * p], ref[i, 2 * p + 1] = a.value, b.value
        state[i] = st.value
    return ref, state


def _check_on_device(seeds):
    import importlib
    afa = importlib.import_module("agri-fly_amd")
    seeds = np.asarray(seeds, np.uint32)
    ref, ref_state = _reference(seeds)
    with afa.Ensemble(8) as e:
        got, state = e.selftest_normals(seeds)
        got32, state32 = e.selftest_normals(seeds, dtype=np.float32)
    np.testing.assert_array_equal(state, ref_state)           # engine words bit-identical
    np.testing.assert_allclose(got, ref, rtol=4e-15, atol=0)
    np.testing.assert_array_equal(state32, state)             # the fp32 engine stops where the fp64 engine does
    assert np.isfinite(got32).all()


def _unsure_layout():
    unsure_at, _, _, _ = _scan()
    unsure = np.flatnonzero(unsure_at) + 1
    first = np.flatnonzero(unsure_at & 1) + 1                  # the FIRST candidate is the unsure one
    ordinary = np.flatnonzero(unsure_at[:4096] == 0) + 1
    assert first.size >= 64 and ordinary.size >= 1024
    rest = np.setdiff1d(unsure, first[:64])
    mixed = np.empty(2 * rest.size, np.int64)
    mixed[0::2], mixed[1::2] = rest, ordinary[64:64 + rest.size]      # every later wave holds both kinds
    return np.concatenate([first[:64], ordinary[:64], mixed]), unsure, ordinary


def test_scan_finds_the_unsure_seeds():
    unsure_at, small, _, iters = _scan()
    unsure = np.flatnonzero(unsure_at) + 1
    assert unsure.size == 279 and list(unsure[:3]) == [8862, 17923, 54772]
    assert int(small[unsure - 1].sum()) == 94
    assert iters.min() == 3 and iters.max() >= 9


def test_top_coordinate_word_is_never_a_sure_accept():
    """A coordinate word of 2147483646 has x~ == 1.0f in the loop's estimate ((float)2147483645 is 2^31, 2^31 * 2^-30 - 1 is 1),
    so r2~ >= 1: such a candidate is accepted, if at all, by the exact arithmetic only."""
    _, _, top_word_sure, _ = _scan()
    assert top_word_sure == 0
    m = M - 1
    h = np.array([1, 2, m // 2, m // 2 + 1, m - 1, m, m // 2 + 7, 3], np.int64)      # test_worst_case_words' corners
    hx, hy = (g.ravel() for g in np.meshgrid(h, h))
    r2f = _fp32_estimate(hx, hy)
    top = (hx == m) | (hy == m)
    assert top.sum() == 15 and (r2f[top] >= np.float32(1.0)).all()
    assert not (r2f[top] < np.float32(1.0) - np.float32(1e-5)).any()


def test_canonical_clamp_cannot_fire_on_this_engine():
    """generate_canonical's `ret >= 1.0` needs the HIGH word at 2147483646 and the low word within ~256 of the top; the high
    word is 16807 x the low word, which pins the low word of that one case at 739806647.  Exact rationals, then the doubles."""
    R = M - 1
    assert pow(A1, -1, M) == 1407677000 and (M - 1407677000) * A1 % M == M - 1
    lo = M - 1407677000
    assert lo == 739806647
    one_below = 1.0 - 2.0 ** -53
    # the largest value with a smaller high word, and the one case with the top high word
    assert Fraction(R - 1 + (R - 2) * R, R * R) < Fraction(one_below) - Fraction(1, 10 ** 10)
    assert Fraction(lo - 1 + (R - 1) * R, R * R) < Fraction(one_below) - Fraction(1, 10 ** 10)
    c = _canonical(np.array([R, lo], np.int64), np.array([R - 1, R], np.int64))
    assert (c < 1.0).all() and c.max() < 1.0 - 3e-10
    # and what it takes: low words the generator cannot pair with that high word
    assert _canonical(np.array([R], np.int64), np.array([R], np.int64))[0] >= 1.0


@pytest.mark.gpu
def test_waves_of_unsure_and_ordinary_seeds():
    seeds, _, _ = _unsure_layout()
    unsure_at, _, _, _ = _scan()
    kinds = (unsure_at[seeds - 1] != 0).reshape(-1)
    waves = [kinds[k:k + 64] for k in range(0, kinds.size, 64)]
    assert waves[0].all() and not waves[1].any() and all(w.any() and not w.all() for w in waves[2:])
    _check_on_device(seeds)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_partly_filled_last_wave(n):
    _, unsure, ordinary = _unsure_layout()
    seeds = np.empty(n, np.int64)
    seeds[0::2] = unsure[100:100 + seeds[0::2].size]
    seeds[1::2] = ordinary[200:200 + seeds[1::2].size]
    _check_on_device(seeds)


@pytest.mark.gpu
def test_one_wave_from_three_to_nine_and_more_iterations():
    _, _, _, iters = _scan()
    lanes = []
    for lane in range(64):
        want = 3 + lane % 8                                   # 3, 4, ..., 9, then anything from 10 up
        pool = np.flatnonzero(iters == want if want < 10 else iters >= 10)
        lanes.append(int(pool[lane // 8]) + 1)
    seeds = np.array(lanes, np.int64)
    assert iters[seeds - 1].min() == 3 and iters[seeds - 1].max() >= 10
    assert set(range(3, 10)) <= set(iters[seeds - 1].tolist())
    _check_on_device(seeds)


@pytest.mark.gpu
def test_streams_that_start_at_a_top_coordinate_word():
    """seeds found by stepping the generator backwards from a candidate whose x or y coordinate word is 2147483646, as the
    first, second or third candidate of the stream, among ordinary seeds"""
    inv = pow(A1, -1, M)
    seeds = []
    for back in (2, 4, 6, 8, 10, 12):                         # the top word is word 2, 4, ..., 12 of the stream
        seeds.append((M - 1) * pow(inv, back, M) % M)
    for s, back in zip(seeds, (2, 4, 6, 8, 10, 12)):
        assert s * pow(A1, back, M) % M == M - 1
    _, _, ordinary = _unsure_layout()
    mixed = np.empty(70, np.int64)
    mixed[:] = ordinary[300:370]
    mixed[5:65:10] = seeds
    _check_on_device(mixed)
