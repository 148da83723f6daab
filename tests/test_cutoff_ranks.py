"""hostpath.cutoff_from_ranks -- the insert cutoff from the two order statistics the device's rank selection returns (uz_head_rank) -- against
hostpath.concordant_cutoff, the literal form of read_collector.py:11-25 over the whole column: equal as floats, bit for bit, and of one type."""
import numpy as np
import pytest

from unfazed_amd.hostpath import concordant_cutoff, cutoff_from_ranks, head_rank_index

LO, HI = -(1 << 31), (1 << 31) - 1


def _columns(n, rng):
    yield rng.integers(LO, HI + 1, n)              # the whole range of int32
    yield rng.integers(0, 4, n) * 150              # heavy ties
    yield rng.choice(np.array([LO, HI, 0]), n)     # the extremes


def _both(t, readlen, stdevs):
    n = t.size
    keys = np.sort(np.abs(t.astype(np.int64) - 2 * readlen))
    k = head_rank_index(n)
    assert 0 <= k <= n - 1
    got = cutoff_from_ranks(n, int(keys[k]), int(keys[min(k + 1, n - 1)]), readlen, stdevs)
    ref = concordant_cutoff(t.astype(np.int32), readlen, stdevs)
    return got, ref


def _same(got, ref):
    return type(got) is type(ref) and np.float64(got).tobytes() == np.float64(ref).tobytes()


def test_every_small_n_and_three_large_ones():
    rng = np.random.default_rng(20240611)
    cases = bad = 0
    for n in list(range(1, 1500)) + [200001, 999999, 1000001]:
        for t in _columns(n, rng):
            got, ref = _both(t, 150, 3)
            cases += 1
            bad += not _same(got, ref)
    assert cases == 4506 and bad == 0


@pytest.mark.parametrize("readlen", [0, 100, 150])
def test_edges_of_the_interpolation(readlen):
    # a == b; n - 1 a multiple of 200 (g at or next to 0: 0.995 (n - 1) is then a whole number in exact arithmetic); the extremes of int32
    for n in (1, 2, 201, 401, 601, 2001, 200, 202, 400, 402):
        for t in (np.full(n, 333), np.arange(n) * 1000 + 7, np.arange(n)[::-1] * (HI // max(n, 1)), np.full(n, LO), np.full(n, HI),
                  np.where(np.arange(n) % 2 == 0, LO, HI)):
            got, ref = _both(np.asarray(t, np.int64), readlen, 3)
            assert _same(got, ref), (n, readlen, got, ref)


def test_stdevs_only_decides_the_type():
    t = np.arange(1000) * 3
    for stdevs in (0, 3, 2.5):
        got, ref = _both(t, 150, stdevs)
        assert _same(got, ref) and isinstance(got, np.float64)


def test_an_empty_head_still_raises_in_the_host_form():
    with pytest.raises(IndexError):
        concordant_cutoff(np.zeros(0, np.int32), 150, 3)
