"""Search settings per side on the host (include/ataxxzero_hip.h, "Search settings per side"): azh_search_set_pairing, the
rule that names the sets of x and of o in game uid, against a restatement in Python — no device."""
import ctypes

import numpy as np
import pytest

from ataxxzero_amd import link

SIZES = [1, 2, 3, 5, 16]


def pairing(uid, n):
    """The rule as the header states it."""
    if n == 1:
        return 0, 0
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]     # lexicographic
    a, b = pairs[(uid // 2) % len(pairs)]
    return (a, b) if uid % 2 == 0 else (b, a)


@pytest.mark.parametrize("n", SIZES)
def test_pairing_equals_the_restatement(n):
    per = max(n * (n - 1), 1)
    uids = list(range(3 * per + 5)) + [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    for uid in uids:
        assert link.search_set_pairing(uid, n) == pairing(uid, n), (uid, n)


@pytest.mark.parametrize("n", SIZES[1:])
def test_every_window_holds_each_ordered_pair_once(n):
    per = n * (n - 1)
    wanted = sorted((a, b) for a in range(n) for b in range(n) if a != b)
    for first in (0, per, 7 * per):
        assert sorted(link.search_set_pairing(uid, n) for uid in range(first, first + per)) == wanted


@pytest.mark.parametrize("n", SIZES)
def test_a_uid_and_its_neighbour_swap_colours(n):
    for uid in range(0, 4 * max(n * (n - 1), 1), 1):
        x, o = link.search_set_pairing(uid, n)
        assert link.search_set_pairing(uid ^ 1, n) == (o, x)
        assert (x < o or n == 1) if uid % 2 == 0 else (x > o or n == 1)


def test_bad_arguments_come_back_as_negative_codes():
    dll = link.load()
    out = np.zeros(2, dtype=np.int32)
    for n in (0, -1, link.SEARCH_SETS_MAX + 1):
        assert dll.azh_search_set_pairing(0, n, ctypes.c_void_p(out.ctypes.data)) == -2
        with pytest.raises(link.AzhError, match="azh_search_set_pairing: need 1 <= n <= 16"):
            link.search_set_pairing(0, n)
    assert dll.azh_search_set_pairing(0, 2, None) == -1
    assert (out == 0).all()


def test_the_struct_is_the_headers():
    assert ctypes.sizeof(link.SearchSet) == 28
    assert [f for f, _ in link.SearchSet._fields_] == ["visits", "leaves", "virtual_loss", "c_puct", "fpu_reduction", "c_base",
                                                       "c_init"]
