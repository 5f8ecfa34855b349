"""commet_amd/residency.py: the plan of an N x N matrix under a byte budget for its resident sets — replayed in a small simulator of
this file's own (not the module's check()), so that a mistake in the module cannot vouch for itself."""
import random

import pytest

from commet_amd import residency


def replay(steps, sizes, budget):
    """-> (loads, peak bytes); asserts: every pair (ref < i) exactly once, J1(ref, T) with i in T before pair (ref, i), the sets a job
    names loaded, the loaded bytes within the budget"""
    n = len(sizes)
    loaded, j1, pairs, loads, peak = set(), set(), [], 0, 0
    for st in steps:
        kind = st[0]
        if kind == "load":
            assert st[1] not in loaded, st
            loaded.add(st[1])
            loads += 1
        elif kind == "evict":
            assert st[1] in loaded, st
            loaded.discard(st[1])
        elif kind == "j1":
            ref, targets = st[1], st[2]
            assert len(targets) > 0 and {ref, *targets} <= loaded, st
            assert all(ref < i for i in targets), st
            j1 |= {(ref, i) for i in targets}
        else:
            assert kind == "pair", st
            ref, i = st[1], st[2]
            assert {ref, i} <= loaded and (ref, i) in j1, st
            pairs.append((ref, i))
        now = sum(sizes[s] for s in loaded)
        assert now <= budget, (st, now, budget)
        peak = max(peak, now)
    assert len(pairs) == len(set(pairs))
    assert sorted(pairs) == [(a, b) for a in range(n - 1) for b in range(a + 1, n)]
    return loads, peak


def test_random_plans_hold_the_four_conditions():
    rng = random.Random(20)
    for case in range(400):
        n = rng.randint(2, 16)
        sizes = [rng.choice((rng.randint(1, 1000), 500)) for _ in range(n)]
        two = sum(sorted(sizes)[-2:])
        budget = two + rng.choice((0, rng.randint(0, 50), rng.randint(0, sum(sizes))))
        steps = residency.plan(sizes, budget)
        loads, peak = replay(steps, sizes, budget)
        assert n <= loads and peak <= budget, (case, sizes, budget)
        if budget >= sum(sizes):
            assert loads == n


@pytest.mark.parametrize("n", [2, 3, 5, 12, 40])
def test_equal_sizes_stay_within_the_block_schemes_loads(n):
    size = 1000
    for cap in range(2, n + 1):
        b = cap - 1
        bound = sum(n - k * b for k in range(-(-(n - 1) // b)))
        for budget in (cap * size, cap * size + size - 1):
            loads, _ = replay(residency.plan([size] * n, budget), [size] * n, budget)
            assert n <= loads <= bound, (n, cap, loads, bound)
            if cap >= n:
                assert loads == n


def test_the_issues_example():
    b = 3
    assert sum(12 - k * b for k in range(-(-11 // b))) == 30
    loads, _ = replay(residency.plan([7] * 12, 4 * 7), [7] * 12, 28)
    assert 12 <= loads <= 30
    assert residency.equal_size_load_bound(12, 4) == 30 and residency.equal_size_load_bound(12, 12) == 12


def test_a_budget_below_the_two_largest_sets_is_refused_with_their_names():
    with pytest.raises(ValueError) as ei:
        residency.plan([5, 9, 3, 8], 16)
    assert "set 1" in str(ei.value) and "set 3" in str(ei.value) and "two largest" in str(ei.value)
    residency.plan([5, 9, 3, 8], 17)


def test_modules_own_check_agrees():
    sizes = [3, 1, 4, 1, 5, 9, 2, 6]
    steps = residency.plan(sizes, 15)
    got = residency.check(steps, sizes, 15)
    assert (got["loads"], got["peak_bytes"]) == replay(steps, sizes, 15)
