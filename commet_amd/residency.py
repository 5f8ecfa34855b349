"""Which sets are on the device when: the plan of an N x N matrix whose sets together exceed a byte budget (matrix.py, --set-budget-gb).

The reference runs one job at a time from disk, so its N is unbounded (Commet.py:186-240, file_manager.h:117-171); the resident driver
needs the sets of a job on the device.  plan() orders the pair chains of the matrix so that few sets are resident at a time:

    a BLOCK of consecutive reference sets stays loaded; the pairs inside the block run; then every later set is streamed past the
    block — loaded, J1 / J2 / J3 of (ref, it) for every ref of the block, evicted.  The next block starts behind the last
    reference set of this one.

J1 of a reference set is thereby split over groups of targets.  A search set's tags depend on the index set and that search set only
(index_and_search.cpp:241-277 keeps one tag vector per search set), so a split J1 gives the same bits; its price is one more index build
of S_ref per group.  J3(ref, i) needs J1(ref, i) and J2(ref, i) only, so a pair's chain completes while its two sets are loaded.

Steps, in order:   ("load", s)   ("evict", s)   ("j1", ref, [targets])   ("pair", ref, i)  = J2(ref, i) then J3(ref, i)

Loads: a block of b sets that streams the m sets behind it costs b + m loads.  With N sets of one size, capacity C = budget // size
and b = C - 1 (one slot for the streamed set) block k loads N - k b sets: sum_{k < ceil((N-1)/b)} (N - k b) in all, N when C >= N.
The targets are streamed last set first and the last one streamed — the set right behind the block — stays for the next block, whose
first reference set it is: one load less per block than that sum.

Pure Python: no GPU, no torch."""


def plan(sizes, budget_bytes):
    """sizes[s]: bytes set s holds when loaded; budget_bytes: the most the loaded sets may hold together.
    -> the list of steps.  Raises ValueError, before anything is planned, when the two largest sets do not fit together."""
    n = len(sizes)
    sizes = [int(x) for x in sizes]
    budget = int(budget_bytes)
    if n >= 2:
        big = sorted(range(n), key=lambda s: (-sizes[s], s))[:2]
        if sizes[big[0]] + sizes[big[1]] > budget:
            raise ValueError(f"the set budget of {budget} bytes cannot hold the two largest sets together: set {big[0]} ({sizes[big[0]]} bytes) "
                             f"and set {big[1]} ({sizes[big[1]]} bytes); every pair of sets has to be loaded at the same time once")
    elif n == 1 and sizes[0] > budget:
        raise ValueError(f"the set budget of {budget} bytes cannot hold set 0 ({sizes[0]} bytes)")
    steps, loaded, used = [], [], 0

    def load(s):
        nonlocal used
        if s not in loaded:
            steps.append(("load", s))
            loaded.append(s)
            used += sizes[s]
            assert used <= budget

    def evict(s):
        nonlocal used
        steps.append(("evict", s))
        loaded.remove(s)
        used -= sizes[s]

    if n == 1:
        load(0)
    a = 0
    while a < n - 1:
        # the block [a, e): as many reference sets as leave room for the largest set that will be streamed past them
        e, held = a + 1, sizes[a]
        while e < n and held + sizes[e] + (max(sizes[e + 1:]) if e + 1 < n else 0) <= budget:
            held += sizes[e]
            e += 1
        for s in list(loaded):                                    # (what the block before left: its members, never needed again)
            if not a <= s < e:
                evict(s)
        for s in range(a, e):
            load(s)
        for ref in range(a, e - 1):                               # the pairs inside the block
            steps.append(("j1", ref, list(range(ref + 1, e))))
            for i in range(ref + 1, e):
                steps.append(("pair", ref, i))
        for i in range(n - 1, e - 1, -1):                         # every later set past the block, last set first
            load(i)
            for ref in range(a, e):
                steps.append(("j1", ref, [i]))
            for ref in range(a, e):
                steps.append(("pair", ref, i))
            if i != e:                                            # (set e stays: the first reference set of the next block)
                evict(i)
        a = e
    return steps


def equal_size_load_bound(n, capacity):
    """most loads the plan may take for n sets of one size of which `capacity` (>= 2) fit the budget: the block scheme with
    b = capacity - 1 reference sets per block and nothing kept between blocks"""
    if capacity >= n:
        return n
    b = capacity - 1
    return sum(n - k * b for k in range(-(-(n - 1) // b)))


def check(steps, sizes, budget_bytes):
    """Replays a plan: every pair once, J1 before its pair, every job's sets loaded, never above the budget (raises AssertionError).
    -> dict(loads, evicts, peak_bytes, j1_steps)"""
    n = len(sizes)
    loaded, used, peak, loads, evicts, j1s = set(), 0, 0, 0, 0, 0
    j1_done, pairs = set(), []
    for st in steps:
        if st[0] == "load":
            assert st[1] not in loaded, st
            loaded.add(st[1])
            used += sizes[st[1]]
            loads += 1
            peak = max(peak, used)
            assert used <= budget_bytes, (st, used, budget_bytes)
        elif st[0] == "evict":
            assert st[1] in loaded, st
            loaded.remove(st[1])
            used -= sizes[st[1]]
            evicts += 1
        elif st[0] == "j1":
            _, ref, targets = st
            assert targets and ref in loaded and all(i in loaded and i > ref for i in targets), st
            j1_done.update((ref, i) for i in targets)
            j1s += 1
        elif st[0] == "pair":
            _, ref, i = st
            assert ref < i and ref in loaded and i in loaded and (ref, i) in j1_done, st
            pairs.append((ref, i))
        else:
            raise AssertionError(f"unknown step {st!r}")
    assert sorted(pairs) == [(r, i) for r in range(n - 1) for i in range(r + 1, n)] and len(set(pairs)) == len(pairs)
    return dict(loads=loads, evicts=evicts, peak_bytes=peak, j1_steps=j1s)
