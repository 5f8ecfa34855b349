"""commet_readset_offload / _restore: a finalized set leaves HBM for pageable host memory and comes back indistinguishable — the same
packed image, the same tags and stats from every job, the same filter bits; while it is away every entry point that would read it
fails with a message (ordinary error returns: nothing here provokes a fault), and the memory it held is the device's again."""
import threading

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

KINDS = ["fixed", "ragged", "two_files"]


def _make(ctx, rng, kind, n=20000):
    """-> (X: the set under test, Y, Z: sets related to it)"""
    import commet_amd
    lo, hi = (100, 100) if kind != "ragged" else (40, 180)
    base = util.random_reads(rng, n, lo, hi, n_rate=0.003)
    others = [util.related_reads(rng, base, n, lo, hi, share=0.4, n_rate=0.003) for _ in range(2)]
    if kind == "two_files":
        x = commet_amd.ReadSet.from_files(ctx, [util.to_batch(base[: n // 3]), util.to_batch(base[n // 3:])])
    else:
        x = commet_amd.ReadSet.from_files(ctx, [util.to_batch(base)])
    return [x] + [commet_amd.ReadSet.from_files(ctx, [util.to_batch(r)]) for r in others]


def _snapshot(ctx, x, y, z, tmp_path, tag):
    """everything the issue wants unchanged: the image's bytes, jobs with X as index and as search set, X's filter bits"""
    path = str(tmp_path / f"x_{tag}.pk")
    x.save(path)
    sel_bits, sel_stats = x.filter(min_len=60, max_n=1, min_shannon=1.9, max_reads=15000)
    jobs = []
    for idx, srch, isel, ssel in ((x, y, None, None), (y, x, None, None), (x, y, sel_bits, None), (y, x, None, sel_bits)):
        tags, st, _ = ctx.index_and_search(idx, [srch], isel, None if ssel is None else [ssel])
        jobs.append((tags[0].tobytes(), {f: st[0][f] for f in ("indexed", "searched", "shared")}))
    many_tags, many_st, _ = ctx.index_many_and_search([y, z], x, [None, None], None)
    jobs.append((many_tags[0].tobytes(), many_st[0]["shared"]))
    return dict(image=open(path, "rb").read(), filter=(sel_bits.tobytes(), sel_stats), jobs=jobs, kcnt=x.kmer_counts().tobytes())


def _refused(fn, text="read set is offloaded"):
    import commet_amd
    with pytest.raises(commet_amd.CommetError) as ei:
        fn()
    assert text in str(ei.value), str(ei.value)


@pytest.mark.parametrize("k", [32, 20])
@pytest.mark.parametrize("kind", KINDS)
def test_offload_then_restore_changes_nothing(tmp_path, kind, k):
    import commet_amd
    rng = np.random.default_rng(11 + KINDS.index(kind) + k)
    with commet_amd.Context(k=k, t=2) as ctx:
        x, y, z = _make(ctx, rng, kind)
        before = _snapshot(ctx, x, y, z, tmp_path, "before")
        ref_yz = ctx.index_and_search(y, [z])
        packed = x.packed_bytes
        assert x.resident and x.device_bytes == packed > 0
        _refused(x.restore, "already resident")
        x.offload()
        assert not x.resident and x.device_bytes == 0 and x.packed_bytes == packed and x.cache_bytes == 0
        assert x.num_reads == 20000 and x.num_files == (2 if kind == "two_files" else 1)       # host-side facts stay
        _refused(x.offload, "already offloaded")
        # every entry point that takes a read set: an error return with the message, the set and the context untouched
        _refused(lambda: ctx.index_reads(x))
        _refused(lambda: ctx.search_reads(x))
        _refused(lambda: ctx.index_and_search(x, [y]))
        _refused(lambda: ctx.index_and_search(y, [x]))
        _refused(lambda: ctx.index_and_search(y, [z, x]))
        _refused(lambda: ctx.index_many_and_search([y, z], x))
        _refused(lambda: ctx.index_many_and_search([y, x], z))
        _refused(lambda: x.filter(min_len=60))
        _refused(x.export)
        _refused(lambda: x.save(str(tmp_path / "no.pk")))
        _refused(x.kmer_counts)
        _refused(x.reserve_cache)
        assert not (tmp_path / "no.pk").exists()
        tags, st, _ = ctx.index_and_search(y, [z])                     # the context is as usable as before
        assert np.array_equal(tags[0], ref_yz[0][0]) and st[0]["shared"] == ref_yz[1][0]["shared"]
        x.restore()
        assert x.resident and x.device_bytes == packed == x.packed_bytes
        after = _snapshot(ctx, x, y, z, tmp_path, "after")
        assert after["image"] == before["image"]
        assert after["filter"] == before["filter"]
        assert after["jobs"] == before["jobs"]
        assert after["kcnt"] == before["kcnt"]
        x.offload()                                                    # a second round trip, and destroy in the offloaded state
        x.restore()
        assert _snapshot(ctx, x, y, z, tmp_path, "again")["jobs"] == before["jobs"]
        x.offload()
        x.close()
        tags, _, _ = ctx.index_and_search(y, [z])
        assert np.array_equal(tags[0], ref_yz[0][0])


def test_a_set_that_is_not_finalized_is_refused():
    import commet_amd
    with commet_amd.Context(k=32, t=2) as ctx:
        rs = commet_amd.ReadSet(ctx, 10, 1000)
        _refused(rs.offload, "not finalized")
        _refused(rs.restore, "not finalized")
        assert rs.resident


@pytest.mark.parametrize("kind", ["fixed", "ragged"])
def test_the_tiled_searchs_list_is_dropped_and_rebuilt(kind):
    import commet_amd
    rng = np.random.default_rng(5)
    with commet_amd.Context(k=32, t=2) as ctx:
        ctx.set_option("tiled_search", 2)
        x, y, _ = _make(ctx, rng, kind)
        ref = ctx.index_and_search(y, [x])
        assert x.cache_bytes > 0                                        # X took the tiled search: its query list is cached
        x.offload()
        assert x.cache_bytes == 0 and ctx.cache_stats()["bytes"] == y.cache_bytes
        x.restore()
        assert x.cache_bytes == 0
        tags, st, _ = ctx.index_and_search(y, [x])
        assert x.cache_bytes > 0                                        # ... rebuilt by the next scan that wants it
        assert np.array_equal(tags[0], ref[0][0]) and st[0]["shared"] == ref[1][0]["shared"]
        ctx.set_option("tiled_search", 1)                               # the gather kernels (a ragged set: its length-order list, rebuilt too)
        ctx.set_option("ordered_scan", 2)
        g0 = ctx.index_and_search(y, [x])
        x.offload()
        x.restore()
        g1 = ctx.index_and_search(y, [x])
        assert np.array_equal(g0[0][0], g1[0][0]) and np.array_equal(g0[0][0], ref[0][0])


def test_the_devices_memory_comes_back():
    """After the offload the set's blocks lie in the library's device cache, and after commet_device_cache_trim the device has at least
    packed_bytes more free memory, less one size class.
    Measured on this process alone: one offload / trim / restore round trip comes first, so that whatever the runtime sets up on the
    first chunked copy and the first pinned buffers exists before the first reading, the set's blocks are fresh ones of their exact size
    classes (a block handed out by the cache may be up to a quarter larger than asked), and the cache is empty.
    The slack: the library asks the driver for blocks in size classes (steps of 1/16 .. 1/32 of a block's size) and packed_bytes counts
    the set's blocks as asked for; blocks below 8 MiB (here the three bitmaps and the length words, 1.1 MB) go straight back to the
    driver, whose own granularity may keep part of them.  One class step of packed_bytes itself (8 MiB for this set) bounds that."""
    import commet_amd
    n, L = 3_000_000, 100
    rng = np.random.default_rng(2)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n * L, dtype=np.uint8)]
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    with commet_amd.Context(k=32, t=2) as ctx:
        dev = ctx.device

        def raw_free():                                             # hipMemGetInfo alone (device_memory counts the cache as free)
            return ctx.device_memory()[0] - commet_amd.device_cache_bytes(dev)

        x = commet_amd.ReadSet.from_files(ctx, [(bases, offs)])
        packed = x.packed_bytes
        step = 1 << (packed.bit_length() - 1 - 4)
        print(f"packed_bytes {packed}, class step {step}; at first: raw free {raw_free()}, cached {commet_amd.device_cache_bytes(dev)}")
        x.offload()                                                 # the round trip that comes first
        print(f"first offload: raw free {raw_free()}, cached {commet_amd.device_cache_bytes(dev)}")
        print(f"trim gave back {commet_amd.device_cache_trim(dev)}: raw free {raw_free()}")
        x.restore()
        assert commet_amd.device_cache_trim(dev) == 0 and commet_amd.device_cache_bytes(dev) == 0
        free_before = raw_free()
        x.offload()
        cached = commet_amd.device_cache_bytes(dev)
        free_cached = raw_free()
        trimmed = commet_amd.device_cache_trim(dev)
        free_after = raw_free()
        print(f"resident: raw free {free_before}; offloaded: cached {cached}, raw free {free_cached}; trim gave back {trimmed}: "
              f"raw free {free_after}, a rise of {free_after - free_before}")
        # the library's own accounting: the set's blocks of 8 MiB and more (all but 1.1 MB of this set) are in the cache, then nowhere
        assert packed - step <= cached <= packed
        assert trimmed == cached and commet_amd.device_cache_bytes(dev) == 0
        # ... and the device's
        assert free_after - free_before >= packed - step
        x.restore()
        assert x.device_bytes == packed
        fed = ctx.index_reads(x, 0, 1000)
        assert fed == 1000 * (L - 32 + 1)


def test_a_second_thread_moves_one_set_while_jobs_run_on_others(tmp_path):
    import commet_amd
    rng = np.random.default_rng(8)
    with commet_amd.Context(k=32, t=2) as ctx:
        x, y, z = _make(ctx, rng, "ragged")
        before = _snapshot(ctx, x, y, z, tmp_path, "before")
        ref = [ctx.index_and_search(y, [z]), ctx.index_and_search(z, [y])]
        errors, rounds = [], [0]
        go = threading.Event()

        def mover():
            try:
                go.wait()
                for _ in range(4):
                    x.offload()
                    assert not x.resident
                    x.restore()
                    rounds[0] += 1
            except BaseException as ex:        # handed to the main thread
                errors.append(ex)

        th = threading.Thread(target=mover)
        th.start()
        go.set()
        for it in range(12):
            a, b = (y, z) if it % 2 == 0 else (z, y)
            tags, st, _ = ctx.index_and_search(a, [b])
            assert np.array_equal(tags[0], ref[it % 2][0][0]) and st[0]["shared"] == ref[it % 2][1][0]["shared"]
        th.join()
        assert not errors, errors
        assert rounds[0] == 4 and x.resident
        after = _snapshot(ctx, x, y, z, tmp_path, "after")
        assert after == before


def test_a_set_in_a_running_job_is_not_offloaded():
    """The check and the release are one critical section with the jobs' entry.  Two jobs over 400 000-read sets in one call (milliseconds inside the library) is started on a second thread; the main thread waits until that thread is about to make the call, gives it a
    moment to get inside, and asks for the offload: refused, "part of a running job", nothing changed.  Should the offload win the race
    to the mutex (the job had not entered yet) the job is the one refused — an ordinary error as well — and the attempt is made again:
    within a few attempts the refusal of the OFFLOAD must be seen, and every job that ran gives the reference's bits."""
    import time
    import commet_amd
    rng = np.random.default_rng(4)
    with commet_amd.Context(k=32, t=2) as ctx:
        x, y, z = _make(ctx, rng, "fixed", n=400000)
        ref = ctx.index_many_and_search([x, z], y)
        refused = 0
        for attempt in range(8):
            about_to, result = threading.Event(), {}

            def job():
                about_to.set()
                try:
                    result["tags"] = ctx.index_many_and_search([x, z], y)[0]
                except commet_amd.CommetError as ex:
                    result["error"] = str(ex)

            th = threading.Thread(target=job)
            th.start()
            about_to.wait()
            time.sleep(0.0005)
            try:
                x.offload()
                moved = True
            except commet_amd.CommetError as ex:
                assert "part of a running job" in str(ex), str(ex)
                moved = False
                refused += 1
                assert x.resident and x.device_bytes == x.packed_bytes           # nothing changed
            th.join()
            if moved:
                x.restore()
            if "error" in result:
                assert moved and "read set is offloaded" in result["error"], result
            else:
                assert all(np.array_equal(a, b) for a, b in zip(result["tags"], ref[0]))
            if refused:
                break
        assert refused >= 1, "the offload was never refused while a job used the set"
        tags, _, _ = ctx.index_many_and_search([x, z], y)
        assert all(np.array_equal(a, b) for a, b in zip(tags, ref[0]))
