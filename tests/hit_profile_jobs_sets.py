"""The read sets of the many-job hit profile's tests (test_gpu_hit_profile_jobs.py on the GPU, test_hit_profile_jobs_cpu.py through the
CPU checker alone): generators only, importable without a GPU, every case seeded and cached so that both files see the same reads.

A FIXTURE is one commet_index_many_and_profile call: jobs (an index set and a cap each) that search one set, with the bytes the design
means the planted read to get.  The bytes a test compares with are never the design's: `checker_bytes` derives min(cap, count) per job
and read from the CPU checker, one run per job and t (a Bloom coincidence cannot make a fixture lie); the CPU file proves that the
checker's bytes ARE the design's for the planted reads.

k = 20, reads of 100 bases: a read holds at most five non-overlapping k-mers, so the checker at t = 1..5 gives every count exactly,
whatever the cap."""
import os

import numpy as np

import hit_profile_group_sets as gs
import oracle_binding as ob
import util

K = 20
L = 100
T_TOP = L // K                                  # no read of L bases has more non-overlapping k-mers


def checker_tags(d, k, t, index_reads, search, max_kmer=0, index_select=None):
    """-> (found bools of the one search set, chunks)"""
    d = str(d)
    os.makedirs(d, exist_ok=True)
    util.write_fasta(os.path.join(d, "I.fa"), index_reads)
    if index_select is not None:
        util.write_bv(os.path.join(d, "I.fa.bv"), "filter of I.fa", index_select)
    open(os.path.join(d, "i.txt"), "w").write("I:I.fa" + (",I.fa.bv" if index_select is not None else "") + "\n")
    util.write_fasta(os.path.join(d, "Q.fa"), search)
    open(os.path.join(d, "s.txt"), "w").write("Q:Q.fa\n")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        rc, res, chunks, kmers = ob.index_and_search("i.txt", "s.txt", f"out{t}", f"log{t}", k, t, max_kmer=max_kmer)
    finally:
        os.chdir(cwd)
    assert rc == 0
    _, n, bits = util.read_bv(os.path.join(d, f"out{t}", "Q.fa_in_I.bv"))
    assert n == len(search)
    return util.bools_from_bits(bits, n), chunks


def checker_counts(d, k, index, search, max_kmer, t_max, index_select=None):
    """min(t_max, hits) per read of the search set, from one checker run per t; -> (counts, chunks)"""
    counts = np.zeros(len(search), dtype=np.uint8)
    chunks = 0
    for t in range(1, t_max + 1):
        tags, chunks = checker_tags(d, k, t, index, search, max_kmer=max_kmer, index_select=index_select)
        assert not (tags & (counts < t - 1)).any()            # found at t: found at t - 1
        counts[tags] = t
    return counts, chunks


def plant(piece, strand):
    return piece if strand == 0 else util.revcomp(piece)


def edge_reads(rng, r):
    """(e) behind the planted read r: r with an N inside a planted window of every fixture (base 45), with a run of Ns, in lower case,
    reads shorter than k, a random read, and 40 identical copies of r"""
    with_n = bytearray(r)
    with_n[45:46] = b"N"
    run_n = bytearray(r)
    run_n[8:13] = b"N" * 5
    return [bytes(with_n), bytes(run_n), r.lower(), r[:K - 1], r[50:50 + K - 5], b"A", gs.rand(rng, L), util.revcomp(r)] + [r] * 40


_FIXTURES = {}


def fixture(name, strand):
    """-> dict(jobs = [index reads], caps, search, max_kmer, chunks = [chunk filters per job], design = {job: byte of search[0]})"""
    key = (name, strand)
    if key in _FIXTURES:
        return _FIXTURES[key]
    rng = np.random.default_rng(2000 + 10 * ["stop", "crosstalk", "max"].index(name) + strand)
    r = gs.rand(rng, L)
    max_kmer = 0
    if name == "stop":
        # (a) job 0 reaches its cap of 1 at window 0; job 1's three hits lie behind it: a walk that ends when ANY job is done gives 0
        jobs = [[plant(r[0:30], strand)], [plant(r[40:100], strand)]]
        caps, chunks, design = [1, 3], [1, 1], {0: 1, 1: 3}
    elif name == "crosstalk":
        # (b) job 0: hits at 0, 20, 40; job 1: at 10, 30, 50.  A `free` shared between the slots lets job 1 take 30 and 50 only
        jobs = [[plant(r[0:60], strand)], [plant(r[10:70], strand)]]
        caps, chunks, design = [255, 255], [1, 1], {0: 3, 1: 3}
    else:
        # (c) ONE job of two chunks: two hits in the first chunk filter, three in the second: max 3, a sum over the job's slots gives 5.
        # A second job (another read's pieces, one chunk) makes the call share a pass
        other = gs.rand(rng, L)
        index, max_kmer = gs.chunked(rng, K, [[plant(r[0:40], strand)], [plant(r[40:100], strand)]])
        jobs = [index, [plant(other[0:25], strand)]]
        caps, chunks, design = [255, 255], [2, 1], {0: 3, 1: 0}
    f = dict(jobs=jobs, caps=caps, search=[r] + edge_reads(rng, r), max_kmer=max_kmer, chunks=chunks, design=design)
    assert all(len(x) <= L for x in f["search"])
    _FIXTURES[key] = f
    return f


FIXTURES = [(n, s) for n in ("stop", "crosstalk", "max") for s in (0, 1)]
_BYTES = {}


def checker_bytes(d, name, strand):
    """-> ([min(cap, count) per read of the search set] per job, [chunks per job]) from the checker; made once per fixture"""
    key = (name, strand)
    if key not in _BYTES:
        f = fixture(name, strand)
        out, chunks = [], []
        for j, (index, cap) in enumerate(zip(f["jobs"], f["caps"])):
            counts, c = checker_counts(os.path.join(str(d), f"{name}{strand}_j{j}"), K, index, f["search"], f["max_kmer"], T_TOP)
            out.append(np.minimum(counts, cap).astype(np.uint8))
            chunks.append(c)
        _BYTES[key] = (out, chunks)
    return _BYTES[key]


# ---- scenario cases: jobs made of scenarios.Scenario sets by selection ---------------------------------------------------------------
# A case is one call.  The scenario's LAST set is searched (it derives half of its reads from the sets before it) (its files ragged, with Ns, lower case, multi-line ...); every job indexes
# one of the other sets under a selection of its own — an even thinning that keeps the first read of every file (every file holds a
# selected read) and makes the wanted number of chunks under the case's one max_kmer; "all": no selection; "empty": no read selected.
# Several jobs therefore index the SAME set under different selections.  (chunks, cap) per job; select: the search set has a selection.
SCENARIO_CASES = {
    "k8_two":      dict(k=8, seed=3151, jobs=[(1, 1), (1, 255)], select=False),                                         # 2 slots
    "k8_mixed":    dict(k=8, seed=3132, jobs=[(3, 5), (9, 2), (2, 255), ("empty", 5), (3, 1), (8, 2), (1, 255), (1, 1)], select=True),   # 3 + 2 + 3 | 9 and the empty one alone | 8 alone in its pass | 1 + 1
    "k20_three":   dict(k=20, seed=3123, jobs=[(1, 2), (2, 5), (1, 255)], select=True),                                  # 4 slots
    "k20_eight":   dict(k=20, seed=3154, jobs=[(1, c) for c in (1, 2, 5, 255, 1, 2, 5, 255)], select=False),              # 8 slots, one pass
    "k20_all":     dict(k=20, seed=3115, jobs=[("all", 5), (2, 2), ("all", 1)], select=True),
    "k32_nine":    dict(k=32, seed=3106, jobs=[(1, c) for c in (1, 2, 5, 255, 1, 2, 5, 255, 3)], select=False),           # two passes: 8 + 1 (alone)
    "k32_two":     dict(k=32, seed=3117, jobs=[(1, 5), (1, 2)], select=True),
    "k33_two":     dict(k=33, seed=3128, jobs=[(1, 5), (1, 1)], select=False),                                          # wide keys: 2,
    "k33_four":    dict(k=33, seed=3139, jobs=[(1, 255), (2, 2), (1, 5)], select=True),                                  # 4
    "k33_eight":   dict(k=33, seed=3110, jobs=[(2, 1), (3, 255), (1, 2), (1, 5)], select=False),                          # and 7 of 8 slots
}


def passes_of(chunks, cap=8):
    """-> (shared passes, jobs that run alone) as commet_index_many_and_profile forms them; chunks: per job, 0 = the device planner does
    not take it"""
    passes, alone, cur, g = [], 0, 0, 0
    for c in chunks:
        if c == 0 or c > cap:
            alone += 1
            continue
        if g + c > cap:
            passes.append(cur)
            cur, g = 0, 0
        cur, g = cur + 1, g + c
    passes.append(cur)
    return sum(1 for p in passes if p >= 2), alone + sum(1 for p in passes if p == 1)


def _thinned(n, first_of_file, frac):
    sel = np.diff(np.floor(np.arange(n + 1) * frac)) > 0
    sel[list(first_of_file)] = True
    return sel


_CASES = {}


def scenario_case(name, d):
    """-> dict(k, scn, max_kmer, search = set name, search_sel = bools or None, jobs = [dict(source, sel = bools or None, cap, chunks)])"""
    if name in _CASES:
        return _CASES[name]
    import oracle_pool
    from scenarios import Scenario
    spec = SCENARIO_CASES[name]
    k = spec["k"]
    scn = Scenario(os.path.join(str(d), "scn_" + name), spec["seed"], k=k, n_scale=4.0, allow_bv=False)
    rng = np.random.default_rng(spec["seed"])
    sources = []
    names = sorted(scn.sets)
    for nme in names[:-1]:
        reads = [r for _, _, rs, _ in scn.sets[nme] for r in rs]
        firsts = np.cumsum([0] + [len(rs) for _, _, rs, _ in scn.sets[nme]])[:-1]
        bases, offs = util.to_batch(reads)
        sources.append((nme, len(reads), firsts, ob.kmer_counts(bases, offs, k).astype(np.int64)))
    most = max([c for c, _ in spec["jobs"] if isinstance(c, int)])
    max_kmer = max(2, min(int(kc.sum()) for _, _, _, kc in sources) // (most + 1))
    jobs = []
    for j, (want, cap) in enumerate(spec["jobs"]):
        nme, n, firsts, kc = sources[j % len(sources)]
        if want == "all":
            sel, chunks = None, len(oracle_pool.chunks_from_counts(kc, max_kmer))
        elif want == "empty":
            sel, chunks = np.zeros(n, dtype=bool), 0
        else:
            for frac in np.arange(0.01, 1.0001, 0.005):
                sel = _thinned(n, firsts, frac + 0.0013 * j)              # (jobs of equal size differ in their reads)
                chunks = len(oracle_pool.chunks_from_counts(kc[sel], max_kmer))
                if chunks == want and not sel.all():
                    break
            else:
                raise AssertionError(f"{name}: no thinning of {nme} makes {want} chunks at max_kmer {max_kmer}")
        jobs.append(dict(source=nme, sel=sel, cap=cap, chunks=chunks))
    n_q = sum(len(rs) for _, _, rs, _ in scn.sets[names[-1]])
    search_sel = (rng.random(n_q) < 0.7) if spec["select"] else None
    _CASES[name] = dict(k=k, scn=scn, max_kmer=max_kmer, search=names[-1], search_sel=search_sel, jobs=jobs)
    return _CASES[name]


def _write_cfg(scn, path, name, sel, prefix):
    parts, pos = [], 0
    for fa, _, reads, _ in scn.sets[name]:
        item = fa
        if sel is not None:
            bv = f"{prefix}_{os.path.basename(fa)}.bv"
            util.write_bv(os.path.join(scn.dir, bv), "selection of " + fa, sel[pos:pos + len(reads)])
            item += "," + bv
        pos += len(reads)
        parts.append(item)
    open(os.path.join(scn.dir, path), "w").write(name + ":" + ";".join(parts) + "\n")


_TRUTH = {}


def scenario_truth(name, d):
    """the checker on every job of the case, at every t <= min(cap, t_top): t_top = (longest read of the search set) // k — a read of
    fewer than t k bases holds no t non-overlapping k-mers, so beyond t_top the checker finds nothing by construction and the count is
    exact.  -> ([min(cap, count) per read of the search set] per job, [chunks per job])"""
    if name in _TRUTH:
        return _TRUTH[name]
    case = scenario_case(name, d)
    scn, k = case["scn"], case["k"]
    q_files = scn.sets[case["search"]]
    t_top = max(1, max(len(r) for _, _, rs, _ in q_files for r in rs) // k)
    _write_cfg(scn, "q.txt", case["search"], case["search_sel"], "q")
    out, chunks_of = [], []
    cwd = os.getcwd()
    os.chdir(scn.dir)
    try:
        for j, job in enumerate(case["jobs"]):
            _write_cfg(scn, f"j{j}.txt", job["source"], job["sel"], f"j{j}")
            n_q = sum(len(rs) for _, _, rs, _ in q_files)
            counts, chunks = np.zeros(n_q, dtype=np.uint8), 0
            for t in range(1, min(job["cap"], t_top) + 1):
                rc, res, chunks, kmers = ob.index_and_search(f"j{j}.txt", "q.txt", f"o{j}_{t}", f"l{j}_{t}", k, t, max_kmer=case["max_kmer"])
                assert rc == 0
                tags = []
                for fa, _, reads, _ in q_files:
                    _, n, bits = util.read_bv(os.path.join(f"o{j}_{t}", os.path.basename(fa) + "_in_" + job["source"] + ".bv"))
                    assert n == len(reads)
                    tags.append(util.bools_from_bits(bits, n))
                tags = np.concatenate(tags)
                assert not (tags & (counts < t - 1)).any()
                counts[tags] = t
            out.append(np.minimum(counts, job["cap"]).astype(np.uint8))
            chunks_of.append(chunks)
    finally:
        os.chdir(cwd)
    _TRUTH[name] = (out, chunks_of)
    return _TRUTH[name]
