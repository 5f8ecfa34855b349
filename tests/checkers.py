"""Checkers that several test files share.  TEST INFRASTRUCTURE ONLY.

key_level_search: the reference's search over the CPU checker's KEYS, for k whose filter no test host can allocate.
checker_job: one run of the restated tool (oracle_binding.index_and_search) over lists of reads, with everything its log line and
its .bv files say."""
import os

import every_k_sets as eks
import oracle_binding as ob
import util


def key_level_search(idx_reads, queries, k, t):
    """search_reads.h:45-83 over the CPU checker's KEYS (ok_keys_of_read: hash_key.h's add / rv_add per complete window) with the four
    lanes kept as Python sets — for k whose 2^(k-1)-byte filter the checker cannot allocate on a test host (k = 38: 128 GiB)"""
    # the one statement of the rule is every_k_sets.key_level_job: here every index read in ONE filter (no chunk fills, no read dropped)
    return eks.key_level_job(k, idx_reads, [queries], eks.ONE_CHUNK).tags(t)[0]


def checker_job(d, k, t, index_reads, search_sets, max_kmer=0):
    """-> (found bools per search set, [dict(indexed, searched, shared, probes)] per search set, chunks, k-mers indexed)"""
    d = str(d)
    os.makedirs(d, exist_ok=True)
    util.write_fasta(os.path.join(d, "I.fa"), index_reads)
    open(os.path.join(d, "i.txt"), "w").write("I:I.fa\n")
    for q, rs in enumerate(search_sets):
        util.write_fasta(os.path.join(d, f"Q{q:02d}.fa"), rs)
    open(os.path.join(d, "s.txt"), "w").write("".join(f"Q{q:02d}:Q{q:02d}.fa\n" for q in range(len(search_sets))))
    cwd = os.getcwd()
    os.chdir(d)
    try:
        rc, res, chunks, kmers = ob.index_and_search("i.txt", "s.txt", f"out{t}", f"log{t}", k, t, max_kmer=max_kmer)
    finally:
        os.chdir(cwd)
    assert rc == 0 and len(res) == len(search_sets)
    by_name = {r["name"]: r for r in res}
    tags, stats = [], []
    for q, rs in enumerate(search_sets):
        _, n, bits = util.read_bv(os.path.join(d, f"out{t}", f"Q{q:02d}.fa_in_I.bv"))
        assert n == len(rs)
        tags.append(util.bools_from_bits(bits, n))
        stats.append(by_name[f"Q{q:02d}"])
    return tags, stats, chunks, kmers
