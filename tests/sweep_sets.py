"""The four synthetic sets of the matrix driver's tests, as files: shared by the threshold sweep's CPU and GPU tests.  TEST INFRASTRUCTURE ONLY."""
import numpy as np


def four_sets(rng_seed=1):
    """the four synthetic sets of test_matrix_driver_matches_oracle_on_synthetic_sets, in the working directory -> (names, files, bvs)"""
    from commet_amd import synth
    import util
    n, L = 6000, 80
    names = ["s0", "s1", "s2", "s3"]
    files = [["s0.fa"], ["s1a.fa", "s1b.fa"], ["s2.fa"], ["s3.fa"]]
    for s, fl in enumerate(files):
        b, o = synth.synth_set(s, n, L, copy_frac=0.3)
        if len(fl) == 1:
            synth.write_fasta(fl[0], b, o)
        else:
            h = n // 2
            synth.write_fasta(fl[0], b[: h * L], o[: h + 1])
            synth.write_fasta(fl[1], b[h * L:], o[h:] - o[h])
    rng = np.random.default_rng(rng_seed)
    bvs = []
    for s, fl in enumerate(files):
        row = []
        for j, f in enumerate(fl):
            sel = rng.random(len(util.parse_fasta(f))) < 0.9
            if (s, j) == (1, 1):
                sel[:] = False                                   # a file with no selected read
            util.write_bv(f + ".bv", "filter of " + f, sel)
            row.append(f + ".bv")
        bvs.append(row)
    open("sets.txt", "w").write("".join(f"{names[s]}: " + "; ".join(f"{f},{b}" for f, b in zip(files[s], bvs[s])) + "\n" for s in range(4)))
    return names, files, bvs
