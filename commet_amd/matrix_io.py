"""The files of the N x N driver (commet_amd.matrix), as Commet.py and its tools read and write them: the set file, .bv vectors,
the filter_reads command and its output, the three csv matrices, a job's .log.  No engine, no rank, no state."""
import os

import numpy as np


# ---- the set file, as Commet.py reads it (Commet.py:42-95) -------------------------------------
def parse_set_file(path):
    names, files, bvs = [], [], []
    with open(path) as fh:
        lines = [ln for ln in fh.read().split("\n") if ln.strip()]
    has_bv = bool(lines) and "," in lines[0]                      # only the first line is inspected (Commet.py:72)
    for ln in lines:
        names.append(ln.split(":")[0].strip())
        items = ln.split(":")[1].split(";")
        files.append([it.strip().split(",")[0] for it in items])
        if has_bv:
            bvs.append([it.strip().split(",")[1] for it in items])
    return names, files, (bvs if has_bv else None)


# ---- .bv files (boolean_vector.h:302-414) -----------------------------------------------------------
def read_bv(path):
    data = open(path, "rb").read()
    h = data.index(b"#")
    nl = data.index(b"\n", h)
    n = int(data[h + 1:nl])
    raw = np.frombuffer(data[nl + 1:nl + 1 + n // 8 + 1], dtype=np.uint8)
    bits = np.zeros(n // 8 + 1, dtype=np.uint8)
    bits[:raw.size] = raw
    return n, bits


def write_bv(path, comment, n, bits):
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o600)
    with os.fdopen(fd, "wb") as fh:
        fh.write(comment.encode() + b"\n#%d\n" % n)
        fh.write(np.ascontiguousarray(bits[:n // 8 + 1], dtype=np.uint8).tobytes())


def c_atoi(text):
    """what C's atoi makes of a string: blanks, a sign, then digits up to the first other character (filter_reads reads -l, -n, -m so)"""
    t = text.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if t[:1] in ("+", "-"):
        sign, i = (-1 if t[0] == "-" else 1), 1
    j = i
    while j < len(t) and t[j] in "0123456789":
        j += 1
    return sign * int(t[i:j]) if j > i else 0


def filter_comment(read_file, l=0, n=-1, e=0.0):
    """the comment block `filter_reads <read_file> -l l [-n n] -e e` puts in front of its vector (filter_reads.cpp:160-176): the file's base
    name, then the options as its stream prints them — `infinite` when -n is not given, -e as a C++ stream prints the float it was read into"""
    i = read_file.rfind("/")
    return ("----------------\nReference file\n  " + (read_file[i + 1:] if i > 0 else read_file) + "\nFilter Options\n"
            "  min read size     : %d\n  max number of N   : %s\n  min shannon index : %s\n"
            % (l, "infinite" if n < 0 else "%d" % n, "%g" % float(np.float32(e))))


def write_filter_bv(path, read_file, count, bits, l=0, n=-1, e=0.0):
    """The .bv `filter_reads <read_file> -l l [-n n] -e e [-m m] -o <path>` writes (boolean_vector.h:302-346), from the file's final bits
    (count reads; -m shows in the bits only).  Appears complete or not at all (written under another name, renamed)."""
    write_bv(path + ".part", filter_comment(read_file, l, n, e), count, bits)
    os.rename(path + ".part", path)


def default_filter_bv(path, read_file, n):
    """What `filter_reads <read_file> -l 0 -e 0 -o <path>` writes (filter_reads.cpp:160-176, boolean_vector.h:148-164, 302-346): with the
    default options no read can be removed, so the vector is all ones over the file's n reads (padding bits cleared) behind the tool's
    comment block — written from the parser's record count instead of a second pass over the file.  Returns the bits."""
    bits = np.full(n // 8 + 1, 0xFF, dtype=np.uint8)
    bits[-1] = (1 << (n & 7)) - 1                                   # bits n .. of the last byte (all of it when n % 8 == 0) are padding
    if path is not None:
        write_filter_bv(path, read_file, n, bits)
    return bits


def filter_command(bin_dir, read_file, bv_path, l, n, e, m, files_in_set):
    """the filter_reads run Commet.py makes for one file of a set (Commet.py:103-121): -n and -m only when given, -m shared out over the set's files"""
    cmd = [os.path.join(bin_dir, "filter_reads"), read_file, "-l", str(l), "-e", str(e)]
    if n >= 0:
        cmd += ["-n", str(n)]
    if m >= 0:
        cmd += ["-m", str(m / files_in_set)]
    return cmd + ["-o", bv_path]


def popcount(bits, n):
    return int(np.unpackbits(bits[:n // 8 + 1], bitorder="little")[:n].sum())


def concat_bits(parts):
    """[(n, bits)] of the files of a set -> set-wide (N, bits)"""
    if len(parts) == 1:
        return parts[0]
    bools = np.concatenate([np.unpackbits(b[:n // 8 + 1], bitorder="little")[:n] for n, b in parts])
    out = np.zeros(bools.size // 8 + 1, dtype=np.uint8)
    pk = np.packbits(bools, bitorder="little")
    out[:pk.size] = pk
    return bools.size, out


def split_bits(bits, counts):
    """set-wide bits -> per-file bit arrays (each n/8+1 bytes)"""
    if len(counts) == 1:
        return [np.ascontiguousarray(bits[:counts[0] // 8 + 1])]
    total = sum(counts)
    bools = np.unpackbits(bits[:total // 8 + 1], bitorder="little")[:total]
    out, pos = [], 0
    for c in counts:
        b = np.zeros(c // 8 + 1, dtype=np.uint8)
        pk = np.packbits(bools[pos:pos + c], bitorder="little")
        b[:pk.size] = pk
        out.append(b)
        pos += c
    return out


# ---- the three matrices, formatted like Commet.py:276-317 ------------------------------------------
def write_matrices(out_dir, names, considered, shared):
    n = len(names)
    head = "".join(";" + s for s in names) + "\n"
    with open(out_dir + "matrix_plain.csv", "w") as fh:
        fh.write(head)
        for i in range(n):
            fh.write(names[i] + "".join(";" + str(shared[i][j]) for j in range(n)) + "\n")
    with open(out_dir + "matrix_percentage.csv", "w") as fh:
        fh.write(head)
        for i in range(n):
            fh.write(names[i] + "".join(";" + str(100 * shared[i][j] / float(considered[i])) for j in range(n)) + "\n")
    with open(out_dir + "matrix_normalized.csv", "w") as fh:
        fh.write(head)
        for i in range(n):
            fh.write(names[i] + "".join(
                ";" + str(100 * (shared[i][j] + shared[j][i]) / float(considered[i] + considered[j])) for j in range(n)) + "\n")


def _log(out_dir, search_name, index_name, st, index_ms, wall_s):
    with open(f"{out_dir}{search_name}_in_{index_name}.log", "w") as fh:
        fh.write(f"Index  time: {index_ms / 1000.0:g} s\nSearch time: {st['search_ms'] / 1000.0:g} s\n"
                 f"Total  time: {wall_s:g} s\n[indexed {st['indexed']}, searched {st['searched']}, shared {st['shared']}]\n")
