"""The rule of the map merge, `cat map-*.dat | LC_ALL=C sort -k 1 -g -k 2 -g` on shmr_map's lines, as the tests'
oracle: the bytes form (field 0 and field 1 as numbers, then the whole line), the numeric-key form (per field the decimal string's rank
among decimal strings, (v * 10^(10 - ndigits), ndigits)), GNU sort itself where it is installed, and seeded generators of map lines that
are dense in ties and in digit-length boundaries.  A line here is nine canonical decimals below 2^32 separated by single blanks, without
its newline."""
import os
import shutil
import subprocess

import numpy as np

BOUNDARY = (0, 1, 9, 10, 11, 99, 100, 999999999, 1000000000, 4294967295)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mapmerge_cases.npz")


def rule_sorted(lines):
    """the bytes form: by field 0 as a number, by field 1 as a number, then by the whole line bytewise"""
    def key(l):
        f = l.split(" ", 2)
        return (int(f[0]), int(f[1]), l.encode())
    return sorted(lines, key=key)


def field_key(v: int):
    nd = len(str(v))
    return (v * 10 ** (10 - nd), nd)


def numeric_sorted(lines):
    """the numeric-key form: what the kernels compare"""
    def key(l):
        f = [int(x) for x in l.split(" ")]
        return (f[0], f[1]) + tuple(field_key(v) for v in f[2:])
    return sorted(lines, key=key)


def gnu_sort(lines):
    """`LC_ALL=C sort -k 1 -g -k 2 -g` on the lines, or None where there is no sort"""
    exe = shutil.which("sort")
    if exe is None:
        return None
    env = {"LC_ALL": "C", "PATH": os.environ.get("PATH", "")}
    data = "".join(l + "\n" for l in lines).encode()
    out = subprocess.run([exe, "-k", "1", "-g", "-k", "2", "-g"], input=data, stdout=subprocess.PIPE, check=True, env=env).stdout
    return out.decode().splitlines()


def text_of(lines) -> bytes:
    return "".join(l + "\n" for l in lines).encode()


def rows_of(lines) -> np.ndarray:
    return np.array([[int(x) for x in l.split(" ")] for l in lines], np.int64).reshape(-1, 9)


def lines_of(rows) -> list:
    return [" ".join(str(int(v)) for v in r) for r in np.asarray(rows).reshape(-1, 9)]


def boundary_lines(rng, n: int, n_keys: int = 6):
    """every field from the digit-length boundaries: text order and numeric order disagree in fields 2 .. 8, few (field 0, field 1) keys"""
    keys = [(int(rng.choice(BOUNDARY)), int(rng.choice(BOUNDARY))) for _ in range(n_keys)]
    out = []
    for _ in range(n):
        k = keys[int(rng.integers(len(keys)))]
        out.append(" ".join(str(v) for v in k + tuple(int(rng.choice(BOUNDARY)) for _ in range(7))))
    return out


def run_lines(rng, lengths, differ=(2, 3, 4, 5, 6, 7, 8), wide=False):
    """runs of the given lengths, one (field 0, field 1) key each, shuffled: the rows of a run differ in the fields `differ` only, drawn
    from values of mixed digit lengths (wide: from all of [0, 2^32))"""
    out = []
    for r, n in enumerate(lengths):
        base = [int(rng.integers(0, 50)), int(rng.integers(0, 10 ** int(rng.integers(1, 10))))]
        base[0] = r   # distinct keys
        rest = [int(rng.integers(0, 1000)) for _ in range(7)]
        for _ in range(n):
            row = list(rest)
            for f in differ:
                row[f - 2] = int(rng.integers(0, 1 << 32)) if wide else int(rng.integers(0, 10 ** int(rng.integers(1, 5))))
            out.append(" ".join(str(v) for v in base + row))
    return [out[i] for i in rng.permutation(len(out))]


def mapped_lines(rng, n: int, per_key: int = 30):
    """lines as shmr_map writes them for a job: about per_key rows per (contig, position), reads and positions of realistic widths"""
    n_keys = max(1, n // per_key)
    ctg = rng.integers(0, 40, n_keys)
    pos = rng.integers(0, 5_000_000, n_keys)
    k = rng.integers(0, n_keys, n)
    rb = rng.integers(0, 30_000, n)
    span = rng.integers(100, 3000, n)
    cols = [ctg[k], pos[k], pos[k] + span, rng.integers(0, 800_000, n), rb, rb + span, rng.integers(0, 2, n), rng.integers(1, 60, n), rng.integers(1, 60, n)]
    return [" ".join(str(int(c[i])) for c in cols) for i in range(n)]


def load_fixture():
    """(the chunk files' texts in order, GNU sort's merged file) of tests/golden/mapmerge_cases.npz"""
    z = np.load(GOLD)
    return [z[f"map_{c}"].tobytes() for c in (1, 2, 3)], z["sorted"].tobytes()
