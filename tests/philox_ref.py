"""numpy restatement of the device candidate law (include/mpo.h, mpo_space_sample):
Philox4x32-10, ``u53`` and the per-dimension maps.  The yardstick of
tests/test_candidates_gpu.py; tests/test_candidates_host.py pins it to the Random123
known-answer vectors."""
import numpy as np

from mpi_opt_amd.space import Categorical, Integer

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (or ints) of one shape, key: 2 ints -> 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]           # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def u53(a, b):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)) * np.uint64(1 << 26) + (b >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def sample_transformed(dimensions, n, seed, first=0):
    """Rows first .. first + n - 1 of the candidate set of ``seed``: (n, d) float64."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(first)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    cols = []
    for j, dim in enumerate(dimensions):
        r = philox4x32_10((i & MASK, i >> np.uint64(32), np.full(n, j // 2), np.zeros(n)), key)
        u = u53(r[2], r[3]) if j % 2 else u53(r[0], r[1])
        if isinstance(dim, Integer):
            s = float(dim.high - dim.low)
            cols.append(np.zeros(n) if s == 0 else np.rint(u * s) / s)
        elif isinstance(dim, Categorical):
            c = len(dim.categories)
            idx = np.minimum((u * c).astype(np.int64), c - 1)
            cols.append(idx.astype(np.float64) if c <= 2 else (idx[:, None] == np.arange(c)).astype(np.float64))
        else:
            cols.append(u)
    return np.column_stack(cols)
