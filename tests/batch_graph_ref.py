"""numpy restatement of the batch edit (include/dgg_hip_batch_graph.h), what tests/test_batch_graph.py compares the GPU against bit for
bit and tests/test_batch_graph_host.py holds against a dense construction:
    hash_rows(...)  x(i,j) of the noise law, mix32 in uint32 arithmetic (tests/subgraph_ref.py's)
    threshold(p)    thr = min(2^32, int(p * 2^32))
    edit(...)       the noisy graph (every stored entry plus every noisy pair, columns ascending, nsrc the stored position or -1) and the
                    target (its entries between nodes of one label), row by row as a sorted merge
    dense(...)      the same two graphs as dense matrices built from masks, a different route to the same answer
and the small graphs both test files use: for every n an empty graph, one with empty rows and one full row, a random one of about 8
entries a row with non-unit values, one with stored self loops and one whose stored columns sit on the window edges 63, 64, 127, 128."""
import numpy as np

from subgraph_ref import GOLDEN, M32, mix32, random_graph

SIZES = (1, 2, 63, 64, 65, 130, 300)
GRAPHS = ("empty", "sparse_full", "random", "selfloops", "edges")
LABELS = ("equal", "different", "three", None)


def threshold(p):
    assert 0.0 <= p <= 1.0
    return min(1 << 32, int(float(p) * 4294967296.0))


def hash_rows(rows, n, seed):
    """x(i, j) for i in rows, j in 0..n-1 -> uint64 [len(rows), n] holding uint32 values"""
    s0, s1 = int(seed[0]) & M32, int(seed[1]) & M32
    key = mix32(np.asarray(rows, np.uint64) ^ np.uint64(s0)) ^ np.uint64(s1)
    j = (np.arange(n, dtype=np.uint64) * np.uint64(GOLDEN)) & np.uint64(M32)
    return mix32(key[:, None] ^ j[None, :])


def noisy_row(i, n, stored, thr, seed):
    """the noisy columns of row i, ascending: hits off the diagonal that are not stored"""
    hit = np.flatnonzero(hash_rows([i], n, seed)[0] < np.uint64(thr))
    return np.setdiff1d(hit[hit != i], stored, assume_unique=True)


def edit(rowptr, col, values, thr, seed, labels=None):
    """-> dict(nrowptr int64 [n+1], ncol int32, nrow int32, nval float32, nsrc int64, n, e; with labels trowptr, tcol, trow, e_t)"""
    n = len(rowptr) - 1
    ncol, nrow, nval, nsrc, nrowptr = [], [], [], [], [0]
    tcol, trow, trowptr = [], [], [0]
    for i in range(n):
        p0, p1 = int(rowptr[i]), int(rowptr[i + 1])
        stored = np.asarray(col[p0:p1], np.int64)
        noise = noisy_row(i, n, stored, thr, seed)
        cols = np.concatenate([stored, noise])
        src = np.concatenate([np.arange(p0, p1, dtype=np.int64), np.full(noise.size, -1, np.int64)])
        val = np.concatenate([np.asarray(values[p0:p1], np.float32), np.ones(noise.size, np.float32)])
        order = np.argsort(cols, kind="stable")                          # a merge of two ascending, disjoint sets
        cols, src, val = cols[order], src[order], val[order]
        ncol.append(cols)
        nsrc.append(src)
        nval.append(val)
        nrow.append(np.full(cols.size, i, np.int64))
        nrowptr.append(nrowptr[-1] + cols.size)
        if labels is not None:
            same = cols[np.asarray(labels)[cols] == labels[i]]
            tcol.append(same)
            trow.append(np.full(same.size, i, np.int64))
            trowptr.append(trowptr[-1] + same.size)
    cat = lambda parts, dt: np.concatenate(parts + [np.zeros(0, dt)]).astype(dt)  # noqa: E731
    out = dict(nrowptr=np.asarray(nrowptr, np.int64), ncol=cat(ncol, np.int32), nrow=cat(nrow, np.int32), nval=cat(nval, np.float32),
               nsrc=cat(nsrc, np.int64), n=n, e=nrowptr[-1], e_t=0)
    if labels is not None:
        out.update(trowptr=np.asarray(trowptr, np.int64), tcol=cat(tcol, np.int32), trow=cat(trow, np.int32), e_t=trowptr[-1])
    return out


def dense_graph(rowptr, col, values):
    n = len(rowptr) - 1
    A = np.zeros((n, n), np.float32)
    A[np.repeat(np.arange(n), np.diff(rowptr)), col] = values
    return A


def dense(rowptr, col, values, thr, seed, labels=None):
    """-> (noisy graph float32 [n, n], its pattern bool [n, n], target float32 [n, n] or None) from masks: x < thr, minus the diagonal,
    minus the stored entries, added to the dense graph; the same-label mask applied to the noisy pattern"""
    n = len(rowptr) - 1
    stored = np.zeros((n, n), bool)
    stored[np.repeat(np.arange(n), np.diff(rowptr)), col] = True
    mask = hash_rows(np.arange(n), n, seed) < np.uint64(thr)
    mask &= ~np.eye(n, dtype=bool)
    mask &= ~stored
    pattern = stored | mask
    target = None
    if labels is not None:
        lab = np.asarray(labels)
        target = (pattern & (lab[:, None] == lab[None, :])).astype(np.float32)
    return dense_graph(rowptr, col, values) + mask.astype(np.float32), pattern, target


def to_dense(n, rowptr, cols, vals):
    A = np.zeros((n, n), np.float32)
    A[np.repeat(np.arange(n), np.diff(rowptr)), cols] = vals
    return A


def csr_from_rows(rows, n, seed):
    """rows: list of ascending column lists -> (rowptr int64 [n+1], col int32 [E], values float32 [E] in [0.5, 1.5))"""
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    col = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    values = (np.random.default_rng(seed).random(col.size) + 0.5).astype(np.float32)
    return rowptr, col, values


def graph(name, n):
    rng = np.random.default_rng(n * 7 + GRAPHS.index(name))
    if name == "empty":
        return csr_from_rows([[] for _ in range(n)], n, 0)
    if name == "sparse_full":                                            # every third row empty, row n // 2 full (its diagonal included)
        rows = [[] if i % 3 == 0 else sorted(rng.choice(n, min(n, 3), replace=False).tolist()) for i in range(n)]
        rows[n // 2] = list(range(n))
        return csr_from_rows(rows, n, 1)
    if name == "random":
        return random_graph(n, np.minimum(rng.integers(4, 13, n), n), n + 2)
    if name == "selfloops":                                              # every second row stores its diagonal entry
        rows = [sorted(set(rng.choice(n, min(n, 5), replace=False).tolist()) | ({i} if i % 2 == 0 else set())) for i in range(n)]
        return csr_from_rows(rows, n, 3)
    assert name == "edges"                                               # stored columns on both sides of the 64-column window edges
    on = [c for c in (0, 63, 64, 127, 128, n - 1) if c < n]
    return csr_from_rows([sorted(set(on if i % 4 else on[1:-1])) for i in range(n)], n, 4)


def labels(kind, n):
    if kind is None:
        return None
    if kind == "equal":
        return np.full(n, 5, np.int64)
    if kind == "different":
        return np.arange(n, dtype=np.int64)[::-1].copy() - 3             # (a negative class id is a class id)
    return np.random.default_rng(n).integers(0, 3, n).astype(np.int64)


def noise_counts(n, thr, seed):
    """-> (hits over the n(n-1) off-diagonal pairs, unordered pairs {i,j} hit in both directions)"""
    mask = hash_rows(np.arange(n), n, seed) < np.uint64(thr)
    mask &= ~np.eye(n, dtype=bool)
    return int(mask.sum()), int((mask & mask.T).sum()) // 2, mask
