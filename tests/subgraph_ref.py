"""numpy restatement of the two sampling kernels (include/dgg_hip_sampling.h), what tests/test_subgraph.py compares the GPU against bit
for bit and tests/test_subgraph_host.py holds against scipy:
    walk(...)      the random-walk law, mix32 in uint32 arithmetic
    induced(...)   the sub-graph induced by a node set with the monotone relabelling, the kept entries in their stored order, and the
                   row sums of the kept values in the kernel's fixed order (64 lane sums in double, xor butterfly, one rounding)
and the 300-node graph both test files use (rows of 0, 1, 63, 64, 65, 128, 129 and 200 entries: every side of the 64-lane stride)."""
import numpy as np

M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9


def mix32(x):
    """csrc/dgg_common.h mix32 on python ints / uint64 arrays holding uint32 values"""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def pick(x, d):
    """((uint64)x * d) >> 32 for uint32 x and 1 <= d < 2^32 (python ints: no overflow to reason about)"""
    return (int(x) * int(d)) >> 32


def walk(rowptr, col, roots, L, seed):
    """-> int32 [B, L+1]"""
    s0, s1 = int(seed[0]) & M32, int(seed[1]) & M32
    B = len(roots)
    out = np.empty((B, L + 1), np.int32)
    for b in range(B):
        v = int(roots[b])
        out[b, 0] = v
        kb = int(mix32(b ^ s0)) ^ s1
        for t in range(1, L + 1):
            p0, p1 = int(rowptr[v]), int(rowptr[v + 1])
            if p1 > p0:
                x = int(mix32(kb ^ ((t * GOLDEN) & M32)))
                v = int(col[p0 + pick(x, p1 - p0)])
            out[b, t] = v
    return out


def lane_sum(vals64, lanes):
    """the kernel's order: lane l adds its entries in ascending position in double; the 64 sums fold by the xor butterfly 32, .., 1"""
    s = np.zeros(64, np.float64)
    for v, l in zip(vals64, lanes):
        s[l] = s[l] + v
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[np.arange(64) ^ off]
    return np.float32(s[0])


def induced(rowptr, col, nodes, values=None):
    """-> dict(orig int32 [n], newid int32 [N], browptr int64 [n+1], bcol int32 [e], brow int32 [e], beid int64 [e], bdeg float32 [n] or None)"""
    N = len(rowptr) - 1
    flag = np.zeros(N, bool)
    flag[np.asarray(nodes, np.int64)] = True
    orig = np.flatnonzero(flag).astype(np.int32)
    newid = np.where(flag, np.cumsum(flag) - 1, -1).astype(np.int32)
    bcol, brow, beid, bdeg, browptr = [], [], [], [], [0]
    for r, v in enumerate(orig):
        p0, p1 = int(rowptr[v]), int(rowptr[v + 1])
        kept = [p for p in range(p0, p1) if newid[col[p]] >= 0]
        bcol += [int(newid[col[p]]) for p in kept]
        brow += [r] * len(kept)
        beid += kept
        browptr.append(browptr[-1] + len(kept))
        if values is not None:
            bdeg.append(lane_sum([np.float64(values[p]) for p in kept], [(p - p0) % 64 for p in kept]))
    return dict(orig=orig, newid=newid, browptr=np.asarray(browptr, np.int64), bcol=np.asarray(bcol, np.int32), brow=np.asarray(brow, np.int32),
                beid=np.asarray(beid, np.int64), bdeg=None if values is None else np.asarray(bdeg, np.float32), n=len(orig), e=len(beid))


def random_graph(N, degs, seed):
    """directed CSR graph with the given out-degrees: columns strictly ascending within a row, values float32 in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(N + 1, np.int64)
    np.cumsum(degs, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(N, int(d), replace=False)) for d in degs] + [np.zeros(0, np.int64)]).astype(np.int32)
    values = (rng.random(col.size) + 0.5).astype(np.float32)
    return rowptr, col, values


N300 = 300
SPECIAL_DEGREES = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 200, 6: 0, 7: 128, 8: 129}       # node -> out-degree


def graph300():
    """N = 300; nodes 0 and 6 have no out-edge (a walk rooted there never leaves), node 5 has 200: four strides, the last one partial"""
    degs = np.random.default_rng(0).integers(2, 12, N300)
    for v, d in SPECIAL_DEGREES.items():
        degs[v] = d
    return random_graph(N300, degs, 1)


def independent_set(rowptr, col, want):
    """`want` nodes no two of which are joined by a stored entry in either direction (and none with a self loop), greedily"""
    N = len(rowptr) - 1
    blocked = np.zeros(N, bool)
    src = np.repeat(np.arange(N), np.diff(rowptr))
    out = []
    for v in range(N):
        nb = col[rowptr[v]:rowptr[v + 1]]
        if blocked[v] or v in nb:
            continue
        out.append(v)
        blocked[nb] = True
        blocked[src[col == v]] = True
        if len(out) == want:
            break
    assert len(out) == want, "the graph is too dense for an independent set of that size"
    return np.asarray(out, np.int32)
