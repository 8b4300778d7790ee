"""The yardstick of the train_stats/* tests: a float64 two-pass restatement of get_adj_diff_stats (reference dgm.py:1313-1350) on dense
numpy arrays, and the comparison rule.  test_adj_stats_host.py holds it against the scalars the reference itself wrote (fixtures
adj_stats_*.npz); test_adj_stats.py holds the kernel and the modules against it."""
import numpy as np

FIELDS = ("on_n", "on_mean", "on_std", "off_n", "off_mean", "off_std", "in_deg_mean", "k_diff_mean", "k_diff_std", "k_mean")
# the seven tags the reference writes, in its order (dgm.py:1337-1348), and the field of FIELDS behind each
TAGS = ("on_edge_mean", "on_edge_std", "off_edge_mean", "off_edge_std", "in_deg_mean", "k_diff_mean", "k_mean")
TAG_FIELD = dict(zip(TAGS, ("on_mean", "on_std", "off_mean", "off_std", "in_deg_mean", "k_diff_mean", "k_mean")))
# Tolerance against the float64 restatement.  The kernel carries every moment in double (relative error ~1e-15 over these sizes, nothing
# next to float32) and rounds ONCE, when it stores: a correctly rounded float32 is within 2^-24 relative of the double it came from.  The
# square root of the std is taken in double before that rounding.  The differences d themselves are float32 subtractions on BOTH sides
# (the reference subtracts in float32, dgm.py:1323), so they are identical inputs, not an error source.  2^-22 leaves two bits over the
# one rounding for the double arithmetic's own reordering (Chan's merges against a two-pass sum).
RTOL = 2.0 ** -22


def moments(v):
    """two-pass mean and UNBIASED std in float64; NaN where torch.mean / torch.std give NaN (n == 0; std also n == 1)"""
    v = np.asarray(v, np.float64).reshape(-1)
    n = v.size
    mean = v.sum() / n if n else np.nan
    std = np.sqrt(((v - mean) ** 2).sum() / (n - 1)) if n > 1 else np.nan
    return float(n), float(mean), float(std)


def stats_dense(A, W, k):
    """A [N,N] float32: the input graph (0 where nothing is stored); W [N,N] float32: the learned soft adjacency; k [N] -> {field: float64}.
    The differences are float32 subtractions, as the reference's; everything after them is float64."""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    d = A - W
    on = moments(d[(A > 0) & (d != 0)])
    off = moments(d[(A == 0) & (d != 0)])
    deg = A.astype(np.float64).sum(1)
    k = np.asarray(k, np.float64).reshape(-1)
    kd = moments(k - deg)
    mean = lambda v: float(v.sum() / v.size) if v.size else float("nan")  # noqa: E731
    return dict(zip(FIELDS, (*on, *off, mean(deg), kd[1], kd[2], mean(k))))


def dense_from_triplets(n, rows, cols, vals):
    out = np.zeros((n, n), np.float32)
    out[np.asarray(rows, np.int64), np.asarray(cols, np.int64)] = vals
    return out


def close(got, want, extra=0.0, rtol=RTOL):
    """NaN matches NaN (and only NaN); otherwise |got - want| <= extra + rtol |want|"""
    got, want = float(got), float(want)
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return abs(got - want) <= extra + rtol * abs(want)


def assert_fields(got, want, fields=FIELDS, extra=None, what=""):
    """got / want: {field: number}; prints every figure before asserting"""
    bad = []
    for f in fields:
        ex = 0.0 if extra is None else float(extra.get(f, 0.0))
        ok = close(got[f], want[f], ex)
        print(f"{what} {f:12s} got {float(got[f])!r:>24} want {float(want[f])!r:>24} |diff| {abs(float(got[f]) - float(want[f])):.3e} {'ok' if ok else 'MISS'}")
        if not ok:
            bad.append(f)
    assert not bad, f"{what}: {bad} outside the bound"
