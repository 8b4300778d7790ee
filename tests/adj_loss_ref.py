"""The yardstick of the adjacency-loss tests: a float64 numpy restatement, on the SPARSE data, of

    S = sum over the stored (i,j) of A of (a_ij - g_ij)^2  +  sum over the (i,j) stored in G and not in A of g_ij^2
    loss = S / (rows * N) ('mean', F.mse_loss of the two dense matrices)   or   S ('sum')

and of the per-entry gradient d loss / d a_e = scale * 2 * (a_e - g_e), plus the problems both test files run: the three row forms of the
learned adjacency with the awkward cases of the issue in every target graph.  test_adj_loss_host.py holds the restatement against
torch.nn.functional.mse_loss on the dense float64 matrices; test_adj_loss.py holds the kernel and the modules against the restatement.

Tolerances (derived, not measured).  Every term of S is a square, so nothing cancels and relative errors of the terms bound the relative
error of the sum.  The kernel forms d = a - g as one float32 subtraction (relative error <= 2^-24), squares it in double (2^-23 on the
term), sums in double (negligible) and rounds the result to float32 once (2^-24): 3 * 2^-24 < RTOL = 2^-22.  The gradient is the same d
(2^-24), times a scale that was rounded to float32 on the host (2^-24), the product rounded once (2^-24): 3 * 2^-24 < RTOL again.  Where
a == g exactly the gradient is exactly 0, as it is at padding."""
import math

import numpy as np

RTOL = 2.0 ** -22


def learned_triplets(form, arrs, n):
    """the learned adjacency as flat (row, col, val) over EVERY slot, col < 0 for padding (a chunk past cptr[n] is padding whatever it
    holds) -- form 'list': (idx [n,K], val); 'chunked': (idx [chunks,64], val, cptr [n+1]); 'csr': (rowptr_l [n+1], col_l [E], val [E])"""
    if form == "list":
        idx, val = arrs
        rows = np.repeat(np.arange(n), idx.shape[1])
        return rows, idx.reshape(-1).astype(np.int64), val.reshape(-1)
    if form == "chunked":
        idx, val, cptr = arrs
        cnt = np.diff(cptr.astype(np.int64))
        crow = np.concatenate([np.repeat(np.arange(n), cnt), np.full(idx.shape[0] - int(cptr[n]), -1)])
        rows = np.repeat(crow, 64)
        cols = np.where(rows >= 0, idx.reshape(-1).astype(np.int64), -1)
        return np.maximum(rows, 0), cols, val.reshape(-1)
    assert form == "csr"
    rowptr_l, col_l, val = arrs
    return np.repeat(np.arange(n), np.diff(rowptr_l)), col_l.astype(np.int64), val


def loss_and_grad(n, rows, cols, vals, g_rowptr, g_col, g_val, reduction="mean"):
    """-> (loss as a Python float, grad float64 with the shape of vals): float64 throughout, the sum by math.fsum (exactly rounded)"""
    vals = np.asarray(vals)
    a = vals.reshape(-1).astype(np.float64)
    live = cols >= 0
    g_rows = np.repeat(np.arange(n), np.diff(g_rowptr))
    gkey = g_rows.astype(np.int64) * n + g_col.astype(np.int64)                 # ascending: rows ascending, columns ascending within a row
    assert np.all(np.diff(gkey) > 0), "the target's columns must ascend strictly within a row"
    akey = np.where(live, rows.astype(np.int64) * n + cols, -1)
    assert np.unique(akey[live]).size == int(live.sum()), "a learned row holds a column twice"
    if gkey.size:
        pos = np.minimum(np.searchsorted(gkey, akey), gkey.size - 1)
        g_at = np.where(live & (gkey[pos] == akey), g_val.astype(np.float64)[pos], 0.0)
    else:
        g_at = np.zeros(a.shape)
    d = np.where(live, a - g_at, 0.0)
    missed = ~np.isin(gkey, akey[live])
    S = math.fsum((d * d).tolist()) + math.fsum((g_val.astype(np.float64)[missed] ** 2).tolist())
    scale = 1.0 / (float(n) * float(n)) if reduction == "mean" else 1.0
    return S * scale, (scale * 2.0 * d).reshape(vals.shape)


def close(x, ref, rtol=RTOL):
    return abs(x - ref) <= rtol * abs(ref)


def grad_close(got, ref, rtol=RTOL):
    """elementwise |got - ref| <= rtol |ref|: exact zeros where ref is 0"""
    return np.abs(got.astype(np.float64) - ref) <= rtol * np.abs(ref)


# ---- the problems ---------------------------------------------------------------------------------------------------------------
def target_graph(n, rng, mean_deg=6):
    """CSR target with integer values in {1, 2, 3}: row 0 empty, row 1 of 130 entries (three 64-entry tiles), the others ~mean_deg"""
    lens = rng.integers(1, 2 * mean_deg, n)
    lens[0], lens[1] = 0, 130
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens]).astype(np.int32)
    val = rng.integers(1, 4, col.size).astype(np.float32)
    return rowptr, col, val


def learned_rows(n, widths, graph, rng):
    """per row i: (cols int64 [m_i] distinct, vals float32 [m_i]) with m_i <= widths[i]: part of the target row is held and part is not,
    a third of the held entries carry a == g exactly, and columns outside the target row are held too.  Row 2 holds nothing (all
    padding); row 3 holds its whole target row (as far as it fits) with a == g on all but one entry -- S is tiny beside sum_G g^2 there."""
    rowptr, col, val = graph
    out = []
    for i in range(n):
        gc, gv = col[rowptr[i]:rowptr[i + 1]].astype(np.int64), val[rowptr[i]:rowptr[i + 1]]
        m = 0 if i == 2 else int(rng.integers(1, widths[i] + 1)) if i > 3 else int(widths[i])
        if i == 3:
            take = np.arange(min(gc.size, m))
        else:
            take = np.flatnonzero(rng.random(gc.size) < 0.6)[:m]
        rest = np.setdiff1d(np.arange(n), gc[take])
        cols = np.concatenate([gc[take], rng.choice(rest, min(m - take.size, rest.size), replace=False)]) if i != 3 else gc[take]
        vals = rng.random(cols.size).astype(np.float32)
        same = np.arange(take.size)[::3] if i != 3 else np.arange(1, take.size)
        vals[same] = gv[take][same]                                                  # a == g exactly
        perm = rng.permutation(cols.size)                                            # (slot order is not column order)
        out.append((cols[perm], vals[perm]))
    return out


def problem(name):
    """-> dict(n, form, arrs (numpy, as learned_triplets takes them), graph (rowptr, col, val)); the four shapes of the issue's table and
    'small_*' ones (n <= 60) for the dense comparison on the host"""
    rng = np.random.default_rng(sum(map(ord, name)))
    form, n, K = {"list16": ("list", 150, 16), "list64": ("list", 4200, 64), "chunked": ("chunked", 300, 64), "csr": ("csr", 300, 0),
                  "small_list": ("list", 57, 9), "small_chunked": ("chunked", 60, 64), "small_csr": ("csr", 53, 0)}[name]
    small = name.startswith("small")
    if small:                                        # (a 130-entry row does not fit: rows of 0 and n - 1 entries instead)
        lens = rng.integers(1, 9, n)
        lens[0], lens[1] = 0, n - 1
        rowptr = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=rowptr[1:])
        col = np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens]).astype(np.int32)
        graph = (rowptr, col, rng.integers(1, 4, col.size).astype(np.float32))
    else:
        graph = target_graph(n, rng)
    if form == "list":
        widths = np.full(n, K)
    elif form == "chunked":
        widths = rng.integers(1, min(150, n) + 1, n)
        widths[1], widths[5] = min(150, n), 64       # (rows 0..3 are filled to their width: 3 chunks against the 130-entry row; one exact chunk)
    else:
        widths = rng.integers(1, 41, n)
        widths[1] = 171 if not small else n          # the Pubmed width: three 64-entry pieces
    rows = learned_rows(n, widths, graph, rng)
    if form == "list":
        idx = np.full((n, K), -1, np.int32)
        val = np.full((n, K), 7.0, np.float32)       # empty slots hold a value nobody may read
        for i, (c, v) in enumerate(rows):
            slots = np.sort(rng.choice(K, c.size, replace=False)) if i % 2 else np.arange(c.size)      # padding inside the row, too
            idx[i, slots], val[i, slots] = c, v
        arrs = (idx, val)
    elif form == "chunked":
        cnt = np.array([(c.size + 63) // 64 for c, _ in rows])                        # row 2: zero chunks
        cptr = np.zeros(n + 1, np.int32)
        np.cumsum(cnt, out=cptr[1:])
        trailing = 2                                                                 # chunks past cptr[n]: nobody's
        idx = np.full((int(cptr[n]) + trailing, 64), -1, np.int32)
        val = np.full(idx.shape, 7.0, np.float32)
        for i, (c, v) in enumerate(rows):
            fi, fv = idx[cptr[i]:cptr[i + 1]].reshape(-1), val[cptr[i]:cptr[i + 1]].reshape(-1)         # (views)
            fi[:c.size], fv[:c.size] = c, v
        arrs = (idx, val, cptr)
    else:
        rows[2] = (np.full(3, -1, np.int64), np.full(3, 7.0, np.float32))              # padding has a CSR spelling too: a column < 0
        rowptr_l = np.zeros(n + 1, np.int64)
        np.cumsum([c.size for c, _ in rows], out=rowptr_l[1:])
        arrs = (rowptr_l, np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([v for _, v in rows]))
    return dict(n=n, form=form, arrs=arrs, graph=graph, rows=rows)


def check_awkward_cases(p):
    """the cases every target graph must include are really there"""
    n, (rowptr, col, val) = p["n"], p["graph"]
    r, c, v = learned_triplets(p["form"], p["arrs"], n)
    live = c >= 0
    lens = np.diff(rowptr)
    assert lens[0] == 0 and lens[1] == (130 if n >= 150 else n - 1)
    gkey = np.repeat(np.arange(n), lens) * n + col
    akey = (r * n + c)[live]
    assert (~np.isin(gkey, akey)).any() and (~np.isin(akey, gkey)).any(), "entries of G outside A, and the reverse"
    _, g = loss_and_grad(n, r, c, v, rowptr, col, val)
    assert (g.reshape(-1)[live & np.isin(r * n + c, gkey)] == 0).any(), "a == g exactly under a learned entry"
    assert not live[r == 2].any() and lens[2] > 0, "a learned row that is all padding"
    assert np.all(val == np.round(val)) and (~live).any()
