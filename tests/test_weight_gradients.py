"""The weight-gradient GEMM family of csrc/dgg_linear.hip against exact and float64 references.

Every parameter gradient of the dense layers is a transposed product  C[M1,M2] += (A * act'(Y))^T B  (+ the column sums of the
masked A = the bias gradient), behind four C entry points: dgg_gemm_tn_acc, dgg_linear_bwd, dgg_gemm_tn_multi, dgg_gemm_tn_pairs.
This module calls them through the C ABI (ops.* would hide misaligned operands, nullable arguments and guard buffers).

Tier 1 (exact).  A holds integers in [-8, 8], B integers in [-15, 15], Y is in {-1, 0, +1}, the activation is none or ReLU,
N <= 100 003.  Every product is an integer, every bf16 split is exact (hi = x, lo = 0) and every partial sum in any order is an
integer below 2^24 -- so every kernel, whatever its summation order, slab count or reducer, must return EXACTLY the integer
product: np.array_equal, no tolerance.  The outputs start from non-zero integers and (where 2^24 allows) the call is made twice:
the result must be initial + 2 x product (the ACCUMULATE contract).  Inputs sit inside NaN-filled buffers, outputs between canary
words, the workspace is exactly what the *_ws_floats function returns (NaN-filled, so a slab the reducer reads but no stream
wrote poisons the result) plus a canary tail.

Tier 2 (real values).  Standard-normal operands, LeakyReLU / ReLU masks with Y = 0.0 entries, against  (A * act'(Y))^T B  in
float64 (the LeakyReLU slope is the float32 0.01 the kernels multiply by).  Statistic: max|got - ref| / max|ref| per output.
The bar per precision class is 4 x the error of the same arithmetic restated on the CPU for the same inputs:
  fp32   float32 matmul of the float32-masked A against float64
  b3     hi = bf16(x), lo = bf16(x - hi);  al^T bh + ah^T bl + ah^T bh  accumulated in float32, against float64
The factor 4 covers a different blocking of the same sum (up to 256 row streams x 4 wavefronts against the host BLAS) and nothing
else.  Column sums are held to 4 x the error of the float32 product of the masked A with a column of ones.

Measured on an MI355X (statistic of C; worst output of the case; `cw` = the same error componentwise against |A|^T |B|):

  case / product                                       cls        CPU    bar=4x    MI355X        cw |    cs CPU cs MI355X
  acc-N100003-64x128nc #0                              fp32  5.66e-07  2.26e-06  2.21e-07  4.43e-09 |  3.61e-06  1.90e-07
  acc-N4097-65x130nt #0                                fp32  3.90e-07  1.56e-06  1.78e-07  1.93e-08 |  3.84e-07  1.55e-07
  acc-N2708-16x1433nc #0                               fp32  4.97e-07  1.99e-06  1.69e-07  2.06e-08 |  5.16e-07  1.04e-07
  lbw-N100003-64x128lc #0                              fp32  7.46e-07  2.98e-06  2.03e-07  5.75e-09 |  3.70e-06  2.16e-07
  lbw-N19717-33x70rt #0                                fp32  2.66e-07  1.06e-06  1.61e-07  1.05e-08 |  2.19e-07  1.09e-07
  lbw-N2100-64x128lt-dx #0                             fp32  4.79e-07  1.91e-06  1.69e-07  3.06e-08 |  2.94e-07  1.32e-07
  multi-N3000-64x128lc+64x128nc+64x128rt #0            fp32  4.87e-07  1.95e-06  1.45e-07  2.34e-08 |  6.49e-07  1.34e-07
  multi-N3000-64x128lc+64x128nc+64x128rt #1            fp32  4.80e-07  1.92e-06  1.85e-07  2.19e-08 |  5.86e-07  1.23e-07
  multi-N3000-64x128lc+64x128nc+64x128rt #2            fp32  3.83e-07  1.53e-06  1.49e-07  2.25e-08 |  4.20e-07  1.39e-07
  multi-N100003-32x96lc+64x96nc+32x96rt #0             fp32  6.01e-07  2.41e-06  2.37e-07  6.80e-09 |  4.40e-07  1.72e-07
  multi-N100003-32x96lc+64x96nc+32x96rt #1             fp32  5.55e-07  2.22e-06  3.62e-07  6.66e-09 |  1.93e-06  1.98e-07
  multi-N100003-32x96lc+64x96nc+32x96rt #2             fp32  4.27e-07  1.71e-06  2.11e-07  6.22e-09 |  4.68e-07  2.69e-07
  multi-N40000-64x128nc+64x128lc-b1 #0                 fp32  3.96e-07  1.58e-06  1.87e-07  6.12e-09 |  2.76e-06  2.06e-07
  multi-N40000-64x128nc+64x128lc-b1 #1                 fp32  4.87e-07  1.95e-06  2.09e-07  9.98e-09 |  1.30e-06  1.12e-07
  multi-N100000-64x128nc+64x128nc+64x128nc #0          b3    3.08e-06  1.23e-05  3.02e-06  7.91e-08 |  3.77e-06  2.33e-07
  multi-N100000-64x128nc+64x128nc+64x128nc #1          b3    4.20e-06  1.68e-05  4.12e-06  8.86e-08 |  2.12e-06  1.46e-07
  multi-N100000-64x128nc+64x128nc+64x128nc #2          b3    4.08e-06  1.63e-05  3.91e-06  7.68e-08 |  2.53e-06  2.30e-07
  multi-N100003-64x128lc+128x128rt #0                  b3    4.93e-06  1.97e-05  5.05e-06  1.47e-07 |  2.99e-06  1.41e-07
  multi-N100003-64x128lc+128x128rt #1                  b3    4.44e-06  1.78e-05  4.60e-06  1.43e-07 |  3.13e-06  1.45e-07
  multi-N4097-64x128nt #0                              b3    4.55e-06  1.82e-05  4.55e-06  4.41e-07 |  5.29e-07  9.93e-08
  multi-N19717-64x500lc+128x500nt #0                   b3    4.50e-06  1.80e-05  4.26e-06  2.59e-07 |  1.41e-06  1.76e-07
  multi-N19717-64x500lc+128x500nt #1                   b3    4.23e-06  1.69e-05  4.19e-06  2.17e-07 |  1.76e-06  1.75e-07
  multi-N2708-64x1432nc+64x1432rc #0                   b3    4.29e-06  1.72e-05  4.26e-06  5.90e-07 |  2.75e-07  1.75e-07
  multi-N2708-64x1432nc+64x1432rc #1                   b3    4.36e-06  1.75e-05  4.40e-06  8.85e-07 |  6.57e-07  6.66e-08
  pairs-N100003-32x65nc+16x32nc+1x16nc #0              fp32  3.65e-07  1.46e-06  1.68e-07  3.81e-09 |  3.83e-07  1.35e-07
  pairs-N100003-32x65nc+16x32nc+1x16nc #1              fp32  7.40e-07  2.96e-06  2.79e-07  3.85e-09 |  9.61e-07  3.83e-07
  pairs-N100003-32x65nc+16x32nc+1x16nc #2              fp32  6.63e-07  2.65e-06  2.51e-07  2.10e-09 |  8.06e-06  1.08e-06
  pairs-N4096-33x128nc+40x1nc+64x96nc #0               fp32  3.96e-07  1.58e-06  1.38e-07  1.26e-08 |  1.04e-06  1.33e-07
  pairs-N4096-33x128nc+40x1nc+64x96nc #1               fp32  4.81e-07  1.92e-06  1.02e-07  6.23e-09 |  3.16e-07  1.26e-07
  pairs-N4096-33x128nc+40x1nc+64x96nc #2               fp32  5.12e-07  2.05e-06  1.55e-07  1.29e-08 |  7.29e-07  1.12e-07

The headline shape (N = 100 000, d = 128, three 64-wide operands, split bf16) measures 3.0e-6 .. 4.1e-6 of max, equal to the CPU
restatement of the same three products: the README's earlier "2e-7 of max" did not hold for standard-normal operands and now
records 4e-6.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ACT_NONE, ACT_LEAKY, ACT_RELU = 0, 1, 2
ERR_ARG, ERR_UNSUPPORTED = 1, 2
CANARY = np.float32(-24680.5)
LEAKY = np.float64(np.float32(0.01))          # the slope the kernels multiply by
INIT_MAX = 100                                 # |initial C|, |initial colsum| of tier 1
EXACT_LIMIT = 1 << 24


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
def P(M1, M2, act=ACT_NONE, lay=0, cs=True, y=None):
    """one product of a case: A [N,M1] (masked through act'(Y) when y), B [N,M2], C layout, column sums wanted"""
    return dict(M1=M1, M2=M2, act=act, lay=lay, cs=cs, y=(act != ACT_NONE) if y is None else y)


def case(kind, N, prods, shiftA=0, shiftB=0, dx=False, cls="fp32"):
    """kind: acc (dgg_gemm_tn_acc) | lbw (dgg_linear_bwd) | multi (dgg_gemm_tn_multi, one shared B) | pairs (dgg_gemm_tn_pairs).
    shiftA / shiftB: operands offset by that many floats from a 256-byte boundary.  cls: precision class of tier 2."""
    c = dict(kind=kind, N=N, prods=prods, shiftA=shiftA, shiftB=shiftB, dx=dx, cls=cls)
    c["id"] = "%s-N%d-%s%s%s%s" % (kind, N, "+".join("%dx%d%s%s%s%s" % (p["M1"], p["M2"], "nlr"[p["act"]], "ct"[p["lay"]],
                                                                        "" if p["cs"] else "q", "" if p["y"] or p["act"] == 0 else "Y0")
                                                      for p in prods),
                                   "-a%d" % shiftA if shiftA else "", "-b%d" % shiftB if shiftB else "", "-dx" if dx else "")
    return c


ROWS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 40000, 100003]


def _exact_cases():
    cs = []
    # ---- dgg_gemm_tn_acc / dgg_linear_bwd: gemm_tn_persist<mb, nb> + gemm_tn_reduce ------------------------------
    for N in ROWS + [1535, 1536, 1537]:                          # (64 x 128: mb 2, nb 4 -- the full weight of the hot path)
        cs.append(case("acc", N, [P(64, 128, lay=N & 1)]))
        cs.append(case("lbw", N, [P(64, 128, ACT_RELU, lay=N & 1)]))          # masked operand, mb 1
    shapes = [(32, 32), (32, 64), (32, 128), (64, 32), (64, 64), (64, 96), (7, 33), (33, 7), (65, 130), (130, 65), (130, 130),
              (24, 70), (16, 1433), (64, 1433)]
    for i, (M1, M2) in enumerate(shapes):
        big = M2 > 1000
        for j, N in enumerate([ROWS[i % 5], 4097 - (i % 3), 10007 if big else (40000, 100003)[i & 1]]):
            k = i + j
            if j < 2 or i % 2 == 0:                              # (the largest row count alternates between the two entry points)
                cs.append(case("acc", N, [P(M1, M2, lay=k & 1, cs=bool(k & 2))]))
            if j < 2 or i % 2 == 1:
                cs.append(case("lbw", N, [P(M1, M2, ACT_RELU, lay=(k >> 1) & 1, cs=bool(k & 1))]))     # dx NULL: mask on the operand load
            if not big or j == 0:
                cs.append(case("lbw", N if N < 40000 else 20011, [P(M1, M2, (ACT_RELU, ACT_NONE)[k & 1], lay=k & 1, cs=bool(k & 2))],
                               dx=True))                                                            # dx wanted: separate act_bwd
    # ---- dgg_gemm_tn_multi, narrow kernel (gemm_tn_multi<1|2|4> + gemm_tn_reduce_multi) -----------------------
    seglists = {1: [32], 3: [32, 64, 32], 8: [32] * 8, 4: [64, 64, 64, 64]}

    def segs(key, M2, k):
        return [P(m, M2, (ACT_NONE, ACT_RELU)[(k + q) & 1], lay=(k + q) >> 1 & 1, cs=(k + q) % 3 != 0,
                  y=None if (k + q) % 5 else False) for q, m in enumerate(seglists[key])]
    k = 0
    for M2 in (24, 40, 70, 96, 128):
        for key in (1, 3, 8, 4):
            for N in (ROWS[k % 5], (4095, 2000, 1000)[k % 3]):
                cs.append(case("multi", N, segs(key, M2, k)))
                k += 1
    for N in (4096, 4097, 40000, 100003):                        # narrow at any N: the input is not 128 wide
        cs.append(case("multi", N, segs(3, 96, N)))
        cs.append(case("multi", N, segs(8, 70, N + 1)))
    for N in (3000, 4097, 40000):                                # 128 wide, operands in multiples of 64, but misaligned: narrow
        cs.append(case("multi", N, segs(4, 128, N), shiftB=1))
        cs.append(case("multi", N, segs(4, 128, N + 1), shiftA=1))
        cs.append(case("multi", N, segs(3, 96, N), shiftA=1, shiftB=1))
    # ---- dgg_gemm_tn_multi, wide kernel (gemm_tn_wide, split bf16 with and without the mask) ------------------
    for N in (4096, 4097, 10751, 10752, 10753, 16383, 16384, 16385, 40000, 100003):
        cs.append(case("multi", N, [P(64, 128, lay=0), P(64, 128, lay=1, cs=False), P(64, 128)], cls="b3"))
        cs.append(case("multi", N, [P(64, 128, ACT_RELU, lay=N & 1), P(128, 128, lay=1)], cls="b3"))
        cs.append(case("multi", N, [P(64, 128, lay=N & 1)], cls="b3"))                              # 256 row streams
    cs.append(case("multi", 100003, [P(128, 128, ACT_RELU), P(128, 128, ACT_RELU, lay=1, y=False)], cls="b3"))
    # ---- dgg_gemm_tn_multi, tiled wide kernel (inputs wider than 128 columns) ---------------------------------
    for M2, small, large in ((132, 1, 100003), (256, 65, 40000), (500, 1000, 19717), (1432, 2, 10007)):
        for N in (small, 4097, large):
            cs.append(case("multi", N, [P(64, M2, ACT_RELU, lay=1), P(64, M2, lay=0, cs=False)], cls="b3"))
            cs.append(case("multi", N, [P(128, M2, lay=N & 1), P(64, M2, ACT_RELU, lay=1, y=False), P(64, M2, ACT_RELU, cs=False)],
                           cls="b3"))
    # ---- dgg_gemm_tn_pairs (gemm_tn_multi<4> with per-block operands) -----------------------------------------
    knet = {64: [(32, 65), (16, 32), (1, 16)], 32: [(16, 33), (8, 16), (1, 8)], 16: [(8, 17), (4, 8), (1, 4)]}
    for N in ROWS + [8191, 8192, 8193]:
        cs.append(case("pairs", N, [P(a, b) for a, b in knet[64]]))
    for h in (32, 16):
        for N in (65, 4096, 4097, 40000):
            cs.append(case("pairs", N, [P(a, b) for a, b in knet[h]]))
    for N in (2, 4096, 4097, 100003):
        cs.append(case("pairs", N, [P(5, 1), P(40, 128, cs=False), P(33, 96)]))                     # padded M1, M2 = 1 and 128
        cs.append(case("pairs", N, [P(32, m2, cs=bool(q & 1)) for q, m2 in enumerate((1, 7, 32, 33, 64, 96, 127, 128))]))   # 256 rows
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids), "duplicate case ids"
    return cs


EXACT = _exact_cases()

# wide cases repeated in a fresh process per environment knob (the library reads the knobs once per process)
KNOB = [case("multi", N, prods, cls="b3") for N in (4097, 40000) for prods in (
    [P(64, 128, lay=0), P(64, 128, lay=1, cs=False), P(64, 128)],
    [P(64, 128, ACT_RELU, lay=1), P(128, 128)],
    [P(64, 500, ACT_RELU, lay=1), P(64, 500, cs=False)])] + [case("multi", 100003, [P(64, 128), P(64, 128, ACT_RELU)], cls="b3")]

# tier 2: the same branches, real-valued
REAL = [
    case("acc", 100003, [P(64, 128)]),
    case("acc", 4097, [P(65, 130, lay=1)]),
    case("acc", 2708, [P(16, 1433)]),
    case("lbw", 100003, [P(64, 128, ACT_LEAKY)]),
    case("lbw", 19717, [P(33, 70, ACT_RELU, lay=1)]),
    case("lbw", 2100, [P(64, 128, ACT_LEAKY, lay=1)], dx=True),
    case("multi", 3000, [P(64, 128, ACT_LEAKY), P(64, 128), P(64, 128, ACT_RELU, lay=1)]),
    case("multi", 100003, [P(32, 96, ACT_LEAKY), P(64, 96), P(32, 96, ACT_RELU, lay=1)]),
    case("multi", 40000, [P(64, 128), P(64, 128, ACT_LEAKY)], shiftB=1),
    case("multi", 100000, [P(64, 128), P(64, 128), P(64, 128)], cls="b3"),
    case("multi", 100003, [P(64, 128, ACT_LEAKY), P(128, 128, ACT_RELU, lay=1)], cls="b3"),
    case("multi", 4097, [P(64, 128, lay=1)], cls="b3"),
    case("multi", 19717, [P(64, 500, ACT_LEAKY), P(128, 500, lay=1)], cls="b3"),
    case("multi", 2708, [P(64, 1432), P(64, 1432, ACT_RELU)], cls="b3"),
    case("pairs", 100003, [P(32, 65), P(16, 32), P(1, 16)]),
    case("pairs", 4096, [P(33, 128), P(40, 1), P(64, 96)]),
]
HEADLINE = REAL[9]                              # N = 100 000, d = 128, three 64-wide operands: the README's recorded accuracy
README_GRAD_ERR = 4e-6


# ---------------------------------------------------------------------------------------------------------------
# inputs and references (numpy only)
# ---------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> nearest bfloat16 (ties to even) -> float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def act_grad(Y, act, dtype):
    if Y is None or act == ACT_NONE:
        return None
    return np.where(Y > 0, dtype(1), dtype(LEAKY) if act == ACT_LEAKY else dtype(0)).astype(dtype)


def masked(A, Y, act, dtype):
    """A * act'(Y) in `dtype` arithmetic"""
    g = act_grad(Y, act, dtype)
    return A.astype(dtype) if g is None else A.astype(dtype) * g


def tn_reference(A, Y, act, B):
    """(A * act'(Y))^T B and the column sums of the masked A, float64"""
    Am = masked(A, Y, act, np.float64)
    return Am.T @ B.astype(np.float64), Am.sum(axis=0)


def tn_fp32(A, Y, act, B):
    """the same product in float32 arithmetic (the fp32 kernels' precision class)"""
    Am = masked(A, Y, act, np.float32)
    return Am.T @ np.ascontiguousarray(B, np.float32), (Am.T @ np.ones((A.shape[0], 1), np.float32))[:, 0]


def tn_split_bf16(A, Y, act, B):
    """the split-bf16 kernels' arithmetic: hi = bf16(x), lo = bf16(x - hi), al bh + ah bl + ah bh accumulated in float32"""
    Am = masked(A, Y, act, np.float32)
    ah = bf16_round(Am)
    al = bf16_round(Am - ah)
    bh = bf16_round(B)
    bl = bf16_round(np.ascontiguousarray(B, np.float32) - bh)
    return (al.T @ bh + ah.T @ bl) + ah.T @ bh


def rel_max(got, ref):
    m = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (m if m > 0 else 1.0))


def make_inputs(c, real=False):
    """seeded inputs of a case: per product A, Y (or None), B, initial C / colsum; W for dgg_linear_bwd's dx"""
    rng = np.random.default_rng(zlib.crc32((c["id"] + ("-real" if real else "")).encode()))
    N = c["N"]

    def operand(M, lim):
        if real:
            return rng.standard_normal((N, M)).astype(np.float32)
        return rng.integers(-lim, lim + 1, (N, M), dtype=np.int8).astype(np.float32)
    inp = []
    Bshared = operand(c["prods"][0]["M2"], 15) if c["kind"] == "multi" else None
    for p in c["prods"]:
        d = dict(A=operand(p["M1"], 8), B=Bshared if Bshared is not None else operand(p["M2"], 15), Y=None)
        if p["y"]:
            if real:
                Y = rng.standard_normal((N, p["M1"])).astype(np.float32)
                Y[rng.random((N, p["M1"])) < 0.05] = 0.0          # exactly 0.0: act'(0) is the NEGATIVE branch (y > 0 ? ...)
            else:
                Y = rng.integers(-1, 2, (N, p["M1"]), dtype=np.int8).astype(np.float32)
            d["Y"] = Y
        shape = (p["M1"], p["M2"])
        d["C0"] = np.zeros(shape, np.float32) if real else rng.integers(-INIT_MAX, INIT_MAX + 1, shape).astype(np.float32)
        d["cs0"] = np.zeros(p["M1"], np.float32) if real else rng.integers(-INIT_MAX, INIT_MAX + 1, p["M1"]).astype(np.float32)
        if c["dx"]:
            d["W"] = (rng.standard_normal(shape) * 0.3).astype(np.float32) if real else rng.integers(-15, 16, shape).astype(np.float32)
        inp.append(d)
    return inp


def reps_of(c):
    """calls per tier-1 case: two (the accumulate contract) wherever initial + 2 x product stays exact in float32"""
    return 2 if INIT_MAX + 2 * c["N"] * 8 * 15 < EXACT_LIMIT else 1


def exact_expected(c, inp):
    """initial + reps x product as int64 (float64 BLAS is exact on these integers: every sum is far below 2^53)"""
    out = []
    for p, d in zip(c["prods"], inp):
        Cr, sr = tn_reference(d["A"], d["Y"], p["act"], d["B"])
        assert np.array_equal(Cr, np.rint(Cr)) and np.array_equal(sr, np.rint(sr))
        r = reps_of(c)
        out.append((d["C0"].astype(np.int64) + r * Cr.astype(np.int64), d["cs0"].astype(np.int64) + r * sr.astype(np.int64)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# CPU self-checks (no GPU): the exactness premises and the reference helpers
# ---------------------------------------------------------------------------------------------------------------
def test_exactness_premises_hold_for_every_case():
    """N * max|a| * max|b| < 2^24 (with the initial value and both calls), and the inputs survive a bf16 round trip: every split is
    hi = x, lo = 0 and every partial sum of every kernel is an exactly representable integer"""
    for c in EXACT + KNOB:
        assert c["N"] <= 100003 and all(p["act"] in (ACT_NONE, ACT_RELU) for p in c["prods"])
        r = reps_of(c)
        assert r in (1, 2)
        assert INIT_MAX + r * c["N"] * 8 * 15 < EXACT_LIMIT
        for p, d in zip(c["prods"], make_inputs(c)):
            ma, mb = np.abs(d["A"]).max(), np.abs(d["B"]).max()
            assert ma <= 8 and mb <= 15
            assert np.abs(d["C0"]).max() + r * c["N"] * ma * mb < EXACT_LIMIT
            for name in ("A", "B", "C0", "cs0", "W"):
                if name in d:
                    assert np.array_equal(d[name].astype(np.int32), d[name]), name
            for name in ("A", "B"):                              # a float32 IS a bf16 exactly when its low 16 bits are zero
                assert not (d[name].view(np.uint32) & 0xFFFF).any(), "%s does not survive the bf16 round trip" % name
            x = d["A"][:64]
            assert np.array_equal(bf16_round(x), x)
            if d["Y"] is not None:
                assert np.abs(d["Y"]).max() <= 1 and np.array_equal(d["Y"].astype(np.int32), d["Y"])
            if c["dx"]:
                assert p["M1"] * 8 * 15 < EXACT_LIMIT


def test_small_cases_cover_every_entry_point_and_row_count():
    for kind in ("acc", "lbw", "multi", "pairs"):
        rows = {c["N"] for c in EXACT if c["kind"] == kind}
        assert set(ROWS) <= rows, (kind, sorted(set(ROWS) - rows))
    assert {c["cls"] for c in REAL} == {"fp32", "b3"}
    assert any(p["act"] == ACT_LEAKY for c in REAL for p in c["prods"])


def test_bf16_round_is_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, 1.005, -3.1415927, 255.0, 257.0, 0.0, 8.0, -15.0, 1e-30, 3.0e38], np.float32)
    import torch
    assert np.array_equal(bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy())
    assert bf16_round(np.float32(1.00390625)) == 1.0            # tie -> even (1 + 2^-8 sits between 1 and 1 + 2^-7)
    assert bf16_round(np.float32(1.01171875)) == np.float32(1.015625)   # tie -> even, upwards
    ints = np.arange(-256, 257).astype(np.float32)
    assert np.array_equal(bf16_round(ints), ints)


def test_references_match_a_naive_triple_loop():
    rng = np.random.default_rng(11)
    N, M1, M2 = 9, 5, 4
    for act in (ACT_NONE, ACT_LEAKY, ACT_RELU):
        A = rng.standard_normal((N, M1)).astype(np.float32)
        B = rng.standard_normal((N, M2)).astype(np.float32)
        Y = rng.standard_normal((N, M1)).astype(np.float32)
        Y[0, :] = 0.0
        Cn, sn = np.zeros((M1, M2)), np.zeros(M1)
        for o in range(M1):
            for n in range(N):
                g = 1.0 if act == ACT_NONE or Y[n, o] > 0 else (float(np.float32(0.01)) if act == ACT_LEAKY else 0.0)
                sn[o] += float(A[n, o]) * g
                for j in range(M2):
                    Cn[o, j] += float(A[n, o]) * g * float(B[n, j])
        Cr, sr = tn_reference(A, Y, act, B)
        np.testing.assert_allclose(Cr, Cn, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(sr, sn, rtol=1e-13, atol=1e-13)
        Cf, sf = tn_fp32(A, Y, act, B)
        assert Cf.dtype == np.float32 and rel_max(Cf, Cn) < 1e-6 and rel_max(sf, sn) < 1e-6
        Cb = tn_split_bf16(A, Y, act, B)
        assert Cb.dtype == np.float32 and 0 < rel_max(Cb, Cn) < 1e-4          # three of the four partial products
        hi_only = bf16_round(masked(A, Y, act, np.float32)).T @ bf16_round(B)
        assert rel_max(hi_only, Cn) > 10 * rel_max(Cb, Cn)                       # ... and the two small ones matter
    # integers: the float64 reference IS the int64 product
    c = case("multi", 37, [P(32, 40, ACT_RELU), P(64, 40)])
    inp = make_inputs(c)
    for p, d, (Ce, se) in zip(c["prods"], inp, exact_expected(c, inp)):
        Ai = d["A"].astype(np.int64) * (1 if d["Y"] is None else (d["Y"] > 0).astype(np.int64))
        Ci = np.zeros((p["M1"], p["M2"]), np.int64)
        for n in range(c["N"]):
            Ci += np.outer(Ai[n], d["B"][n].astype(np.int64))
        assert np.array_equal(Ce, d["C0"].astype(np.int64) + 2 * Ci) and np.array_equal(se, d["cs0"].astype(np.int64) + 2 * Ai.sum(0))


# ---------------------------------------------------------------------------------------------------------------
# GPU side: guarded buffers and the four entry points through the C ABI
# ---------------------------------------------------------------------------------------------------------------
class Guarded:
    """`body` inside a larger device buffer: `fill` on both sides (NaN around inputs, canary words around outputs); the body starts
    `shift` floats after a 256-byte boundary"""

    def __init__(self, dev, body, fill, shift=0, guard=64):
        import torch
        body = np.ascontiguousarray(body, np.float32)
        g = (max(64, guard) + 63) // 64 * 64
        host = np.full(g + shift + body.size + g, fill, np.float32)
        self.lo, self.n, self.shape, self.fill = g + shift, body.size, body.shape, fill
        host[self.lo:self.lo + self.n] = body.ravel()
        self.buf = torch.from_numpy(host).to(dev)
        self.addr = self.buf.data_ptr() + 4 * self.lo
        assert self.buf.data_ptr() % 256 == 0 and self.addr % 16 == (4 * shift) % 16

    def read(self):
        """(body, guards intact)"""
        h = self.buf.cpu().numpy()
        gd = np.concatenate([h[:self.lo], h[self.lo + self.n:]])
        ok = bool(np.isnan(gd).all()) if np.isnan(self.fill) else bool((gd == self.fill).all())
        return h[self.lo:self.lo + self.n].reshape(self.shape).copy(), ok


def _parr(addrs):
    return (C.c_void_p * len(addrs))(*addrs)


def _iarr(vs):
    return (C.c_int * len(vs))(*[int(v) for v in vs])


class Workspace:
    """exactly `floats` floats of NaN + a canary tail (longer than two row streams' slabs: an overrun lands in the tail)"""

    def __init__(self, dev, floats):
        import torch
        self.floats = int(floats)
        self.tail = self.floats // 100 + 4096
        host = np.full(self.floats + self.tail, np.nan, np.float32)
        host[self.floats:] = CANARY
        self.buf = torch.from_numpy(host).to(dev)
        self.addr = self.buf.data_ptr()

    def tail_intact(self):
        return bool((self.buf[self.floats:] == float(CANARY)).all().item())


def ws_floats(c):
    from dgg_amd import _lib
    L = _lib.lib()
    p0 = c["prods"][0]
    if c["kind"] == "acc":
        return L.dgg_gemm_tn_ws_floats(c["N"], p0["M1"], p0["M2"])
    if c["kind"] == "lbw":
        return L.dgg_linear_bwd_ws_floats(c["N"], p0["M2"], p0["M1"])
    if c["kind"] == "multi":
        return L.dgg_gemm_tn_multi_ws_floats(c["N"], sum(p["M1"] for p in c["prods"]), p0["M2"])
    return L.dgg_gemm_tn_multi_ws_floats(c["N"], sum((p["M1"] + 31) // 32 * 32 for p in c["prods"]), 128)


def call_entry(c, A, Y, B, Cs, css, ws_addr, N=None, W=None, dx=None, nseg=None):
    """one call of the case's entry point on device addresses (None = NULL); returns the status code"""
    from dgg_amd import _lib, ops
    L, st, pr = _lib.lib(), ops._stream(), c["prods"]
    N = c["N"] if N is None else N
    if c["kind"] == "acc":
        return L.dgg_gemm_tn_acc(A[0], B[0], N, pr[0]["M1"], pr[0]["M2"], Cs[0], pr[0]["lay"], css[0], ws_addr, st)
    if c["kind"] == "lbw":
        return L.dgg_linear_bwd(B[0], N, pr[0]["M2"], W, pr[0]["M1"], pr[0]["lay"], pr[0]["act"], Y[0], A[0], dx, Cs[0], css[0], ws_addr, st)
    n = len(pr) if nseg is None else nseg
    if c["kind"] == "multi":
        return L.dgg_gemm_tn_multi(n, _parr(A), _iarr([p["M1"] for p in pr]), _parr(Y), _iarr([p["act"] for p in pr]), B[0], N,
                                   pr[0]["M2"], _parr(Cs), _iarr([p["lay"] for p in pr]), _parr(css), ws_addr, st)
    return L.dgg_gemm_tn_pairs(n, _parr(A), _iarr([p["M1"] for p in pr]), _parr(B), _iarr([p["M2"] for p in pr]), N, _parr(Cs),
                               _parr(css), ws_addr, st)


def run_case(dev, c, inp, reps=1, expect_rc=0, N_call=None, null_ws=False, ws_n=None):
    """uploads the guarded operands, calls the entry point `reps` times, checks every guard and returns per product
    (C as [M1, M2], colsum or None, dx or None).  With expect_rc != 0 (or N_call = 0) the outputs must come back untouched."""
    import torch
    pr, N = c["prods"], c["N"]
    assert all(p["lay"] == 0 for p in pr) or c["kind"] != "pairs"
    gB0 = Guarded(dev, inp[0]["B"], np.nan, c["shiftB"], guard=2 * pr[0]["M2"])
    gA, gY, gB, gC, gcs = [], [], [], [], []
    for q, (p, d) in enumerate(zip(pr, inp)):
        gA.append(Guarded(dev, d["A"], np.nan, c["shiftA"], guard=2 * p["M1"]))
        gY.append(Guarded(dev, d["Y"], np.nan, c["shiftA"], guard=2 * p["M1"]) if d["Y"] is not None else None)
        gB.append(gB0 if (c["kind"] == "multi" or q == 0) else Guarded(dev, d["B"], np.nan, c["shiftB"], guard=2 * p["M2"]))
        gC.append(Guarded(dev, d["C0"] if p["lay"] == 0 else d["C0"].T, CANARY))
        gcs.append(Guarded(dev, d["cs0"], CANARY) if p["cs"] else None)
    W = Guarded(dev, inp[0]["W"] if pr[0]["lay"] == 0 else inp[0]["W"].T, np.nan) if c["dx"] else None
    gdx = Guarded(dev, np.full((N, pr[0]["M2"]), 7.0, np.float32), CANARY) if c["dx"] else None
    ws = Workspace(dev, ws_floats(c) if ws_n is None else ws_n)
    addr = lambda gs: [None if g is None else g.addr for g in gs]
    for _ in range(reps):
        rc = call_entry(c, addr(gA), addr(gY), addr(gB), addr(gC), addr(gcs), None if null_ws else ws.addr, N=N_call,
                        W=None if W is None else W.addr, dx=None if gdx is None else gdx.addr)
        assert rc == expect_rc or (expect_rc == -1 and rc in (ERR_ARG, ERR_UNSUPPORTED)), "%s: status %d" % (c["id"], rc)
    torch.cuda.synchronize()
    assert ws.tail_intact(), "%s: the workspace was overrun (canary tail after %d floats)" % (c["id"], ws.floats)
    res = []
    for q, (p, d) in enumerate(zip(pr, inp)):
        Cb, ok = gC[q].read()
        assert ok, "%s: canary words around C of product %d were overwritten" % (c["id"], q)
        sb = None
        if gcs[q] is not None:
            sb, ok = gcs[q].read()
            assert ok, "%s: canary words around colsum of product %d were overwritten" % (c["id"], q)
        res.append((Cb if p["lay"] == 0 else Cb.T, sb, None))
    if gdx is not None:
        dxb, ok = gdx.read()
        assert ok, "%s: canary words around dx were overwritten" % c["id"]
        res[0] = (res[0][0], res[0][1], dxb)
    if expect_rc != 0 or N_call == 0:
        for (Cb, sb, dxb), d in zip(res, inp):
            assert np.array_equal(Cb, d["C0"]) and (sb is None or np.array_equal(sb, d["cs0"])), "%s: a refused call wrote its outputs" % c["id"]
            assert dxb is None or (dxb == 7.0).all()
    return res


def check_exact(dev, c):
    """runs a tier-1 case; returns a list of mismatch descriptions (empty = exact)"""
    inp = make_inputs(c)
    exp = exact_expected(c, inp)
    got = run_case(dev, c, inp, reps=reps_of(c))
    bad = []
    for q, (p, d, (Ce, se), (Cg, sg, dxg)) in enumerate(zip(c["prods"], inp, exp, got)):
        if not np.array_equal(Cg.astype(np.float64), Ce.astype(np.float64)):
            w = np.argwhere(Cg.astype(np.float64) != Ce)
            bad.append("%s product %d: C differs in %d of %d elements, first at (row %d, column %d): got %r, expected %d; rows %s columns %s"
                       % (c["id"], q, len(w), Ce.size, w[0][0], w[0][1], Cg[tuple(w[0])], Ce[tuple(w[0])],
                          sorted(set(w[:, 0]))[:8], sorted(set(w[:, 1]))[:8]))
        if sg is not None and not np.array_equal(sg.astype(np.float64), se.astype(np.float64)):
            w = np.flatnonzero(sg.astype(np.float64) != se)
            bad.append("%s product %d: colsum differs at %s: got %r, expected %r" % (c["id"], q, w[:8], sg[w[:8]], se[w[:8]]))
        if dxg is not None:
            Wm = d["W"].astype(np.float64)                       # [out, d]
            dxe = masked(d["A"], d["Y"], p["act"], np.float64) @ Wm
            if not np.array_equal(dxg.astype(np.float64), dxe):
                w = np.argwhere(dxg.astype(np.float64) != dxe)
                bad.append("%s: dx differs in %d elements, first at %s" % (c["id"], len(w), w[0]))
    return bad


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------
# tier 1
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", EXACT, ids=[c["id"] for c in EXACT])
def test_exact_integer_product(dev, c):
    """initial + reps x (A * relu'(Y))^T B and the column sums, bit for bit"""
    bad = check_exact(dev, c)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["DGG_TN_B3", "DGG_TN_WIDE"])
def test_exact_integer_product_under_escape_knob(dev, knob):
    """DGG_TN_B3=0 (the fp32 wide kernel) and DGG_TN_WIDE=0 (128-wide inputs through the narrow kernel): a fresh process per knob"""
    env = dict(os.environ)
    env[knob] = "0"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--knob-child"]
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("the %s=0 child process hung: nothing further is started on the GPU" % knob, returncode=3)
    out = r.stdout.decode(errors="replace")
    if r.returncode not in (0, 1):
        pytest.exit("the %s=0 child process ended abnormally (status %d): nothing further is started on the GPU\n%s"
                    % (knob, r.returncode, out[-2000:]), returncode=3)
    assert r.returncode == 0 and "KNOB_CHILD_OK %d" % len(KNOB) in out, out[-4000:]


def _knob_child():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import dgg_amd  # noqa: F401
    d = torch.device("cuda:0")
    bad = []
    for c in KNOB:
        bad += check_exact(d, c)
    if bad:
        print("\n".join(bad))
        return 1
    print("KNOB_CHILD_OK %d" % len(KNOB))
    return 0


# ---------------------------------------------------------------------------------------------------------------
# refusals and N == 0
# ---------------------------------------------------------------------------------------------------------------
REFUSED = [
    ("width-not-32", case("multi", 300, [P(48, 64), P(32, 64)]), {}),
    ("width-below-32", case("multi", 300, [P(16, 64)]), {}),
    ("over-256-columns", case("multi", 300, [P(128, 64), P(128, 64), P(32, 64)]), {}),
    ("nine-segments", case("multi", 300, [P(32, 64)] * 9), {}),
    ("wide-M2-not-4", case("multi", 300, [P(64, 130), P(64, 130)]), {}),
    ("wide-M2-operand-not-64", case("multi", 300, [P(32, 132)]), {}),
    ("pairs-M2-129", case("pairs", 300, [P(32, 64), P(16, 129)]), {}),
    ("pairs-over-256-rows", case("pairs", 300, [P(33, 8)] * 5), {}),
    ("pairs-nine", case("pairs", 300, [P(8, 8)] * 9), {}),
    ("multi-null-ws", case("multi", 300, [P(64, 64)]), dict(null_ws=True)),
    ("pairs-null-ws", case("pairs", 300, [P(32, 65), P(16, 32)]), dict(null_ws=True)),
    ("acc-null-ws", case("acc", 300, [P(33, 65)]), dict(null_ws=True)),
    ("lbw-null-ws", case("lbw", 300, [P(33, 65, ACT_RELU)]), dict(null_ws=True)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,c,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_return_an_error_and_write_nothing(dev, name, c, kw):
    run_case(dev, c, make_inputs(c), expect_rc=-1, ws_n=1 << 16, **kw)      # (the workspace is never reached)
    from dgg_amd import _lib
    assert _lib.lib().dgg_last_error().decode() != ""


@pytest.mark.gpu
@pytest.mark.parametrize("c", [case("acc", 64, [P(33, 65)]), case("lbw", 64, [P(33, 65, ACT_RELU)]), case("lbw", 64, [P(32, 64)], dx=True),
                               case("multi", 64, [P(64, 128, ACT_RELU), P(32, 128)]), case("pairs", 64, [P(32, 65), P(1, 16)])],
                         ids=lambda c: c["id"])
def test_zero_rows_succeed_and_write_nothing(dev, c):
    run_case(dev, c, make_inputs(c), N_call=0)


# ---------------------------------------------------------------------------------------------------------------
# tier 2
# ---------------------------------------------------------------------------------------------------------------
def real_case_figures(dev, c):
    """per product: dict of the CPU figure of the case's precision class, the bar, and the statistic measured on the GPU"""
    inp = make_inputs(c, real=True)
    got = run_case(dev, c, inp)
    rows = []
    for q, (p, d, (Cg, sg, dxg)) in enumerate(zip(c["prods"], inp, got)):
        Cr, sr = tn_reference(d["A"], d["Y"], p["act"], d["B"])
        Cf, sf = tn_fp32(d["A"], d["Y"], p["act"], d["B"])
        cpu = rel_max(Cf, Cr) if c["cls"] == "fp32" else rel_max(tn_split_bf16(d["A"], d["Y"], p["act"], d["B"]), Cr)
        absAB = np.abs(masked(d["A"], d["Y"], p["act"], np.float64)).T @ np.abs(d["B"]).astype(np.float64)
        row = dict(id=c["id"], q=q, cls=c["cls"], cpu=cpu, bar=4 * cpu, gpu=rel_max(Cg, Cr),
                   cw=float((np.abs(Cg - Cr) / np.where(absAB > 0, absAB, 1.0)).max()))
        if sg is not None:
            row.update(cs_cpu=rel_max(sf, sr), cs_bar=4 * rel_max(sf, sr), cs_gpu=rel_max(sg, sr))
        rows.append(row)
        print("TIER2 " + json.dumps(row))
    return rows, inp, got


@pytest.mark.gpu
@pytest.mark.parametrize("c", REAL, ids=[c["id"] for c in REAL])
def test_real_valued_product_within_four_times_the_cpu_restatement(dev, c):
    rows, _, _ = real_case_figures(dev, c)
    for r in rows:
        assert r["gpu"] <= r["bar"], "C of product %d: %.3g of max against a bar of %.3g (4 x the %s restatement on the CPU)" % (
            r["q"], r["gpu"], r["bar"], r["cls"])
        if "cs_gpu" in r:
            assert r["cs_gpu"] <= r["cs_bar"], "colsum of product %d: %.3g of max against a bar of %.3g" % (r["q"], r["cs_gpu"], r["cs_bar"])


@pytest.mark.gpu
def test_headline_gradient_accuracy_is_what_the_readme_records(dev):
    """N = 100 000, d = 128, three 64-wide operands through the split-bf16 wide kernel: README 'gradients 4e-6 of max'"""
    rows, _, _ = real_case_figures(dev, HEADLINE)
    worst = max(r["gpu"] for r in rows)
    print("HEADLINE worst %.3g of max (README: %.1g)" % (worst, README_GRAD_ERR))
    assert README_GRAD_ERR / 3 <= worst <= README_GRAD_ERR * 3
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "gradients 4e-6 of max" in f.read()


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,out,layout,act", [(1500, 40, 24, 0, 1), (300, 20, 12, 1, 2), (2100, 128, 64, 1, 2), (257, 1433, 64, 0, 1)])
def test_linear_bwd_dx_bit_exact(dev, N, d, out, layout, act):
    """dx of dgg_linear_bwd is the forward kernel on the transposed weight: the k-ordered fmaf chain over dp = dy * act'(y)"""
    from oracle import oracle as O
    c = case("lbw", N, [P(out, d, act, lay=layout)], dx=True)
    inp = make_inputs(c, real=True)
    (_, _, dx), = run_case(dev, c, inp)
    d0 = inp[0]
    dp = masked(d0["A"], d0["Y"], act, np.float32)
    W = d0["W"] if layout == 0 else np.ascontiguousarray(d0["W"].T)
    ref = O.linear(dp, W, None, ACT_NONE, 1 - layout)
    assert np.array_equal(dx, ref), "dx is not the k-ordered fmaf chain of dp and W (%d elements differ)" % int((dx != ref).sum())


if __name__ == "__main__":
    if "--knob-child" in sys.argv:
        sys.exit(_knob_child())
