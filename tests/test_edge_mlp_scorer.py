"""The edge-MLP scorer kernels of csrc/dgg_edgemlp.hip against exact and float64 references.

dgg_edge_mlp_fwd, dgg_edgelist_topk_p[_rows] and the five entry points of edge_mlp_bwd_kernel (dgg_edge_mlp_bwd with an ELL block or a
CSR pattern, _rows, _det, _partp, _partp_rows) are called through the C ABI.  The backward kernel also serves every edge-MLP scorer on
all-pairs candidates, so every training step of u-v-deg, u-v-deg-dist, u-v-A_uv, A_uv and edge_conv goes through it.

Graphs.  CSR candidates: build_graph of test_csr_adjacency.py at N = 270..273 and 1 (row lengths 0, 1, 2, 63, 64, 65, 127, 128, 129,
200, a hub column, a self loop, 1 to 4 live wavefronts in the last block).  ELL selections: build_block of test_partitioned_backward.py,
shapes `wave` (700 rows) and `shard` (1100 nodes, rows [300, 811)), PER = 8 (the UQ of edge_mlp_colsum): a hub every live row selects,
in-degrees 1, 7, 8, 9, 33, 127, 128, 129, both kinds of inactive entry, a dead row, a self loop, rows of 64, 63 and 33 active ranks;
K = 64 and the first 5 ranks of the same block.  `loop`: 4109 rows, K = 4, hw = 8 -- the smallest block at which the default 1024
workgroups take a second row (the last 13 rows).  Inputs sit between NaN guards, outputs are handed in NaN-filled (or holding a start
pattern) between canary words, every test checks that no input was written.

Tier 1, bit for bit
  forward against O.edge_mlp_fwd: hw in 1, 15, 16, 17, 48, 64, 256; ex_mode 0, 1, 2 (h in 1, 16, 128, 129, 192); with / without deg;
    act 0 / 1; E in 1, 255, 256, 257 and the graph's own; ex_out = NULL; AB 4 bytes past a 16-byte boundary (the scalar path).
  dgg_edgelist_topk_p / _rows against O.edgelist_topk_p (the oracle on the whole graph, sliced; eid rebased): values of rank_values,
    four noise modes (explicit G with ldG = N + 3 and NaN padding; the hashes keyed on the global pair at row0 != 0), K in 1, 7, 63, 64,
    rows outside the range untouched.
  backward sums exact by construction: AB = 0, b1 = 1, w2 = signed powers of two in cancelling pairs (hw = 1: w2 = 0), wdu = wdv = wex = 1,
    deg and ex integers in 0..2, b2 = 0, dval integers |.| <= 3, val in {1/2, 1, 2}.  Then z_o >= 1, s = 0, p = 1/2 exactly, ds = dp / 4
    and every term of every sum is a multiple of 1/4 with magnitudes far below 2^24 units: any summation order gives the same bits.
    test_exactness_premises_hold_for_every_case proves this per case on the CPU (O.edge_mlp_fwd returns exactly 0.5, the oracle's
    backward equals the integer reference).  Forms: ELL at hw in 1, 2, 4, 8, 16, 64, 128, 256; _rows on the shard (A halves outside the
    rows and dpar start at integer patterns, B halves of unlisted nodes stay +0.0); rowptr form (eid = NULL with and without dex, an
    explicit eid, whole 64/LPE batches of the 200-long row without cotangent); _det with workspaces of 1, 3 and 3 + 1/(5hw+2) rows and a
    cotangent pattern whose per-workgroup db2 sum is 2^24 + 1 (needs the low word); _partp / _partp_rows with dz_rows = the record
    count, half of it, and 1, recorded entries without cotangent, and the contract case: a partition rebuilt in the same workspace with
    w = 0 on entries that keep a cotangent.  DGG_EMLP_GRID = 2 and 5 each in one fresh child process.
  refusals and empties return their documented code and write nothing.

Tier 2, float64.  Reference: restate_edge_mlp_bwd(np.float64, ...), the oracle's formula in numpy (held to O.edge_mlp_bwd and
O.edge_mlp_bwd_csr on the CPU).  p_edge, ex, idx, val, eid come from the oracle's forward and feed both sides: the excluded share is
0.  Statistic: max|got - ref| / max|ref| for the two halves of dAB, dex and the five hw-blocks of dpar; for db2, one cancelling sum,
the denominator is sum |ds_e|.  Bar: 4 x the larger error of the same arithmetic in float32 on the CPU (fma chain, ora_exp, 1e-8f;
db2 in double from the entry to its workgroup's sum, then float32 across the workgroups as the atomics add them, det: double
throughout; fmaf is emulated through one double product and sum) in row order and in a seeded shuffle -- and, for the sums that the
GPU adds by float atomics in another order every run (dB, the blocks of dpar, db2), in NDRAW = 32 further seeded orders of the same
per-entry float32 terms (further_orders), because where one number decides the statistic two draws are a noisy bar.  Forms
and shapes go together (atomic / partp: wave, rows / partp_rows: shard, det: the N = 270 CSR pattern); within every form hw, act,
perturb, the ex mode and deg take each of their values (hw = 2 is refused by the partp form).  One more case runs the atomic form on
the CSR pattern (rows of up to 200 entries in batches, dex that is not zero).

Each of these changes to the kernels, made in a scratch copy and run on an MI355X, fails these tier-1 tests and no other tier-1 test:
  1. no second trip of the row loop (`i += gridDim.x * 4`)   test_default_dispatch_takes_a_second_row, test_det_backward_is_the_integer_
                                                                reference[one-row, three-rows, three-rows-and-a-float], test_emlp_grid_knob_*
  2. no clamp of p1 in edge_mlp_colsum                          test_partp_backward_is_the_integer_reference[4, 16, 64, 256] (dz_rows = half of
                                                                the records and 1: NaN rows of dz_rec reach dAB), test_emlp_grid_knob_*
  3. edge_mlp_parsum without db2's low word                     test_det_backward_is_the_integer_reference[three-rows, three-rows-and-a-float,
                                                                every-workgroup] (the low-word pattern; one workgroup has nothing to carry)
  4. `r < K` for the CSR dex zero-fill                          test_csr_backward_is_the_integer_reference[every N] and the CSR cases of
                                                                test_det_backward_is_the_integer_reference (dex of skipped batches stays NaN)
  5. no `(AB & 15) == 0` test in the forward                    argued from the code, not run: the 16-byte loads would go to addresses that
     are 4 mod 16, a misaligned vector access that the memory system may split or refuse; test_forward_equals_the_oracle[16] and [64] hand
     AB in at such an address and hold p_edge and ex_out to the oracle's bits, which today only the scalar path can give there.
  The contract case: before the kernel looked at the weight, test_partp_entry_without_a_record_takes_the_atomics[4, 16, 64, 256] failed
  (wave hw = 256: 121 056 of 358 400 elements of dAB differed, B halves of nodes nobody lists were written).

Measured on an MI355X (err / max|ref| per output, db2: err / sum|ds|; the bar is computed in the test from the three CPU columns,
nothing is fixed here).  Case = form shape hw act perturb ex-mode deg.  `CPU more`: the largest error of the 32 further seeded orders
(further_orders; only the sums the GPU adds by float atomics have them).  A block of dpar that the case does not feed (dwdu / dwdv
without deg) is zero on every side.  The float atomics land in another order every run, so the figures of dB, dpar and db2 move from
run to run; with the bar taken from row order and the shuffle alone, two figures of 1944 over twelve runs came out above it (db2 of
partp_rows shard hw=64 at 1.36 x, dB of rows shard hw=2 at 1.11 x: one number decides either), which is why the further orders are
there.  With them, thirteen runs of the 19 cases (2223 figures) were all under their bars; the largest figure / bar seen was
dB 0.53, dwex 0.14, db1 0.11, dw2 0.13, db2 0.42 in the atomic forms, and db2 0.79 in the det form (hw = 16), which adds in a fixed order
and gives that same figure every run.  The 96 GPU tests of this module take 12 s, the 4 CPU tests 2 s.

  output                                                           CPU row   CPU shuf   CPU more   bar = 4x     MI355X
  bwd wave hw=2 a0 p0 ex1 deg1 dA                                 2.91e-07   1.30e-07   0.00e+00   1.17e-06   1.31e-07
  bwd wave hw=2 a0 p0 ex1 deg1 dB                                 3.75e-07   2.57e-07   1.30e-06   5.19e-06   3.05e-07
  bwd wave hw=2 a0 p0 ex1 deg1 dex                                1.51e-07   1.51e-07   0.00e+00   6.04e-07   1.51e-07
  bwd wave hw=2 a0 p0 ex1 deg1 dwdu                               2.70e-06   8.90e-07   5.04e-06   2.01e-05   4.49e-07
  bwd wave hw=2 a0 p0 ex1 deg1 dwdv                               2.06e-06   9.64e-07   3.93e-06   1.57e-05   2.38e-07
  bwd wave hw=2 a0 p0 ex1 deg1 dwex                               1.16e-05   2.07e-05   9.26e-05   3.70e-04   2.67e-06
  bwd wave hw=2 a0 p0 ex1 deg1 db1                                3.17e-06   1.28e-06   4.74e-06   1.90e-05   9.01e-07
  bwd wave hw=2 a0 p0 ex1 deg1 dw2                                3.73e-06   1.68e-06   9.84e-06   3.94e-05   3.09e-07
  bwd wave hw=2 a0 p0 ex1 deg1 db2                                3.18e-11   3.67e-09   6.62e-09   2.65e-08   1.04e-08
  bwd wave hw=16 a1 p1 ex2 deg0 dA                                2.11e-07   1.19e-07   0.00e+00   8.44e-07   1.16e-07
  bwd wave hw=16 a1 p1 ex2 deg0 dB                                6.91e-07   3.76e-07   9.72e-07   3.89e-06   9.25e-07
  bwd wave hw=16 a1 p1 ex2 deg0 dex                               1.10e-07   1.10e-07   0.00e+00   4.39e-07   1.08e-07
  bwd wave hw=16 a1 p1 ex2 deg0 dwdu                              0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  bwd wave hw=16 a1 p1 ex2 deg0 dwdv                              0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  bwd wave hw=16 a1 p1 ex2 deg0 dwex                              2.05e-06   1.04e-06   6.69e-06   2.67e-05   3.46e-07
  bwd wave hw=16 a1 p1 ex2 deg0 db1                               3.81e-06   1.60e-06   6.56e-06   2.63e-05   5.21e-07
  bwd wave hw=16 a1 p1 ex2 deg0 dw2                               1.19e-06   1.76e-06   3.86e-06   1.54e-05   1.83e-07
  bwd wave hw=16 a1 p1 ex2 deg0 db2                               8.48e-11   1.28e-09   1.45e-08   5.79e-08   1.12e-09
  bwd wave hw=64 a1 p0 ex2 deg1 dA                                2.90e-07   2.74e-07   0.00e+00   1.16e-06   1.33e-07
  bwd wave hw=64 a1 p0 ex2 deg1 dB                                2.47e-07   1.90e-07   4.98e-07   1.99e-06   3.65e-07
  bwd wave hw=64 a1 p0 ex2 deg1 dex                               2.98e-07   2.98e-07   0.00e+00   1.19e-06   2.36e-07
  bwd wave hw=64 a1 p0 ex2 deg1 dwdu                              1.45e-06   1.03e-06   4.36e-06   1.74e-05   3.50e-07
  bwd wave hw=64 a1 p0 ex2 deg1 dwdv                              1.24e-06   1.56e-06   5.22e-06   2.09e-05   3.86e-07
  bwd wave hw=64 a1 p0 ex2 deg1 dwex                              1.10e-06   3.02e-06   4.25e-06   1.70e-05   3.11e-07
  bwd wave hw=64 a1 p0 ex2 deg1 db1                               1.33e-06   1.39e-06   3.30e-06   1.32e-05   6.24e-07
  bwd wave hw=64 a1 p0 ex2 deg1 dw2                               1.99e-06   2.00e-06   3.14e-06   1.26e-05   4.08e-07
  bwd wave hw=64 a1 p0 ex2 deg1 db2                               1.30e-09   3.36e-09   1.73e-08   6.93e-08   5.69e-09
  bwd wave hw=256 a0 p1 ex1 deg0 dA                               7.51e-07   7.61e-07   0.00e+00   3.05e-06   5.03e-07
  bwd wave hw=256 a0 p1 ex1 deg0 dB                               2.25e-06   2.03e-06   8.62e-07   9.02e-06   1.07e-06
  bwd wave hw=256 a0 p1 ex1 deg0 dex                              1.42e-06   1.42e-06   0.00e+00   5.70e-06   6.16e-07
  bwd wave hw=256 a0 p1 ex1 deg0 dwdu                             0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  bwd wave hw=256 a0 p1 ex1 deg0 dwdv                             0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  bwd wave hw=256 a0 p1 ex1 deg0 dwex                             2.96e-06   1.95e-06   1.18e-06   1.19e-05   4.43e-07
  bwd wave hw=256 a0 p1 ex1 deg0 db1                              1.75e-06   1.96e-06   1.34e-06   7.86e-06   3.45e-07
  bwd wave hw=256 a0 p1 ex1 deg0 dw2                              1.93e-06   2.14e-06   3.17e-06   1.27e-05   3.15e-07
  bwd wave hw=256 a0 p1 ex1 deg0 db2                              3.53e-08   3.16e-08   4.63e-08   1.85e-07   8.72e-09
  rows shard hw=2 a0 p0 ex1 deg1 dA                               1.13e-07   1.02e-07   0.00e+00   4.51e-07   8.73e-08
  rows shard hw=2 a0 p0 ex1 deg1 dB                               1.52e-07   1.02e-07   8.93e-07   3.57e-06   2.92e-07
  rows shard hw=2 a0 p0 ex1 deg1 dex                              3.62e-07   3.62e-07   0.00e+00   1.45e-06   3.18e-07
  rows shard hw=2 a0 p0 ex1 deg1 dwdu                             8.83e-08   8.82e-07   3.24e-06   1.30e-05   3.26e-07
  rows shard hw=2 a0 p0 ex1 deg1 dwdv                             5.21e-07   5.71e-07   6.28e-06   2.51e-05   7.48e-08
  rows shard hw=2 a0 p0 ex1 deg1 dwex                             2.79e-07   2.29e-07   2.40e-06   9.60e-06   1.10e-07
  rows shard hw=2 a0 p0 ex1 deg1 db1                              1.09e-06   1.81e-07   4.14e-06   1.66e-05   1.61e-07
  rows shard hw=2 a0 p0 ex1 deg1 dw2                              8.77e-06   2.38e-06   1.16e-05   4.65e-05   5.71e-07
  rows shard hw=2 a0 p0 ex1 deg1 db2                              1.09e-09   4.58e-09   1.24e-08   4.98e-08   2.69e-09
  rows shard hw=16 a1 p1 ex2 deg0 dA                              1.70e-07   1.55e-07   0.00e+00   6.81e-07   9.20e-08
  rows shard hw=16 a1 p1 ex2 deg0 dB                              4.36e-07   3.48e-07   7.67e-07   3.07e-06   2.44e-07
  rows shard hw=16 a1 p1 ex2 deg0 dex                             6.08e-08   6.08e-08   0.00e+00   2.43e-07   7.49e-08
  rows shard hw=16 a1 p1 ex2 deg0 dwdu                            0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  rows shard hw=16 a1 p1 ex2 deg0 dwdv                            0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  rows shard hw=16 a1 p1 ex2 deg0 dwex                            1.56e-06   9.38e-07   2.82e-06   1.13e-05   2.36e-07
  rows shard hw=16 a1 p1 ex2 deg0 db1                             1.41e-06   1.70e-06   4.63e-06   1.85e-05   1.49e-07
  rows shard hw=16 a1 p1 ex2 deg0 dw2                             1.38e-06   1.37e-06   2.92e-06   1.17e-05   2.13e-07
  rows shard hw=16 a1 p1 ex2 deg0 db2                             1.15e-09   3.04e-09   7.94e-09   3.17e-08   1.86e-09
  rows shard hw=64 a1 p0 ex2 deg1 dA                              3.69e-07   6.07e-07   0.00e+00   2.43e-06   3.06e-07
  rows shard hw=64 a1 p0 ex2 deg1 dB                              7.55e-07   5.70e-07   3.68e-07   3.02e-06   3.43e-07
  rows shard hw=64 a1 p0 ex2 deg1 dex                             6.33e-07   6.33e-07   0.00e+00   2.53e-06   3.85e-07
  rows shard hw=64 a1 p0 ex2 deg1 dwdu                            1.56e-06   6.94e-07   2.58e-06   1.03e-05   5.51e-07
  rows shard hw=64 a1 p0 ex2 deg1 dwdv                            1.53e-06   1.82e-06   3.42e-06   1.37e-05   2.06e-06
  rows shard hw=64 a1 p0 ex2 deg1 dwex                            1.94e-06   8.08e-07   2.14e-06   8.54e-06   6.98e-07
  rows shard hw=64 a1 p0 ex2 deg1 db1                             1.86e-06   1.44e-06   3.03e-06   1.21e-05   5.22e-07
  rows shard hw=64 a1 p0 ex2 deg1 dw2                             1.01e-06   1.79e-06   1.52e-06   7.17e-06   9.03e-07
  rows shard hw=64 a1 p0 ex2 deg1 db2                             7.48e-09   3.47e-09   1.75e-08   7.00e-08   1.95e-08
  rows shard hw=256 a0 p1 ex1 deg0 dA                             4.52e-07   4.43e-07   0.00e+00   1.81e-06   2.83e-07
  rows shard hw=256 a0 p1 ex1 deg0 dB                             5.58e-07   4.60e-07   8.34e-07   3.34e-06   7.11e-07
  rows shard hw=256 a0 p1 ex1 deg0 dex                            6.02e-07   6.02e-07   0.00e+00   2.41e-06   2.76e-07
  rows shard hw=256 a0 p1 ex1 deg0 dwdu                           0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  rows shard hw=256 a0 p1 ex1 deg0 dwdv                           0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  rows shard hw=256 a0 p1 ex1 deg0 dwex                           1.11e-06   1.56e-06   1.72e-06   6.87e-06   6.53e-07
  rows shard hw=256 a0 p1 ex1 deg0 db1                            2.61e-06   1.81e-06   1.64e-06   1.05e-05   5.99e-07
  rows shard hw=256 a0 p1 ex1 deg0 dw2                            1.96e-06   1.43e-06   3.86e-06   1.55e-05   6.13e-07
  rows shard hw=256 a0 p1 ex1 deg0 db2                            1.26e-08   1.26e-08   1.74e-08   6.95e-08   1.59e-08
  det csr270 hw=2 a0 p0 ex1 deg1 dA                               5.63e-07   2.82e-07   0.00e+00   2.25e-06   2.95e-08
  det csr270 hw=2 a0 p0 ex1 deg1 dB                               1.80e-07   1.74e-07   7.35e-07   2.94e-06   6.14e-07
  det csr270 hw=2 a0 p0 ex1 deg1 dex                              1.30e-07   1.30e-07   0.00e+00   5.19e-07   1.18e-07
  det csr270 hw=2 a0 p0 ex1 deg1 dwdu                             3.61e-05   1.83e-05   7.56e-05   3.03e-04   2.33e-06
  det csr270 hw=2 a0 p0 ex1 deg1 dwdv                             1.93e-06   3.90e-07   5.63e-06   2.25e-05   8.29e-07
  det csr270 hw=2 a0 p0 ex1 deg1 dwex                             1.45e-06   4.27e-07   9.57e-06   3.83e-05   4.06e-07
  det csr270 hw=2 a0 p0 ex1 deg1 db1                              6.79e-06   2.80e-06   1.51e-05   6.04e-05   2.62e-07
  det csr270 hw=2 a0 p0 ex1 deg1 dw2                              2.89e-06   2.22e-06   2.09e-06   1.15e-05   8.49e-08
  det csr270 hw=2 a0 p0 ex1 deg1 db2                              8.38e-10   8.38e-10   0.00e+00   3.35e-09   1.25e-09
  det csr270 hw=16 a1 p1 ex2 deg0 dA                              3.14e-07   5.53e-07   0.00e+00   2.21e-06   1.59e-07
  det csr270 hw=16 a1 p1 ex2 deg0 dB                              4.17e-07   2.60e-07   5.90e-07   2.36e-06   2.47e-07
  det csr270 hw=16 a1 p1 ex2 deg0 dex                             1.04e-07   1.04e-07   0.00e+00   4.16e-07   7.27e-08
  det csr270 hw=16 a1 p1 ex2 deg0 dwdu                            0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  det csr270 hw=16 a1 p1 ex2 deg0 dwdv                            0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  det csr270 hw=16 a1 p1 ex2 deg0 dwex                            1.79e-06   1.39e-06   7.05e-06   2.82e-05   2.61e-07
  det csr270 hw=16 a1 p1 ex2 deg0 db1                             1.45e-06   1.04e-06   3.19e-06   1.28e-05   8.05e-08
  det csr270 hw=16 a1 p1 ex2 deg0 dw2                             1.14e-06   5.59e-07   3.83e-06   1.53e-05   1.76e-07
  det csr270 hw=16 a1 p1 ex2 deg0 db2                             8.13e-10   8.13e-10   0.00e+00   3.25e-09   2.58e-09
  det csr270 hw=64 a1 p0 ex2 deg1 dA                              4.30e-07   2.65e-07   0.00e+00   1.72e-06   2.75e-07
  det csr270 hw=64 a1 p0 ex2 deg1 dB                              3.97e-07   3.41e-07   2.03e-07   1.59e-06   4.19e-07
  det csr270 hw=64 a1 p0 ex2 deg1 dex                             3.07e-07   3.07e-07   0.00e+00   1.23e-06   3.30e-07
  det csr270 hw=64 a1 p0 ex2 deg1 dwdu                            9.14e-07   1.14e-06   1.08e-06   4.57e-06   1.55e-07
  det csr270 hw=64 a1 p0 ex2 deg1 dwdv                            1.34e-06   1.47e-06   2.00e-06   8.02e-06   5.14e-07
  det csr270 hw=64 a1 p0 ex2 deg1 dwex                            2.43e-06   2.41e-06   1.51e-06   9.71e-06   2.47e-07
  det csr270 hw=64 a1 p0 ex2 deg1 db1                             1.64e-06   2.09e-06   2.73e-06   1.09e-05   4.80e-07
  det csr270 hw=64 a1 p0 ex2 deg1 dw2                             3.37e-06   2.35e-06   5.00e-06   2.00e-05   7.32e-07
  det csr270 hw=64 a1 p0 ex2 deg1 db2                             1.45e-08   1.45e-08   0.00e+00   5.79e-08   6.90e-09
  det csr270 hw=256 a0 p1 ex1 deg0 dA                             5.32e-07   4.73e-07   0.00e+00   2.13e-06   3.84e-07
  det csr270 hw=256 a0 p1 ex1 deg0 dB                             5.88e-07   6.09e-07   2.62e-07   2.44e-06   2.94e-07
  det csr270 hw=256 a0 p1 ex1 deg0 dex                            8.40e-07   8.40e-07   0.00e+00   3.36e-06   2.77e-07
  det csr270 hw=256 a0 p1 ex1 deg0 dwdu                           0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  det csr270 hw=256 a0 p1 ex1 deg0 dwdv                           0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  det csr270 hw=256 a0 p1 ex1 deg0 dwex                           5.55e-06   2.11e-06   2.37e-06   2.22e-05   5.46e-07
  det csr270 hw=256 a0 p1 ex1 deg0 db1                            7.80e-06   7.65e-06   5.20e-06   3.12e-05   1.29e-06
  det csr270 hw=256 a0 p1 ex1 deg0 dw2                            1.82e-06   2.23e-06   2.23e-06   8.91e-06   5.12e-07
  det csr270 hw=256 a0 p1 ex1 deg0 db2                            2.82e-08   2.82e-08   0.00e+00   1.13e-07   3.56e-09
  partp wave hw=16 a1 p0 ex2 deg1 dA                              1.99e-07   1.73e-07   0.00e+00   7.97e-07   1.73e-07
  partp wave hw=16 a1 p0 ex2 deg1 dB                              2.95e-07   5.54e-07   1.03e-06   4.14e-06   3.23e-07
  partp wave hw=16 a1 p0 ex2 deg1 dex                             1.95e-07   1.95e-07   0.00e+00   7.78e-07   2.47e-07
  partp wave hw=16 a1 p0 ex2 deg1 dwdu                            8.71e-07   1.95e-06   2.75e-06   1.10e-05   3.37e-07
  partp wave hw=16 a1 p0 ex2 deg1 dwdv                            3.79e-06   1.32e-06   6.82e-06   2.73e-05   2.53e-07
  partp wave hw=16 a1 p0 ex2 deg1 dwex                            6.42e-07   3.44e-06   3.05e-06   1.38e-05   2.64e-07
  partp wave hw=16 a1 p0 ex2 deg1 db1                             2.14e-06   1.27e-06   3.77e-06   1.51e-05   2.39e-07
  partp wave hw=16 a1 p0 ex2 deg1 dw2                             4.56e-06   4.51e-06   6.49e-06   2.60e-05   1.54e-07
  partp wave hw=16 a1 p0 ex2 deg1 db2                             2.57e-09   5.22e-09   2.08e-08   8.32e-08   3.28e-09
  partp wave hw=64 a0 p1 ex1 deg0 dA                              3.02e-07   2.82e-07   0.00e+00   1.21e-06   2.82e-07
  partp wave hw=64 a0 p1 ex1 deg0 dB                              3.71e-07   3.23e-07   3.89e-07   1.56e-06   3.57e-07
  partp wave hw=64 a0 p1 ex1 deg0 dex                             5.01e-07   5.01e-07   0.00e+00   2.00e-06   5.01e-07
  partp wave hw=64 a0 p1 ex1 deg0 dwdu                            0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  partp wave hw=64 a0 p1 ex1 deg0 dwdv                            0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  partp wave hw=64 a0 p1 ex1 deg0 dwex                            1.02e-06   7.78e-07   1.40e-06   5.61e-06   3.65e-07
  partp wave hw=64 a0 p1 ex1 deg0 db1                             1.77e-06   1.22e-06   1.16e-06   7.09e-06   3.97e-07
  partp wave hw=64 a0 p1 ex1 deg0 dw2                             1.69e-06   1.04e-06   2.46e-06   9.83e-06   4.45e-07
  partp wave hw=64 a0 p1 ex1 deg0 db2                             4.89e-09   1.14e-08   2.93e-08   1.17e-07   3.26e-09
  partp wave hw=256 a0 p0 ex1 deg1 dA                             8.21e-07   8.25e-07   0.00e+00   3.30e-06   4.64e-07
  partp wave hw=256 a0 p0 ex1 deg1 dB                             1.64e-06   1.68e-06   9.27e-07   6.74e-06   7.97e-07
  partp wave hw=256 a0 p0 ex1 deg1 dex                            2.07e-06   2.07e-06   0.00e+00   8.29e-06   9.17e-07
  partp wave hw=256 a0 p0 ex1 deg1 dwdu                           4.22e-06   6.29e-06   2.97e-06   2.52e-05   1.21e-06
  partp wave hw=256 a0 p0 ex1 deg1 dwdv                           1.96e-06   2.64e-06   1.61e-06   1.06e-05   3.81e-07
  partp wave hw=256 a0 p0 ex1 deg1 dwex                           2.48e-06   1.67e-06   1.48e-06   9.91e-06   6.33e-07
  partp wave hw=256 a0 p0 ex1 deg1 db1                            2.31e-06   2.07e-06   1.64e-06   9.22e-06   2.91e-07
  partp wave hw=256 a0 p0 ex1 deg1 dw2                            2.49e-06   2.64e-06   2.79e-06   1.12e-05   4.06e-07
  partp wave hw=256 a0 p0 ex1 deg1 db2                            8.46e-09   8.46e-09   2.52e-08   1.01e-07   4.07e-09
  partp_rows shard hw=16 a1 p0 ex2 deg1 dA                        1.01e-07   8.00e-08   0.00e+00   4.02e-07   9.66e-08
  partp_rows shard hw=16 a1 p0 ex2 deg1 dB                        1.54e-07   1.12e-07   4.36e-07   1.75e-06   2.53e-07
  partp_rows shard hw=16 a1 p0 ex2 deg1 dex                       1.41e-07   1.41e-07   0.00e+00   5.62e-07   1.50e-07
  partp_rows shard hw=16 a1 p0 ex2 deg1 dwdu                      2.84e-07   9.67e-07   1.83e-06   7.32e-06   2.10e-07
  partp_rows shard hw=16 a1 p0 ex2 deg1 dwdv                      3.56e-07   3.56e-07   1.23e-06   4.91e-06   1.38e-07
  partp_rows shard hw=16 a1 p0 ex2 deg1 dwex                      1.09e-06   1.80e-06   3.00e-06   1.20e-05   3.59e-07
  partp_rows shard hw=16 a1 p0 ex2 deg1 db1                       3.39e-07   9.93e-07   2.73e-06   1.09e-05   5.71e-07
  partp_rows shard hw=16 a1 p0 ex2 deg1 dw2                       1.41e-06   3.86e-07   3.29e-06   1.32e-05   1.62e-07
  partp_rows shard hw=16 a1 p0 ex2 deg1 db2                       4.75e-09   4.75e-09   1.19e-08   4.75e-08   2.96e-09
  partp_rows shard hw=64 a0 p1 ex1 deg0 dA                        2.76e-07   2.64e-07   0.00e+00   1.11e-06   1.46e-07
  partp_rows shard hw=64 a0 p1 ex1 deg0 dB                        3.52e-07   2.83e-07   2.60e-07   1.41e-06   3.21e-07
  partp_rows shard hw=64 a0 p1 ex1 deg0 dex                       1.03e-06   1.03e-06   0.00e+00   4.11e-06   4.12e-07
  partp_rows shard hw=64 a0 p1 ex1 deg0 dwdu                      0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  partp_rows shard hw=64 a0 p1 ex1 deg0 dwdv                      0.00e+00   0.00e+00   0.00e+00   0.00e+00   0.00e+00
  partp_rows shard hw=64 a0 p1 ex1 deg0 dwex                      1.97e-06   3.01e-06   3.85e-06   1.54e-05   2.01e-06
  partp_rows shard hw=64 a0 p1 ex1 deg0 db1                       1.25e-06   8.84e-07   1.80e-06   7.19e-06   4.80e-07
  partp_rows shard hw=64 a0 p1 ex1 deg0 dw2                       8.96e-07   8.21e-07   1.88e-06   7.50e-06   3.69e-07
  partp_rows shard hw=64 a0 p1 ex1 deg0 db2                       1.12e-09   4.24e-09   1.50e-08   5.99e-08   6.92e-09
  partp_rows shard hw=256 a0 p0 ex1 deg1 dA                       6.61e-07   6.77e-07   0.00e+00   2.71e-06   5.37e-07
  partp_rows shard hw=256 a0 p0 ex1 deg1 dB                       1.23e-06   1.07e-06   1.10e-06   4.92e-06   4.67e-07
  partp_rows shard hw=256 a0 p0 ex1 deg1 dex                      9.00e-07   9.00e-07   0.00e+00   3.60e-06   6.73e-07
  partp_rows shard hw=256 a0 p0 ex1 deg1 dwdu                     3.82e-06   2.59e-06   3.56e-06   1.53e-05   1.00e-06
  partp_rows shard hw=256 a0 p0 ex1 deg1 dwdv                     2.79e-06   2.35e-06   3.26e-06   1.30e-05   8.72e-07
  partp_rows shard hw=256 a0 p0 ex1 deg1 dwex                     3.52e-06   2.92e-06   5.94e-06   2.38e-05   1.12e-06
  partp_rows shard hw=256 a0 p0 ex1 deg1 db1                      3.24e-06   2.32e-06   3.56e-06   1.43e-05   8.58e-07
  partp_rows shard hw=256 a0 p0 ex1 deg1 dw2                      2.00e-06   2.33e-06   2.82e-06   1.13e-05   5.93e-07
  partp_rows shard hw=256 a0 p0 ex1 deg1 db2                      5.84e-08   3.86e-08   5.84e-08   2.33e-07   1.89e-08
  bwd csr270 hw=64 a1 p1 ex2 deg1 dA                              2.33e-07   2.91e-07   0.00e+00   1.17e-06   8.72e-08
  bwd csr270 hw=64 a1 p1 ex2 deg1 dB                              2.64e-07   2.49e-07   9.96e-07   3.98e-06   2.17e-07
  bwd csr270 hw=64 a1 p1 ex2 deg1 dex                             3.09e-07   3.09e-07   0.00e+00   1.24e-06   2.19e-07
  bwd csr270 hw=64 a1 p1 ex2 deg1 dwdu                            2.46e-06   1.03e-06   1.54e-06   9.86e-06   1.28e-07
  bwd csr270 hw=64 a1 p1 ex2 deg1 dwdv                            2.50e-06   1.01e-06   2.22e-06   9.99e-06   4.90e-07
  bwd csr270 hw=64 a1 p1 ex2 deg1 dwex                            1.64e-06   3.25e-06   3.97e-06   1.59e-05   1.92e-07
  bwd csr270 hw=64 a1 p1 ex2 deg1 db1                             1.62e-06   1.34e-06   4.71e-06   1.88e-05   2.04e-07
  bwd csr270 hw=64 a1 p1 ex2 deg1 dw2                             2.62e-06   1.55e-06   2.32e-06   1.05e-05   1.69e-07
  bwd csr270 hw=64 a1 p1 ex2 deg1 db2                             6.99e-09   3.01e-10   8.11e-09   3.24e-08   8.15e-10
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_csr_adjacency import (EPS, ERR_ARG, ERR_UNSUPPORTED, EXACT_LIMIT, F32, IFILL, LEAKY, ints, LENGTHS, N0, SIZES, Ctx, build_graph, check_graph, expect, figures, hold, orders, rank_values, same, seg,
                                seg_sum, untouched, vec)
from test_partitioned_backward import SHAPES, build_block, check_profile, nans, rel_max   # (Guard / CANARY: through Ctx)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = 8                                       # UQ of edge_mlp_colsum: the walk length whose neighbours get named in-degrees
F8 = np.float64
I8 = np.int64
FWD_HW = (1, 15, 16, 17, 48, 64, 256)
FWD_H = (1, 16, 128, 129, 192)
FWD_E = (1, 255, 256, 257)
TOPK_K = (1, 7, 63, 64)
BWD_HW = (1, 2, 4, 8, 16, 64, 128, 256)
PARTP_HW = (4, 16, 64, 256)
T2_HW = (2, 16, 64, 256)
NDRAW = 32                                    # further seeded orders of the float32 restatement for the sums the GPU adds by atomics
HEAVY = 64                                    # ... of dB: the nodes that at least this many entries list
NUNIT = 16                                    # ... of dB and the blocks of dpar: the first hidden units (wider blocks are a maximum over many)
LOOP = dict(ncols=4109, row0=0, rows=4109)
TINY = dict(ncols=50, row0=0, rows=50)          # CPU premises only
SEED = (4321, 99)
GRID_KNOBS = (2, 5)


# ---------------------------------------------------------------------------------------------------------------
# selections
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ell_block(shape, K):
    """-> idx int32 [rows, K], act bool [rows, K], info, shape dict"""
    if shape in ("loop", "tiny"):
        sh = LOOP if shape == "loop" else TINY
        n = sh["rows"]
        rng = np.random.default_rng(n)
        idx = rng.integers(0, n, (n, K)).astype(np.int32)
        idx[:, 0] = 17                                                  # a hub
        idx[rng.random((n, K)) < 0.1] = -1
        idx[n - 13:, 1] = np.arange(13, dtype=np.int32) + 20            # every second-trip row has a live entry of its own
        return idx, idx >= 0, dict(hub=17), sh
    sh = SHAPES[shape]
    rows = sh["rows"]
    rng = np.random.default_rng(40 + rows)
    cap = rng.integers(3, 13, rows)
    cap[[5, 6, 7, rows - 1]] = (64, 63, 33, 64)
    idx, act, info = build_block(sh, PER, cap, seed=3)
    assert idx.shape == (rows, 64)
    return np.ascontiguousarray(idx[:, :K]), np.ascontiguousarray(act[:, :K]), info, sh


def second_trip_rows(rows, gmax=1024):
    grid = min((rows + 3) // 4, gmax)
    return max(0, rows - 4 * grid)


def test_selections_have_every_prescribed_row_length_and_in_degree():
    for N in SIZES:
        check_graph(build_graph(N, False))
    g = build_graph(N0, False)
    cnt = np.diff(g["rowptr"])
    assert all(cnt[g["named"][L]] == L for L in LENGTHS) and len(g["unlisted"]) == 2
    for shape in ("wave", "shard"):
        idx, act, info, sh = ell_block(shape, 64)
        check_profile(sh, idx, act, info, PER)
        assert set(info["degs"]) == {1, 7, 8, 9, 33, 127, 128, 129}
        assert {64, 63, 33} <= set(act.sum(1).tolist())
        i5, a5, _, _ = ell_block(shape, 5)
        assert i5.shape == (sh["rows"], 5) and np.array_equal(i5, idx[:, :5]) and ((i5 >= 0) & ~a5).any() and (i5 < 0).any()
    assert SHAPES["wave"]["row0"] == 0 and SHAPES["shard"] == dict(ncols=1100, row0=300, rows=511)
    idx, _, _, sh = ell_block("loop", 4)
    assert second_trip_rows(4109) == 13 and second_trip_rows(4108) == 12 and second_trip_rows(4096) == 0
    assert (idx[-13:] >= 0).any(1).all()
    # ... and the profile check notices a hub that lost a row
    idx, act, info, sh = ell_block("wave", 64)
    broken = act.copy()
    broken[0, np.flatnonzero(idx[0] == info["hub"])[0]] = False
    with pytest.raises(AssertionError):
        check_profile(sh, idx, broken, info, PER)


# ---------------------------------------------------------------------------------------------------------------
# one description of a backward call: x (host arrays) -> flat entries -> references
# ---------------------------------------------------------------------------------------------------------------
def flat(x, use_ex=True):
    """the entries (idx >= 0) of a case in row order: u (node of the row), j, pos (slot in dex), g, val, exv"""
    if x["rowptr"] is not None:
        g = x["graph"]
        E = g["E"]
        exv = x["ex"][:E] if use_ex else None
        return dict(u=g["erow"].astype(I8), j=x["idx"].astype(I8), pos=np.arange(E), g=x["dval"], val=x["val"], exv=exv, nslot=E)
    m = x["idx"] >= 0
    r, c_ = np.nonzero(m)
    exv = x["ex"][x["eid"][m]] if use_ex else None
    return dict(u=x["row0"] + r.astype(I8), j=x["idx"][m].astype(I8), pos=r * x["K"] + c_, g=x["dval"][m], val=x["val"][m], exv=exv, nslot=x["idx"].size)


def exact_params(hw):
    rng = np.random.default_rng(70 + hw)
    w2 = np.zeros(hw, F32)
    for q in range(hw // 2):
        w2[2 * q] = rng.choice([1.0, 2.0]) * rng.choice([-1.0, 1.0])
        w2[2 * q + 1] = -w2[2 * q]
    one = np.ones(hw, F32)
    return dict(wdu=one, wdv=one.copy(), wex=one.copy(), b1=one.copy(), w2=w2, b2=np.zeros(1, F32))


@functools.lru_cache(maxsize=None)
def exact_case(shape, K, hw):
    """shape: wave / shard / loop (ELL, K ranks) or csrN (the CSR pattern of build_graph(N, unlisted form))"""
    rng = np.random.default_rng(1000 + 17 * hw + K + sum(map(ord, shape)))
    x = dict(shape=shape, hw=hw, P=exact_params(hw))
    if shape.startswith("csr"):
        N = int(shape[3:])
        g = build_graph(N, False)
        E = g["E"]
        x.update(graph=g, ncols=N, row0=0, rows=N, K=7, rowptr=g["rowptr"], idx=g["col"], eid=None)
        dval = ints(rng, E) * (rng.random(E) < 0.85)
        if N > 1:                                                       # whole batches of the 200-long row without a cotangent
            a, b = seg(g, 200)
            epi = 64 // (hw // (4 if hw % 4 == 0 else 1))
            dval[a + epi:min(a + 2 * epi, b)] = 0.0
            dval[a + (199 // epi) * epi:b] = 0.0
            if hw == 256:
                dval[a + 2:a + 9] = 0.0
            x["skipped"] = np.flatnonzero(dval[a:b] == 0) + a
        perm = rng.permutation(E).astype(np.int32)                      # an explicit eid: ex_perm[eid[e]] == ex[e]
        ex = rng.integers(0, 3, E).astype(F32)
        exp_ = np.empty(E, F32)
        exp_[perm] = ex
        x.update(dval=dval.astype(F32), val=rng.choice(np.array([0.5, 1.0, 2.0], F32), E), ex=ex, eid_perm=perm, ex_perm=exp_)
    else:
        idx, act, info, sh = ell_block(shape, K)
        m = idx >= 0
        n = int(m.sum())
        eid = np.full(idx.shape, -1, np.int32)
        eid[m] = rng.permutation(n).astype(np.int32) + 2
        dval = np.where(m, ints(rng, idx.shape) * (rng.random(idx.shape) < 0.85), 0.0).astype(F32)
        x.update(ncols=sh["ncols"], row0=sh["row0"], rows=sh["rows"], K=K, rowptr=None, idx=idx, act=act, info=info, eid=eid, dval=dval,
                 val=np.where(m, rng.choice(np.array([0.5, 1.0, 2.0], F32), idx.shape), 0.0).astype(F32), ex=rng.integers(0, 3, n + 5).astype(F32))
    x["deg"] = rng.integers(0, 3, x["ncols"]).astype(F32)
    x["AB"] = np.zeros((x["ncols"], 2 * hw), F32)
    x["dpar0"] = ints(rng, 5 * hw + 1, 5)
    x["Apat"] = ints(rng, (x["ncols"], hw), 5)
    return x


def exact_ref(x, perturb, use_deg=True, use_ex=True, dval=None, ex=None):
    """the integer reference: ds = dp / 4, dz = ds w2 (an outer product: every sum is a scalar sum times w2) -> dA, dB [ncols, hw], dpar,
    ok (every term a multiple of the unit, every sum of magnitudes below 2^24 units, hid included)"""
    if dval is not None or ex is not None:
        x = dict(x)
        x["dval"] = x["dval"] if dval is None else dval
        x["ex"] = x["ex"] if ex is None else ex
    f = flat(x, use_ex)
    hw, n, w2 = x["hw"], x["ncols"], x["P"]["w2"].astype(F8)
    g, val = f["g"].astype(F8), f["val"].astype(F8)
    ds = (2.0 * g * val if perturb else g) / 4.0
    du = x["deg"].astype(F8)[f["u"]] if use_deg else np.zeros(len(g))
    dv = x["deg"].astype(F8)[f["j"]] if use_deg else np.zeros(len(g))
    exv = f["exv"].astype(F8) if use_ex else np.zeros(len(g))
    z = 1.0 + du + dv + exv
    sums, mags = [], []
    for t in (ds, np.abs(ds)):
        sA, sB = np.zeros(n), np.zeros(n)
        np.add.at(sA, f["u"], t)
        np.add.at(sB, f["j"], t)
        sums.append((sA, sB, (t * du).sum(), (t * dv).sum(), (t * exv).sum(), t.sum(), (t * z).sum()))
    (sA, sB, a, b, c_, d, e), m = sums[0], sums[1]
    dpar = np.concatenate([a * w2, b * w2, c_ * w2, d * w2, np.full(hw, e), [d]])
    wmax = max(float(np.abs(w2).max()), 1.0)
    unit = 0.25
    worst = max(m[0].max(initial=0), m[1].max(initial=0), m[2], m[3], m[4], m[5], m[6]) * wmax / unit
    whole = all(np.array_equal(v, np.round(v)) for v in (ds / unit, z, w2, np.asarray(a / unit), np.asarray(e / unit)))
    hid_ok = bool((z >= 1).all()) and float(z.max(initial=1)) * float(np.abs(w2).sum()) < EXACT_LIMIT and float(w2.sum()) == 0.0
    return dict(dA=sA[:, None] * w2, dB=sB[:, None] * w2, dpar=dpar, listed=np.bincount(f["j"][ds != 0], minlength=n), ok=whole and hid_ok and worst < EXACT_LIMIT,
                z=z, ds=ds, f=f)


def lowword_pattern(x):
    """dval / ex of a det call whose first workgroup sums ds to 2^24 + 1 (w2 = 0 on this pattern, so only dw2 and db2 are non-zero): the
    first live entries of rows 0 and 4 carry ds = +-2^24 at z = 1, the one of row 2 carries ds = 1 at z = 2"""
    rowsel = []
    for i in (0, 2, 4):
        if x["rowptr"] is not None:
            rowsel.append(int(x["rowptr"][i]))
            assert x["rowptr"][i + 1] > x["rowptr"][i]
        else:
            rowsel.append(i * x["K"] + int(np.flatnonzero(x["idx"][i] >= 0)[0]))
    dval = np.zeros(x["dval"].size, F32)
    dval[rowsel] = (2.0 ** 26, 4.0, -2.0 ** 26)
    ex = np.zeros_like(x["ex"])
    eid = np.arange(x["dval"].size) if x["eid"] is None else x["eid"].ravel()
    ex[eid[rowsel[1]]] = 1.0
    return dval.reshape(x["dval"].shape), ex


EXACT_ELL = [("wave", 64, hw) for hw in BWD_HW] + [("wave", 5, hw) for hw in BWD_HW] + [("loop", 4, 8)] + [("shard", 64, hw) for hw in (1, 4, 16, 64, 256)] + \
            [("shard", 5, hw) for hw in (16, 256)]
EXACT_CSR = [("csr%d" % N, 7, hw) for N in SIZES for hw in BWD_HW]


def test_exactness_premises_hold_for_every_case():
    from oracle import oracle as O
    for key in EXACT_ELL + EXACT_CSR:
        x = exact_case(*key)
        P = x["P"]
        for use_deg, use_ex in ((True, True), (False, False)):
            for perturb in (0, 1):
                r = exact_ref(x, perturb, use_deg, use_ex)
                assert r["ok"], key
                assert all(np.array_equal(v.astype(F32), v) for v in (r["dA"], r["dB"], r["dpar"] + x["dpar0"])), key
        # the oracle's forward gives p = 1/2 exactly on every entry
        if key[2] in (1, 2, 16, 256) and key[0] in ("wave", "csr270", "loop", "csr1"):
            f = flat(x)
            xp = np.zeros((x["ncols"], 1), F32)
            p, _ = O.edge_mlp_fwd(x["AB"], xp, f["u"], f["j"], x["deg"], f["exv"], 1, 0.0, P["wdu"], P["wdv"], P["wex"], P["b1"], P["w2"], 0.0, 1)
            assert (p == F32(0.5)).all(), key
    assert F32(0.5) + EPS == F32(0.5)
    # the oracle's backward (double sums) is the integer reference bit for bit; with perturb it divides by p + 1e-8 in DOUBLE, 2e-8 off
    # 1/2: that rounds away wherever the sum is not a cancellation (sums that cancel to 0 come out as 4e-16), within 2^-24 of the maximum
    for key in (("tiny", 4, 8), ("wave", 64, 16), ("wave", 5, 2), ("loop", 4, 8), ("wave", 64, 1)):
        x = exact_case(*key)
        P = x["P"]
        for perturb in (0, 1):
            for act in (0, 1):
                r = exact_ref(x, perturb)
                dAB, dpar, dex = O.edge_mlp_bwd(x["AB"], x["idx"], x["eid"], x["val"], x["dval"], x["deg"], x["ex"], P["wdu"], P["wdv"], P["wex"], P["b1"],
                                                P["w2"], 0.0, act, bool(perturb))
                rAB = np.concatenate([r["dA"], r["dB"]], 1)
                if perturb == 0:
                    assert same(dAB, rAB) and same(dpar, r["dpar"]) and not dex.any(), (key, perturb, act)
                else:
                    assert rel_max(dAB, rAB) < 2.0 ** -24 and rel_max(dpar, r["dpar"]) < 2.0 ** -24 and np.abs(dex).max() < 1e-6, (key, perturb, act)
    x = exact_case("csr271", 7, 16)
    r = exact_ref(x, 0, False, False)
    dAB, dpar = O.edge_mlp_bwd_csr(x["AB"], x["rowptr"], x["idx"], x["dval"], x["P"]["b1"], x["P"]["w2"], 0.0, 1)
    assert same(dAB, np.concatenate([r["dA"], r["dB"]], 1)) and same(dpar, r["dpar"])
    assert len(x["skipped"]) >= 16 + 8
    # the low-word pattern: with w2 = 0 every float sum is exact, the first workgroup's db2 sum is 2^24 + 1 (no float), the total is 1
    for key in (("wave", 64, 16), ("csr271", 7, 16), ("wave", 64, 256)):
        x = dict(exact_case(*key))
        x["P"] = dict(x["P"], w2=np.zeros(x["hw"], F32))
        dval, ex = lowword_pattern(x)
        r = exact_ref(x, 0, False, True, dval=dval, ex=ex)
        ds, u = r["ds"], r["f"]["u"]
        wg0 = float(ds[u < 4].sum())                                     # rows 0..3: the first workgroup, whatever the grid
        assert wg0 == 2.0 ** 24 + 1 and float(F32(wg0)) != wg0 and wg0 - float(F32(wg0)) == 1.0
        assert float(ds.sum()) == 1.0 and r["dpar"][-1] == 1.0 and (r["dpar"][4 * x["hw"]:5 * x["hw"]] == 2.0).all() and not r["dA"].any()
        nz = np.flatnonzero(ds)
        assert list(u[nz]) == [0, 2, 4] and list(r["z"][nz]) == [1.0, 2.0, 1.0]
        assert float(F32(2.0 ** 24) + F32(2.0)) == 2.0 ** 24 + 2                  # dw2 of that workgroup: exact in float
    # ... and the check does fail outside the exact range
    x = dict(exact_case("wave", 64, 16))
    assert not exact_ref(x, 0, dval=x["dval"] * F32(1 << 22))["ok"]
    x["deg"] = x["deg"] + F32(0.3)
    assert not exact_ref(x, 0)["ok"]


# ---------------------------------------------------------------------------------------------------------------
# tier 2: the oracle's formula in numpy
# ---------------------------------------------------------------------------------------------------------------
def fma(T, a, b, c):
    """float64: a b + c.  float32: fmaf through one double product (exact) and sum, rounded to float32"""
    if T == np.float64:
        return a * b + c
    return (np.asarray(a, F8) * np.asarray(b, F8) + np.asarray(c, F8)).astype(F32)


def total(T, t):
    """the terms added one by one in the order given, in T"""
    return np.cumsum(t, axis=0, dtype=T)[-1] if len(t) else np.zeros(t.shape[1:], T)


def restate_edge_mlp_bwd(T, f, ncols, hw, AB, deg, P, act, perturb, perm=None, groups=None, keep=False):
    """f: the entries (flat); deg None: no degree terms; f['exv'] None: no extra.  float32: p recomputed as the kernel does (fma chain
    over the hidden units, ora_exp, 1e-8f); db2 in double from the entry to the sum of its group (groups [entries]: the workgroup of
    the entry's row; None: one group, the det form's double sum over everything), the groups' sums rounded to float32 and added in
    float32 in the order in which the groups turn up, as the atomics onto dpar do.  -> dict dA, dB [ncols, hw], dex [nslot],
    dwdu .. dw2 [hw], db2, abs_ds"""
    from oracle import oracle as O
    perm = np.arange(len(f["u"])) if perm is None else perm
    u, j, g, val = f["u"][perm], f["j"][perm], f["g"][perm].astype(T), f["val"][perm].astype(T)
    n = len(u)
    p_ = {k_: P[k_].astype(T) for k_ in ("wdu", "wdv", "wex", "b1", "w2")}
    z = AB[u, :hw].astype(T) + AB[j, hw:].astype(T)
    du = dv = exv = np.zeros(n, T)
    if deg is not None:
        du, dv = deg.astype(T)[u], deg.astype(T)[j]
        z = fma(T, du[:, None], p_["wdu"][None, :], z)
        z = fma(T, dv[:, None], p_["wdv"][None, :], z)
    if f["exv"] is not None:
        exv = f["exv"][perm].astype(T)
        z = fma(T, exv[:, None], p_["wex"][None, :], z)
    z = z + p_["b1"][None, :]
    hid = np.where(z > 0, z, T(LEAKY) * z) if act == 1 else z
    s = np.zeros(n, T)
    for o in range(hw):
        s = fma(T, hid[:, o], p_["w2"][o], s)
    s = s + T(P["b2"][0])
    e = np.exp(-s) if T == np.float64 else (vec(O.exp)(-s) if n else np.zeros(0, F32))
    p = T(1) / (T(1) + e)
    dp = g * val / (p + T(EPS)) if perturb else g
    ds = (dp * p * (T(1) - p)).astype(T)
    dh = ds[:, None] * p_["w2"][None, :]
    dz = np.where(z > 0, dh, T(LEAKY) * dh) if act == 1 else dh
    de = np.zeros(n, T)
    if f["exv"] is not None:
        for o in range(hw):
            de = fma(T, dz[:, o], p_["wex"][o], de)
    dex = np.zeros(f["nslot"], T)
    dex[f["pos"][perm]] = de
    ds8 = ds.astype(F8)
    if T == np.float64 or groups is None:
        db2 = T(ds8.sum())
    else:
        _, first, inv = np.unique(groups[perm], return_index=True, return_inverse=True)
        db2 = total(F32, np.bincount(inv, weights=ds8).astype(F32)[np.argsort(first, kind="stable")])
    out = dict(dA=seg_sum(u, dz, ncols), dB=seg_sum(j, dz, ncols), dex=dex, dwdu=total(T, dz * du[:, None]), dwdv=total(T, dz * dv[:, None]),
               dwex=total(T, dz * exv[:, None]), db1=total(T, dz), dw2=total(T, ds[:, None] * hid), db2=db2, abs_ds=float(np.abs(ds8).sum()))
    assert all(v.dtype == T for k_, v in out.items() if k_ not in ("abs_ds", "db2"))
    if keep:                                                           # the per-entry terms, for further_orders
        out["terms"] = dict(j=j, dz=dz, ds8=ds8, gid=None if groups is None else groups[perm], dwdu=dz * du[:, None], dwdv=dz * dv[:, None],
                            dwex=dz * exv[:, None], db1=dz, dw2=ds[:, None] * hid)
    return out


ATOMIC_OUTS = ("dB", "dwdu", "dwdv", "dwex", "db1", "dw2", "db2")


def further_orders(terms, ref, ncols, n=NDRAW, seed=0):
    """The sums that the GPU adds by float atomics (dB, the blocks of dpar, db2) come out in another order every run, and where ONE number
    decides the statistic (db2 is a scalar; at hw = 2 the hub's two sums decide max|dB|) the larger of two float32 draws is itself a
    lucky or unlucky draw.  So the float32 restatement's per-entry terms are added in n further seeded orders -> {output: the largest
    error of those orders, in the statistic of the table}.  dB: the nodes that HEAVY or more entries list (the long sums; the others
    stay with the two full draws) and, as for the blocks of dpar, the first NUNIT hidden units; db2: the groups' float32 sums in n orders (no groups: one double sum, nothing to draw)."""
    rng = np.random.default_rng(7000 + seed)
    j, dz = terms["j"], terms["dz"][:, :NUNIT]
    heavy = np.flatnonzero(np.bincount(j, minlength=ncols) >= HEAVY)
    slot = np.full(ncols, -1, I8)
    slot[heavy] = np.arange(len(heavy))
    on = np.flatnonzero(slot[j] >= 0)
    worst = dict.fromkeys(ATOMIC_OUTS, 0.0)
    den = {k_: float(np.abs(ref[k_]).max()) or 1.0 for k_ in ATOMIC_OUTS[:-1]}
    gsum = None
    if terms["gid"] is not None:
        gsum = np.bincount(np.unique(terms["gid"], return_inverse=True)[1], weights=terms["ds8"]).astype(F32)
    for _ in range(n):
        perm = rng.permutation(len(j))
        if len(on):
            po = on[rng.permutation(len(on))]
            dB = seg_sum(slot[j[po]], dz[po], len(heavy))
            worst["dB"] = max(worst["dB"], float(np.abs(dB.astype(F8) - ref["dB"][heavy, :NUNIT]).max()) / den["dB"])
        for k_ in ATOMIC_OUTS[1:-1]:
            worst[k_] = max(worst[k_], float(np.abs(total(F32, terms[k_][perm, :NUNIT]).astype(F8) - ref[k_][:NUNIT]).max()) / den[k_])
        if gsum is not None:
            worst["db2"] = max(worst["db2"], float(abs(float(total(F32, gsum[rng.permutation(len(gsum))])) - ref["db2"]) / (ref["abs_ds"] or 1.0)))
    return worst


OUTS = ("dA", "dB", "dex", "dwdu", "dwdv", "dwex", "db1", "dw2")


def t2_params(hw, rng):
    v = lambda s_: (rng.standard_normal(hw) * s_).astype(F32)  # noqa: E731
    return dict(wdu=v(0.05), wdv=v(0.05), wex=v(0.5), b1=v(0.1), w2=v(0.4), b2=np.array([0.1], F32))


@functools.lru_cache(maxsize=None)
def t2_case(shape, K, hw, act, perturb, ex_mode, use_deg):
    """normal data; p_edge / ex from the oracle's forward on the case's own entries, val = p (perturbed through O.log / O.exp)"""
    from oracle import oracle as O
    rng = np.random.default_rng(2000 + 13 * hw + K + sum(map(ord, shape)) + 2 * act + perturb)
    x = dict(shape=shape, hw=hw, P=t2_params(hw, rng), act=act, perturb=perturb, use_deg=use_deg)
    if shape.startswith("csr"):
        g = build_graph(int(shape[3:]), False)
        x.update(graph=g, ncols=g["N"], row0=0, rows=g["N"], K=7, rowptr=g["rowptr"], idx=g["col"], eid=None)
        m = np.ones(g["E"], bool)
        u, j = g["erow"].astype(I8), g["col"].astype(I8)
    else:
        idx, _, _, sh = ell_block(shape, K)
        m = idx >= 0
        x.update(ncols=sh["ncols"], row0=sh["row0"], rows=sh["rows"], K=K, rowptr=None, idx=idx)
        u, j = sh["row0"] + np.nonzero(m)[0].astype(I8), idx[m].astype(I8)
    n, N = len(u), x["ncols"]
    x["AB"] = (0.5 * rng.standard_normal((N, 2 * hw))).astype(F32)
    x["deg"] = (3 + 20 * rng.random(N)).astype(F32)
    h = 129
    xp = (0.2 * rng.standard_normal((N, h))).astype(F32)
    ex_in = (0.5 + rng.random(n)).astype(F32)
    P = x["P"]
    p, ex = O.edge_mlp_fwd(x["AB"], xp, u, j, x["deg"] if use_deg else None, ex_in, ex_mode, -1.0, P["wdu"], P["wdv"], P["wex"], P["b1"], P["w2"], P["b2"][0],
                           act)
    assert ex_mode == 2 or np.array_equal(ex, ex_in)
    val = vec(O.exp)((vec(O.log)((p + EPS).astype(F32)) + (0.3 * rng.gumbel(size=n)).astype(F32)).astype(F32)) if perturb else p
    dval = rng.standard_normal(n).astype(F32)
    dval[rng.integers(0, n, 7)] = 0.0
    if x["rowptr"] is not None:
        x.update(val=val, dval=dval, ex=ex)
    else:
        eid = np.full(x["idx"].shape, -1, np.int32)
        order = rng.permutation(n).astype(np.int32)
        eid[m] = order
        exa = np.empty(n, F32)
        exa[order] = ex
        x.update(eid=eid, ex=exa, val=np.zeros(m.shape, F32), dval=np.zeros(m.shape, F32))
        x["val"][m], x["dval"][m] = val, dval
    x["p_edge"] = p
    return x


T2_COMBOS = [(0, 0, 1, True), (1, 1, 2, False), (1, 0, 2, True), (0, 1, 1, False)]       # (act, perturb, ex_mode, deg), one per hw
T2_FORMS = {"bwd": ("wave", 64), "rows": ("shard", 64), "det": ("csr270", 7), "partp": ("wave", 64), "partp_rows": ("shard", 5)}
T2_CASES = [(form, hw) + T2_COMBOS[(q + (1 if form.startswith("partp") else 0)) % 4] for form in T2_FORMS for q, hw in enumerate(T2_HW)
            if not (form.startswith("partp") and hw == 2)]
T2_FORMS["bwd-csr"] = ("csr270", 7)             # the atomic form on the CSR pattern: rows of up to 200 entries in batches, dex that is not zero
T2_CASES.append(("bwd-csr", 64, 1, 1, 2, True))


def test_tier2_cases_cover_every_value_with_every_form():
    for form in [k_ for k_ in T2_FORMS if k_ != "bwd-csr"]:
        mine = [c for c in T2_CASES if c[0] == form]
        assert {c[1] for c in mine} == set(T2_HW) - ({2} if form.startswith("partp") else set())
        for pos, values in ((2, {0, 1}), (3, {0, 1}), (4, {1, 2}), (5, {True, False})):
            assert {c[pos] for c in mine} == values, (form, pos)


def test_float64_restatement_matches_the_oracle():
    """restate_edge_mlp_bwd(float64) against O.edge_mlp_bwd (ELL, whole graph) and O.edge_mlp_bwd_csr: the oracle accumulates in double
    and rounds its results to float32 once, so 4 * 2^-24 of max bounds the difference; the float32 restatement in both orders stays
    within 1e-4"""
    from oracle import oracle as O
    tol = 4 * 2.0 ** -24
    for hw, (act, perturb, ex_mode, use_deg) in zip((2, 16, 64, 16), T2_COMBOS):
        x = t2_case("wave", 64, hw, act, perturb, ex_mode, use_deg)
        P, f = x["P"], flat(x)
        deg = x["deg"] if use_deg else None
        ref = restate_edge_mlp_bwd(np.float64, f, x["ncols"], hw, x["AB"], deg, P, act, perturb)
        dAB, dpar, dex = O.edge_mlp_bwd(x["AB"], x["idx"], x["eid"], x["val"], x["dval"], deg, x["ex"], P["wdu"] if use_deg else None,
                                        P["wdv"] if use_deg else None, P["wex"], P["b1"], P["w2"], P["b2"][0], act, bool(perturb))
        got = dict(dA=dAB[:, :hw], dB=dAB[:, hw:], dex=dex.ravel(), **{k_: dpar[q * hw:(q + 1) * hw] for q, k_ in enumerate(OUTS[3:])})
        for k_ in OUTS:
            assert rel_max(got[k_], ref[k_]) < tol, (hw, k_, rel_max(got[k_], ref[k_]))
        assert abs(float(dpar[5 * hw]) - ref["db2"]) < tol * ref["abs_ds"]
        for perm in orders(len(f["u"]), 1):
            r32 = restate_edge_mlp_bwd(np.float32, f, x["ncols"], hw, x["AB"], deg, P, act, perturb, perm)
            assert all(rel_max(r32[k_], ref[k_]) < 1e-4 for k_ in OUTS) and abs(float(r32["db2"]) - ref["db2"]) < 1e-4 * ref["abs_ds"]
    x = t2_case("csr270", 7, 16, 1, 0, 1, False)
    f = flat(x, use_ex=False)
    ref = restate_edge_mlp_bwd(np.float64, f, x["ncols"], 16, x["AB"], None, x["P"], 1, 0)
    dAB, dpar = O.edge_mlp_bwd_csr(x["AB"], x["rowptr"], x["idx"], x["dval"], x["P"]["b1"], x["P"]["w2"], x["P"]["b2"][0], 1)
    assert rel_max(dAB[:, :16], ref["dA"]) < tol and rel_max(dAB[:, 16:], ref["dB"]) < tol and rel_max(dpar[48:64], ref["db1"]) < tol
    assert rel_max(dpar[64:80], ref["dw2"]) < tol and abs(float(dpar[80]) - ref["db2"]) < tol * ref["abs_ds"] and not dpar[:48].any()
    # the further orders draw from the same distribution as the two full ones: same magnitude, zero draws give zero, no groups no db2
    x = t2_case("shard", 64, 2, 0, 0, 1, True)
    f = flat(x)
    ref = restate_edge_mlp_bwd(np.float64, f, x["ncols"], 2, x["AB"], x["deg"], x["P"], 0, 0)
    r32 = restate_edge_mlp_bwd(np.float32, f, x["ncols"], 2, x["AB"], x["deg"], x["P"], 0, 0, None, (f["u"] - x["row0"]) // 4, keep=True)
    more = further_orders(r32["terms"], ref, x["ncols"])
    assert set(more) == set(ATOMIC_OUTS) and all(0 < v < 1e-4 for v in more.values())
    assert more["dB"] >= 0.25 * rel_max(r32["dB"], ref["dB"]) and more["db2"] < 16 * 2.0 ** -24
    assert not any(further_orders(r32["terms"], ref, x["ncols"], n=0).values())
    assert further_orders(dict(r32["terms"], gid=None), ref, x["ncols"], n=2)["db2"] == 0.0
    assert (np.bincount(f["j"], minlength=x["ncols"]) >= HEAVY).sum() == 4          # the hub and the nodes of in-degree 127, 128, 129
    # fma(float32) is one rounding: 2^-24 * (1 + 2^-24) + 1 rounds to 1 + 2^-23 through the fused product, to 1 through two roundings
    a = F32(1 + 2.0 ** -12)
    assert fma(np.float32, a, a, F32(-1.0)) == F32(2.0 ** -11 + 2.0 ** -24) and F32(a * a) - F32(1.0) == F32(2.0 ** -11)
    # db2 by groups: double inside a group, float32 across the groups in the order they turn up
    fz = dict(u=np.zeros(4, I8), j=np.zeros(4, I8), pos=np.arange(4), g=np.array([2.0 ** 27, 4.0, -2.0 ** 27, 4.0], F32), val=np.ones(4, F32), exv=None, nslot=4)
    Pz = dict(exact_params(2), w2=np.zeros(2, F32))
    one = lambda gr: float(restate_edge_mlp_bwd(np.float32, fz, 1, 2, np.zeros((1, 4), F32), None, Pz, 0, 0, None, gr)["db2"])  # noqa: E731
    assert one(None) == 2.0 and one(np.array([0, 0, 0, 1])) == 2.0 and one(np.array([0, 1, 2, 3])) == 1.0 and one(np.array([0, 1, 0, 1])) == 2.0
    assert total(np.float32, np.array([1e8, 1.0, -1e8], F32)) == 0.0 and total(np.float32, np.array([1e8, -1e8, 1.0], F32)) == 1.0


# ---------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import dgg_amd  # noqa: F401
    return torch.device("cuda:0")


ROWS_ARGS = "AB N hw row0 row1 rowptr idx eid val dval K deg ex wdu wdv wex b1 w2 b2 act perturb dAB dpar dex"
PARTP_TAIL = "deg ex wdu wdv wex b1 w2 b2 act perturb part"
FORMS = {
    "bwd": ("dgg_edge_mlp_bwd", ROWS_ARGS.replace(" row0 row1", "")),
    "rows": ("dgg_edge_mlp_bwd_rows", ROWS_ARGS),
    "det": ("dgg_edge_mlp_bwd_det", ROWS_ARGS + " ws ws_floats"),
    "partp": ("dgg_edge_mlp_bwd_partp", "AB rows hw idx eid val dval w K " + PARTP_TAIL + " ncols dz_rec dz_rows dAB dpar dex"),
    "partp_rows": ("dgg_edge_mlp_bwd_partp_rows", "AB N hw row0 row1 idx eid val dval w K " + PARTP_TAIL + " dz_rec dz_rows dAB dpar dex"),
}


def launch(c, form, a, **over):
    name, names = FORMS[form]
    a = dict(a, **over)
    return c.call(name, *[a[k_] for k_ in names.split()])


def dab_start(x):
    """A halves: NaN on the rows of the block (they are stored), an integer pattern elsewhere; B halves +0.0 (they are accumulated)"""
    hw, r0, r1 = x["hw"], x["row0"], x["row0"] + x["rows"]
    s = np.zeros((x["ncols"], 2 * hw), F32)
    s[:, :hw] = x["Apat"] if "Apat" in x else 0.0
    s[r0:r1, :hw] = np.nan
    return s


def operands(c, x, act, perturb, use_deg=True, use_ex=True, dex=True, eid="own", dval=None, ex=None, w2=None):
    """uploads a case -> dict of the named arguments of every form (outputs NaN-filled or holding their start pattern)"""
    P = x["P"]
    a = dict(AB=c.inp(x["AB"]), N=x["ncols"], rows=x["rows"], ncols=x["ncols"], hw=x["hw"], row0=x["row0"], row1=x["row0"] + x["rows"], K=x["K"],
             rowptr=None if x["rowptr"] is None else c.inp(x["rowptr"]), idx=c.inp(x["idx"]), val=c.inp(x["val"]),
             dval=c.inp(x["dval"] if dval is None else dval), act=act, perturb=perturb, b1=c.inp(P["b1"]), w2=c.inp(P["w2"] if w2 is None else w2),
             b2=c.inp(P["b2"]), deg=None, wdu=None, wdv=None, ex=None, wex=None, eid=None, ws=None, ws_floats=0, w=None, part=None, dz_rec=None,
             dz_rows=0)
    if use_deg:
        a.update(deg=c.inp(x["deg"]), wdu=c.inp(P["wdu"]), wdv=c.inp(P["wdv"]))
    if use_ex:
        exa = x["ex"] if ex is None else ex
        if eid == "perm":
            a.update(ex=c.inp(x["ex_perm"]), eid=c.inp(x["eid_perm"]))
        else:
            a.update(ex=c.inp(exa), eid=None if x["eid"] is None else c.inp(x["eid"]))
        a["wex"] = c.inp(P["wex"])
    a["dAB"] = c.out(None, start=dab_start(x))
    a["dpar"] = c.out(None, start=x["dpar0"] if "dpar0" in x else np.zeros(5 * x["hw"] + 1, F32))
    a["dex"] = c.out(x["dval"].shape) if dex else None
    return a


def check_exact(bad, tag, x, a, ref):
    hw, r0, r1 = x["hw"], x["row0"], x["row0"] + x["rows"]
    exp = dab_start(x)
    exp[r0:r1, :hw] = ref["dA"][r0:r1]
    exp[:, hw:] = ref["dB"]
    got = expect(bad, tag + " dAB", a["dAB"], exp)
    quiet = np.flatnonzero(ref["listed"] == 0)
    if got[quiet, hw:].view(np.uint32).any():
        bad.append(tag + ": the B half of a node nobody lists is not +0.0")
    expect(bad, tag + " dpar", a["dpar"], x["dpar0"] + ref["dpar"])
    if a["dex"] is not None:
        expect(bad, tag + " dex", a["dex"], np.zeros(x["dval"].shape, F32))


def combo(q):
    """(act, perturb, use_deg, use_ex, dex) of the q-th run: every pair of values turns up within four runs"""
    return ((0, 0, True, True, True), (1, 1, False, True, True), (1, 0, True, False, False), (0, 1, False, False, True), (1, 1, True, True, False))[q % 5]


def run_exact(dev, form, key, q, bad, **kw):
    x = exact_case(*key)
    act, perturb, use_deg, use_ex, dex = combo(q)
    c = Ctx(dev)
    a = operands(c, x, act, perturb, use_deg, use_ex, dex)
    rc = launch(c, form, a, **kw)
    tag = "%s %s act=%d perturb=%d deg=%d ex=%d" % (form, key, act, perturb, use_deg, use_ex)
    if rc != 0:
        bad.append("%s returned %d" % (tag, rc))
        return
    check_exact(bad, tag, x, a, exact_ref(x, perturb, use_deg, use_ex))
    c.inputs_intact()


@pytest.mark.gpu
@pytest.mark.parametrize("hw", BWD_HW)
def test_ell_backward_is_the_integer_reference(dev, hw):
    bad = []
    for q in range(5):
        run_exact(dev, "bwd", ("wave", 64, hw), q + hw, bad)
    for q in range(2):
        run_exact(dev, "bwd", ("wave", 5, hw), q + hw, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_default_dispatch_takes_a_second_row(dev):
    """4109 rows under the default 1024 workgroups: the last 13 rows are second trips of the persistent loop"""
    bad = []
    for q in range(4):
        run_exact(dev, "bwd", ("loop", 4, 8), q, bad)
    r = exact_ref(exact_case("loop", 4, 8), 0)
    assert np.abs(r["dA"][-13:]).sum() > 0 and not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", (1, 4, 16, 64, 256))
def test_rows_backward_on_a_shard_is_the_integer_reference(dev, hw):
    bad = []
    for q in range(4):
        run_exact(dev, "rows", ("shard", 64, hw), q + hw, bad)
    x = exact_case("shard", 64, hw)
    r = exact_ref(x, 0)
    assert r["listed"][x["info"]["zero_in"]] == 0 and r["listed"][x["info"]["zero_out"]] == 0 and (x["Apat"][:300] != 0).any()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_csr_backward_is_the_integer_reference(dev, N):
    """rowptr form: eid = NULL (identity) with dex requested and with dex = NULL, an explicit eid, no ex at all; rows of up to 200 entries
    walked in 64 / LPE batches, whole batches of the 200-long row without a cotangent (their dex is zero-filled), empty rows"""
    bad = []
    for q, hw in enumerate(BWD_HW):
        x = exact_case("csr%d" % N, 7, hw)
        for run in range(3):
            act, perturb, use_deg = (q + run) % 2, (q + run // 2) % 2, run != 1
            use_ex, dex, eid = run != 2 or q % 2 == 0, run != 1, "perm" if run == 2 else "own"
            c = Ctx(dev)
            a = operands(c, x, act, perturb, use_deg, use_ex, dex, eid)
            tag = "csr N=%d hw=%d run %d" % (N, hw, run)
            assert launch(c, "bwd", a) == 0, tag
            check_exact(bad, tag, x, a, exact_ref(x, perturb, use_deg, use_ex))
            c.inputs_intact()
    assert not bad, "\n".join(bad)


DET_WS = {"one-row": lambda np_: np_, "three-rows": lambda np_: 3 * np_, "three-rows-and-a-float": lambda np_: 3 * np_ + 1}


@pytest.mark.gpu
@pytest.mark.parametrize("ws_kind", list(DET_WS) + ["every-workgroup"])
def test_det_backward_is_the_integer_reference(dev, ws_kind):
    """the workspace decides the grid: 1 workgroup walks every row, 3 workgroups, 3 with a row that is not whole, and one row per
    workgroup the atomic form would launch; then the pattern whose first workgroup sums db2 to 2^24 + 1"""
    bad = []
    for q, key in enumerate((("wave", 64, 16), ("csr271", 7, 16), ("wave", 5, 256), ("csr273", 7, 2), ("shard", 64, 4))):
        x = exact_case(*key)
        np_ = 5 * x["hw"] + 2
        nws = DET_WS[ws_kind](np_) if ws_kind in DET_WS else ((x["rows"] + 3) // 4) * np_
        for low in (False, True):
            if low and key[0] == "shard":
                continue
            act, perturb, use_deg, use_ex, dex = combo(q)
            c = Ctx(dev)
            over = {}
            if low:
                dval, ex = lowword_pattern(x)
                over, perturb, use_deg, use_ex = dict(dval=dval, ex=ex, w2=np.zeros(x["hw"], F32)), 0, False, True
            a = operands(c, x, act, perturb, use_deg, use_ex, dex, **over)
            a.update(ws=c.out(nws), ws_floats=nws)
            tag = "det %s ws=%d%s" % (key, nws, " low word" if low else "")
            assert launch(c, "det", a) == 0, tag
            xr = dict(x, P=dict(x["P"], w2=np.zeros(x["hw"], F32))) if low else x
            check_exact(bad, tag, x, a, exact_ref(xr, perturb, use_deg, use_ex, **{k_: v for k_, v in over.items() if k_ != "w2"}))
            c.inputs_intact()
    assert not bad, "\n".join(bad)


def build_part(c, dev, a, x, w, ws=None):
    """dgg_partp_build of (idx, w) in a workspace the test owns -> the device workspace, the record count"""
    import torch
    from dgg_amd import _lib
    nbytes = _lib.lib().dgg_partp_ws_bytes(x["rows"], x["K"], x["ncols"])
    assert nbytes > 0 and _lib.lib().dgg_partp_has_map(x["rows"]) == 1
    if ws is None:
        ws = torch.zeros(nbytes + 512, dtype=torch.uint8, device=dev)
    gw = c.inp(w)
    assert c.call("dgg_partp_build", a["idx"], gw, a["val"], c.inp(np.ones(x["rows"], F32)), x["rows"], x["K"], x["ncols"], ws.data_ptr()) == 0
    a.update(w=gw, part=ws.data_ptr())
    return ws, int(((x["idx"] >= 0) & (w != 0)).sum())


def partp_weights(x, seed=0):
    """w != 0 on the active entries (build_block's `act`) and on a share of the rest; 0 elsewhere"""
    rng = np.random.default_rng(seed + x["hw"])
    m = x["idx"] >= 0
    return (m & (x["act"] | (rng.random(m.shape) < 0.3))).astype(F32) * rng.choice(np.array([0.5, 1.0, 3.0], F32), m.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", PARTP_HW)
def test_partp_backward_is_the_integer_reference(dev, hw):
    """the neighbour side through the payload partition: dz_rec NaN-filled, dz_rows = the record count, half of it (the records beyond
    go the atomic way, edge_mlp_colsum clamps), 1; cotangents only on recorded entries, some recorded entries without one"""
    bad = []
    for q, (form, key) in enumerate((("partp", ("wave", 64, hw)), ("partp_rows", ("shard", 64, hw)), ("partp", ("wave", 5, hw)), ("partp_rows", ("shard", 5, hw)))):
        x = exact_case(*key)
        w = partp_weights(x)
        dval = (x["dval"] * (w != 0)).astype(F32)
        assert ((w != 0) & (dval == 0)).any() and ((x["idx"] >= 0) & (w == 0)).any()
        for run, frac in enumerate((1.0, 0.5, 0.0)):
            if q >= 2 and run != (q + hw) % 3:
                continue
            act, perturb, use_deg, use_ex, dex = combo(q + run)
            c = Ctx(dev)
            a = operands(c, x, act, perturb, use_deg, use_ex, dex, dval=dval)
            ws, nrec = build_part(c, dev, a, x, w)
            nrows = max(1, int(nrec * frac))
            a.update(dz_rec=c.out((nrec, hw)), dz_rows=nrows)           # (the buffer holds every record; the kernels are told of nrows)
            tag = "%s %s dz_rows=%d of %d" % (form, key, nrows, nrec)
            assert launch(c, form, a) == 0, tag
            if not np.isnan(a["dz_rec"].read("dz_rec")[nrows:]).all():
                bad.append(tag + ": a row of dz_rec beyond dz_rows was written")
            check_exact(bad, tag, x, a, exact_ref(x, perturb, use_deg, use_ex, dval=dval))
            c.inputs_intact()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", PARTP_HW)
def test_partp_entry_without_a_record_takes_the_atomics(dev, hw):
    """the contract case: the partition is built with every selected entry recorded, then rebuilt in the same workspace with w = 0 on a
    named set of entries that keep their cotangent.  Those entries have no record (their slot of the entry -> record map still holds
    the first build's position): they must reach dAB through the atomics, and no other entry's contribution may change"""
    bad = []
    for form, key in (("partp", ("wave", 64, hw)), ("partp_rows", ("shard", 5, hw))):
        x = exact_case(*key)
        m = x["idx"] >= 0
        w_all = m.astype(F32)
        rng = np.random.default_rng(hw)
        named = m & (x["dval"] != 0) & (rng.random(m.shape) < 0.15)
        hubcol = x["idx"] == x["info"]["hub"]
        named |= hubcol & (x["dval"] != 0) & (np.arange(x["rows"])[:, None] % 3 == 0)
        assert named.sum() > 50 and (named & hubcol).sum() > 10
        w_cut = np.where(named, 0.0, w_all).astype(F32)
        c = Ctx(dev)
        act, perturb, use_deg, use_ex, dex = combo(hw)
        a = operands(c, x, act, perturb, use_deg, use_ex, dex)
        ws, nrec = build_part(c, dev, a, x, w_all)
        ws, ncut = build_part(c, dev, a, x, w_cut, ws)
        assert ncut == nrec - int(named.sum())
        a.update(dz_rec=c.out((nrec, hw)), dz_rows=nrec)
        tag = "%s %s rebuilt without %d records" % (form, key, int(named.sum()))
        assert launch(c, form, a) == 0, tag
        check_exact(bad, tag, x, a, exact_ref(x, perturb, use_deg, use_ex))
        c.inputs_intact()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# DGG_EMLP_GRID is read once per process: one fresh process per value
# ---------------------------------------------------------------------------------------------------------------
def grid_child_checks(dev):
    bad = []
    for q in range(3):
        run_exact(dev, "bwd", ("wave", 64, 16), q, bad)
    x = exact_case("wave", 64, 16)
    w = partp_weights(x)
    dval = (x["dval"] * (w != 0)).astype(F32)
    for q, frac in enumerate((1.0, 0.5)):
        act, perturb, use_deg, use_ex, dex = combo(q)
        c = Ctx(dev)
        a = operands(c, x, act, perturb, use_deg, use_ex, dex, dval=dval)
        ws, nrec = build_part(c, dev, a, x, w)
        a.update(dz_rec=c.out((nrec, 16)), dz_rows=int(nrec * frac))
        if launch(c, "partp", a) != 0:
            bad.append("partp refused")
            continue
        check_exact(bad, "partp wave dz_rows=%d" % a["dz_rows"], x, a, exact_ref(x, perturb, use_deg, use_ex, dval=dval))
        c.inputs_intact()
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRID_KNOBS)
def test_emlp_grid_knob_in_a_fresh_process(dev, grid):
    env = dict(os.environ)
    env["DGG_EMLP_GRID"] = str(grid)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--grid-child"]
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("the DGG_EMLP_GRID=%d child process hung: nothing further is started on the GPU" % grid, returncode=3)
    out = r.stdout.decode(errors="replace")
    if r.returncode not in (0, 1):
        pytest.exit("the DGG_EMLP_GRID=%d child process ended abnormally (status %d): nothing further is started on the GPU\n%s" % (grid, r.returncode, out[-2000:]),
                    returncode=3)
    assert r.returncode == 0 and "GRID_CHILD_OK %d" % grid in out, out[-4000:]


def _grid_child():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import dgg_amd  # noqa: F401
    bad = grid_child_checks(torch.device("cuda:0"))
    if bad:
        print("\n".join(bad))
        return 1
    print("GRID_CHILD_OK %s" % os.environ.get("DGG_EMLP_GRID"))
    return 0


# ---------------------------------------------------------------------------------------------------------------
# tier 1: forward and top-K
# ---------------------------------------------------------------------------------------------------------------
def fwd_inputs(g, hw, h, seed=0):
    rng = np.random.default_rng(3000 + g["N"] + hw + h + seed)
    N, E = g["N"], g["E"]
    x = t2_params(hw, rng)
    x.update(AB=(0.5 * rng.standard_normal((N, 2 * hw))).astype(F32), xp=(0.2 * rng.standard_normal((N, h))).astype(F32),
             deg=(3 + 20 * rng.random(N)).astype(F32), ex_in=(0.5 + rng.random(E)).astype(F32), erow=g["erow"].astype(np.int32), col=g["col"])
    return x


def fwd_run(dev, bad, g, x, hw, h, E, ex_mode, use_deg, act, want_ex=True, shift=False):
    from oracle import oracle as O
    c = Ctx(dev)
    N, Eg = g["N"], g["E"]
    if shift:                                                          # AB 4 bytes past a 16-byte boundary
        gab = c.inp(np.concatenate([[np.nan], x["AB"].ravel()]).astype(F32))
        ab = gab.addr + 4
        assert ab % 16 == 4
    else:
        ab = c.inp(x["AB"])
    p, ex = c.out(Eg), (c.out(Eg) if want_ex else None)
    d_ = c.inp(x["deg"]) if use_deg else None
    rc = c.call("dgg_edge_mlp_fwd", ab, c.inp(x["xp"]) if ex_mode == 2 else None, N, h, hw, c.inp(x["erow"]), c.inp(x["col"]), E, d_,
                c.inp(x["ex_in"]) if ex_mode == 1 else None, ex_mode, -1.0, c.inp(x["wdu"]) if use_deg else None, c.inp(x["wdv"]) if use_deg else None,
                c.inp(x["wex"]) if ex_mode else None, c.inp(x["b1"]), c.inp(x["w2"]), c.inp(x["b2"]), act, p, ex)
    tag = "fwd N=%d hw=%d h=%d E=%d ex_mode=%d deg=%d act=%d shift=%d" % (N, hw, h, E, ex_mode, use_deg, act, shift)
    if rc != 0:
        bad.append(tag + " returned %d" % rc)
        return
    rp, rex = O.edge_mlp_fwd(x["AB"], x["xp"], x["erow"][:E], x["col"][:E], x["deg"] if use_deg else None, x["ex_in"][:E] if ex_mode == 1 else None, ex_mode,
                             -1.0, x["wdu"], x["wdv"], x["wex"], x["b1"], x["w2"], x["b2"][0], act)
    expect(bad, tag + " p_edge", p, np.concatenate([rp, nans(Eg - E)]))
    if want_ex:
        expect(bad, tag + " ex_out", ex, np.concatenate([rex, nans(Eg - E)]))
    c.inputs_intact()


@pytest.mark.gpu
@pytest.mark.parametrize("hw", FWD_HW)
def test_forward_equals_the_oracle(dev, hw):
    bad = []
    q = FWD_HW.index(hw)
    g = build_graph(SIZES[q % 4], False)
    x = fwd_inputs(g, hw, 16)
    for ex_mode in (0, 1, 2):
        for use_deg in (True, False):
            act = (ex_mode + use_deg + q) % 2
            fwd_run(dev, bad, g, x, hw, 16, g["E"], ex_mode, use_deg, act, want_ex=not (ex_mode == 1 and use_deg))
            fwd_run(dev, bad, g, x, hw, 16, FWD_E[(ex_mode * 2 + use_deg + q) % 4], ex_mode, use_deg, 1 - act)
    for E in FWD_E:
        fwd_run(dev, bad, g, x, hw, 16, E, 2, True, 1)
    if hw in (16, 64):
        for ex_mode, use_deg in ((0, False), (2, True)):
            fwd_run(dev, bad, g, x, hw, 16, g["E"], ex_mode, use_deg, 1, shift=True)
    g1 = build_graph(1, False)
    fwd_run(dev, bad, g1, fwd_inputs(g1, hw, 16), hw, 16, 1, 2, True, 1)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("h", FWD_H)
def test_forward_distance_extra_equals_the_oracle(dev, h):
    """ex_mode 2 at the latent widths that take both branches of pair_d2_thread"""
    bad = []
    g = build_graph(SIZES[FWD_H.index(h) % 4], False)
    for hw in (16, 17):
        fwd_run(dev, bad, g, fwd_inputs(g, hw, h), hw, h, g["E"], 2, hw == 16, 1)
    assert not bad, "\n".join(bad)


def noise_matrix(N, seed=0):
    rng = np.random.default_rng(5000 + N + seed)
    Gp = np.full((N, N + 3), np.nan, F32)
    Gp[:, :N] = (0.3 * rng.gumbel(size=(N, N))).astype(F32)
    return Gp


def topk_run(dev, bad, g, p, mode, K, r0, r1, Gp):
    from oracle import oracle as O
    N, rowptr, col = g["N"], g["rowptr"], g["col"]
    ridx, rval, reid = O.edgelist_topk_p(p, N, rowptr, col, K, mode, None if Gp is None else np.ascontiguousarray(Gp[:, :N]), SEED)
    c = Ctx(dev)
    e0, e1 = int(rowptr[r0]), int(rowptr[r1])
    whole = (r0, r1) == (0, N)
    outs = [c.out((N, K), np.int32), c.out((N, K)), c.out((N, K), np.int32)]
    ptrs = [gd.addr + 4 * r0 * K for gd in outs]
    gG = None if mode != 1 else c.inp(Gp[r0:r1])
    gp, grp, gcl = c.inp(p[e0:e1]), c.inp(rowptr[r0:r1 + 1] - e0), c.inp(col[e0:e1])
    if whole:
        rc = c.call("dgg_edgelist_topk_p", gp, N, grp, gcl, mode, gG, N + 3, SEED[0], SEED[1], K, *ptrs)
    else:
        rc = c.call("dgg_edgelist_topk_p_rows", gp, N, r0, r1, grp, gcl, mode, gG, N + 3, SEED[0], SEED[1], K, *ptrs)
    tag = "topk_p N=%d rows [%d, %d) mode=%d K=%d" % (N, r0, r1, mode, K)
    if rc != 0:
        bad.append(tag + " returned %d" % rc)
        return
    for nm, gd, ref, fill in (("idx", outs[0], ridx, IFILL), ("val", outs[1], rval, np.nan), ("eid", outs[2], np.where(reid >= 0, reid - e0, -1), IFILL)):
        exp = np.full((N, K), fill, ref.dtype)
        exp[r0:r1] = ref[r0:r1]
        expect(bad, "%s %s" % (tag, nm), gd, exp)
    cnt = np.diff(rowptr)[r0:r1]
    short = np.arange(K)[None, :] >= cnt[:, None]
    assert (ridx[r0:r1][short] == -1).all() and (rval[r0:r1][short] == 0).all() and (reid[r0:r1][short] == -1).all()
    c.inputs_intact()


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_topk_on_given_probabilities_equals_the_oracle(dev, N):
    bad = []
    g = build_graph(N, True)
    Gp = noise_matrix(N)
    for mode in range(4):
        p = rank_values(g, seed=mode)
        for K in TOPK_K:
            topk_run(dev, bad, g, p, mode, K, 0, N, Gp if mode == 1 else None)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("N", (N0, N0 + 3))
def test_topk_rows_of_a_shard_equal_the_sliced_oracle(dev, N):
    """rows [r0, r1): the CSR slice rebased, G and the outputs the shard's rows, the hashes keyed on the global pair"""
    bad = []
    g = build_graph(N, True)
    Gp = noise_matrix(N, 1)
    mid = g["named"]["all"]
    for q, (r0, r1) in enumerate(((1, N - 2), (mid, mid + 3), (N - 5, N), (0, 3), (2, 3))):
        for mode in range(4):
            K = TOPK_K[(q + mode) % 4]
            topk_run(dev, bad, g, rank_values(g, seed=mode), mode, K, r0, r1, Gp if mode == 1 else None)
    topk_run(dev, bad, g, rank_values(g), 3, 64, 1, N - 2, None)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# refusals and empties
# ---------------------------------------------------------------------------------------------------------------
def small_case(hw=8):
    """the wave block's first five ranks at hw = 8; another hw only resizes the operands (nothing is launched on them)"""
    x = dict(exact_case("wave", 5, 8))
    if hw != 8:
        x["hw"] = hw
        x["P"] = {k_: np.resize(v, 1 if k_ == "b2" else hw).astype(F32) for k_, v in x["P"].items()}
        x["AB"] = np.zeros((x["ncols"], 2 * hw), F32)
        x["dpar0"] = np.zeros(5 * hw + 1, F32)
        x["Apat"] = np.zeros((x["ncols"], hw), F32)
    return x


BWD_REFUSALS = [
    ("K-0", "bwd", dict(K=0), ERR_UNSUPPORTED), ("K-65", "bwd", dict(K=65), ERR_UNSUPPORTED),
    ("hw-3", "bwd", dict(hw=3), ERR_UNSUPPORTED), ("hw-12", "bwd", dict(hw=12), ERR_UNSUPPORTED), ("hw-48", "bwd", dict(hw=48), ERR_UNSUPPORTED),
    ("hw-512", "bwd", dict(hw=512), ERR_UNSUPPORTED),
    ("ex-without-wex", "bwd", dict(wex=None), ERR_ARG), ("ex-without-eid-or-rowptr", "bwd", dict(eid=None), ERR_ARG),
    ("deg-without-wdu", "bwd", dict(wdu=None), ERR_ARG),
    ("row0-negative", "rows", dict(row0=-1), ERR_ARG), ("row1-below-row0", "rows", dict(row0=9, row1=8), ERR_ARG), ("row1-beyond-N", "rows", dict(row1=701), ERR_ARG),
    ("det-ws-null", "det", dict(ws=None, ws_floats=1 << 20), ERR_ARG), ("det-ws-one-float-short", "det", dict(ws_floats=5 * 8 + 1), ERR_ARG),
    ("partp-hw-6", "partp", dict(hw=6), ERR_UNSUPPORTED), ("partp-w-null", "partp", dict(w=None), ERR_ARG), ("partp-dz-null", "partp", dict(dz_rec=None), ERR_ARG),
    ("partp-dz-rows-0", "partp", dict(dz_rows=0), ERR_ARG), ("partp-ws-null", "partp", dict(part=None), ERR_UNSUPPORTED),
    ("partp-rows-K-65", "partp_rows", dict(K=65), ERR_UNSUPPORTED), ("partp-rows-row1-beyond-N", "partp_rows", dict(row1=701), ERR_ARG),
    ("rows-0", "rows", dict(row0=5, row1=5), 0), ("det-rows-0", "det", dict(row0=700, row1=700), 0), ("partp-rows-0", "partp", dict(rows=0), 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r[0] for r in BWD_REFUSALS])
def test_backward_refusals_and_empty_blocks_write_nothing(dev, name):
    _, form, over, code = next(r for r in BWD_REFUSALS if r[0] == name)
    x = small_case(over.get("hw", 8))
    c = Ctx(dev)
    a = operands(c, x, 1, 1)
    for k_ in ("dAB", "dpar"):
        a[k_] = c.out(a[k_].shape)                                     # NaN-filled: any write shows
    if form.startswith("partp"):
        x8 = small_case(8)
        build_part(c, dev, a, x8, (x8["idx"] >= 0).astype(F32))
        a.update(dz_rec=c.out((64, x["hw"])), dz_rows=64)
    a.update(ws=c.out(4096), ws_floats=4096)
    over = dict(over)
    over.pop("hw", None)
    assert launch(c, form, a, **over) == code
    assert all(untouched(a[k_]) for k_ in ("dAB", "dpar", "dex", "ws")) and (a["dz_rec"] is None or untouched(a["dz_rec"]))
    c.inputs_intact()


@pytest.mark.gpu
def test_forward_and_topk_refusals_and_empties_write_nothing(dev):
    g = build_graph(N0, False)
    x = fwd_inputs(g, 16, 16)
    c = Ctx(dev)
    N, E = g["N"], g["E"]
    p, ex = c.out(E), c.out(E)
    base = dict(AB=c.inp(x["AB"]), xp=c.inp(x["xp"]), N=N, h=16, hw=16, erow=c.inp(x["erow"]), col=c.inp(x["col"]), E=E, deg=c.inp(x["deg"]),
                ex_in=c.inp(x["ex_in"]), ex_mode=1, t=-1.0, wdu=c.inp(x["wdu"]), wdv=c.inp(x["wdv"]), wex=c.inp(x["wex"]), b1=c.inp(x["b1"]),
                w2=c.inp(x["w2"]), b2=c.inp(x["b2"]), act=1, p=p, ex=ex)
    for over, code in ((dict(ex_mode=-1), ERR_ARG), (dict(ex_mode=3), ERR_ARG), (dict(ex_in=None), ERR_ARG), (dict(ex_mode=2, xp=None), ERR_ARG),
                       (dict(wex=None), ERR_ARG), (dict(ex_mode=2, wex=None), ERR_ARG), (dict(wdu=None), ERR_ARG), (dict(wdv=None), ERR_ARG), (dict(E=0), 0)):
        assert c.call("dgg_edge_mlp_fwd", *dict(base, **over).values()) == code, over
        assert untouched(p) and untouched(ex), over
    K = 7
    outs = [c.out((N, K), np.int32), c.out((N, K)), c.out((N, K), np.int32)]
    tb = dict(p=c.inp(rank_values(g)), N=N, row0=0, row1=N, rowptr=c.inp(g["rowptr"]), col=c.inp(g["col"]), mode=1, G=c.inp(noise_matrix(N)), ldG=N + 3,
              s0=1, s1=2, K=K, idx=outs[0], val=outs[1], eid=outs[2])
    for over, code in ((dict(K=0), ERR_UNSUPPORTED), (dict(K=65), ERR_UNSUPPORTED), (dict(G=None), ERR_ARG), (dict(mode=4), ERR_UNSUPPORTED),
                       (dict(mode=-1), ERR_UNSUPPORTED), (dict(row0=5, row1=4), ERR_ARG), (dict(row1=N + 1), ERR_ARG), (dict(row0=-1), ERR_ARG),
                       (dict(row0=9, row1=9), 0)):
        assert c.call("dgg_edgelist_topk_p_rows", *dict(tb, **over).values()) == code, over
        assert all(untouched(o) for o in outs), over
    whole = {k_: v for k_, v in tb.items() if k_ not in ("row0", "row1")}
    for over, code in ((dict(K=65), ERR_UNSUPPORTED), (dict(G=None), ERR_ARG), (dict(N=0), 0)):
        assert c.call("dgg_edgelist_topk_p", *dict(whole, **over).values()) == code, over
        assert all(untouched(o) for o in outs), over
    c.inputs_intact()


# ---------------------------------------------------------------------------------------------------------------
# tier 2 on the GPU
# ---------------------------------------------------------------------------------------------------------------
def t2_rows(name, got, ref, cpus, more):
    """the rows of the table: bar = 4 x the largest float32 error on the CPU -- row order, the seeded shuffle and, for the sums the GPU
    adds by atomics, the NDRAW further orders (cpu_more)"""
    rows = [figures("%s %s" % (name, k_), got[k_], ref[k_], [q[k_] for q in cpus]) for k_ in OUTS]
    den = ref["abs_ds"] if ref["abs_ds"] > 0 else 1.0
    rows.append(dict(out=name + " db2", cpu_row=abs(float(cpus[0]["db2"]) - ref["db2"]) / den, cpu_shuf=abs(float(cpus[1]["db2"]) - ref["db2"]) / den,
                     gpu=abs(float(got["db2"]) - ref["db2"]) / den))
    for r in rows:
        r["cpu_more"] = more.get(r["out"].split()[-1], 0.0)
        r["bar"] = 4 * max(r["cpu_row"], r["cpu_shuf"], r["cpu_more"])
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", T2_CASES, ids=["%s-hw%d-a%d-p%d-ex%d-deg%d" % c for c in T2_CASES])
def test_backward_within_four_times_the_float32_restatement(dev, case):
    form, hw, act, perturb, ex_mode, use_deg = case
    shape, K = T2_FORMS[form]
    form = form.split("-")[0]                                          # (bwd-csr: the atomic form on the CSR pattern)
    x = t2_case(shape, K, hw, act, perturb, ex_mode, use_deg)
    c, bad = Ctx(dev), []
    a = operands(c, x, act, perturb, use_deg, True, True)
    if form == "det":
        nws = 37 * (5 * hw + 2)
        a.update(ws=c.out(nws), ws_floats=nws)
    if form.startswith("partp"):
        w = (x["idx"] >= 0).astype(F32)
        ws, nrec = build_part(c, dev, a, x, w)
        nrows = nrec if hw != 64 else nrec // 2
        a.update(dz_rec=c.out((nrec, hw)), dz_rows=nrows)
    assert launch(c, form, a) == 0
    dAB, dpar, dex = a["dAB"].read("dAB"), a["dpar"].read("dpar"), a["dex"].read("dex")
    r0, r1 = x["row0"], x["row0"] + x["rows"]
    f = flat(x)
    deg = x["deg"] if use_deg else None
    ref = restate_edge_mlp_bwd(np.float64, f, x["ncols"], hw, x["AB"], deg, x["P"], act, perturb)
    groups = None if form == "det" else (f["u"] - r0) // 4          # (one workgroup per four rows: every block here has fewer than 4096 rows)
    cpus = [restate_edge_mlp_bwd(np.float32, f, x["ncols"], hw, x["AB"], deg, x["P"], act, perturb, perm, groups, keep=True)
            for perm in orders(len(f["u"]), hw)]
    more = further_orders(cpus[0]["terms"], ref, x["ncols"], seed=hw)
    # entries of neither side are left out: the A halves outside the rows are untouched zeros of the start pattern on both sides
    outside = np.ones(x["ncols"], bool)
    outside[r0:r1] = False
    excluded = int((~np.isfinite(dAB)).sum() + (~np.isfinite(dpar)).sum() + (~np.isfinite(dex)).sum()) + int(np.abs(dAB[outside, :hw]).sum() != 0) + \
        int(len(f["u"]) != int((x["idx"] >= 0).sum()) if x["rowptr"] is None else 0)
    assert excluded == 0, "%d elements were left out of the comparison" % excluded
    got = dict(dA=dAB[:, :hw], dB=dAB[:, hw:], dex=dex.ravel(), db2=dpar[5 * hw], **{k_: dpar[q * hw:(q + 1) * hw] for q, k_ in enumerate(OUTS[3:])})
    hold(t2_rows("%s %s hw=%d act=%d perturb=%d ex=%d deg=%d" % (form, shape, hw, act, perturb, ex_mode, use_deg), got, ref, cpus, more), bad)
    c.inputs_intact()
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    if "--grid-child" in sys.argv:
        sys.exit(_grid_child())
